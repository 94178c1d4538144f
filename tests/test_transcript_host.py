"""CPU-side checks of the transcript exports on a host-only ctx: every refusal of h2r_transcript_round next to a
valid twin that ends in H2R_E_UNSUPPORTED (its last check), and the host twin h2r_transcript_eval -- the very functions the kernel inlines
-- byte for byte against the plain model (tests/transcript_ref.py: hashlib and Python integers) on the smallest inputs where a streaming
BLAKE2b goes wrong.  Of a state record the model knows the byte counter, the fill and the pending block bytes; the chaining value h has no
counterpart in hashlib and is pinned through every later challenge."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transcript_ref as T
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib

Q, R = T.Q, T.R
NULL, SHAPE, UNSUP, ASSERTION = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED, _lib.H2R_E_ASSERTION
BASE = 0x100000                                  # never dereferenced: the checks are host arithmetic on the addresses
OMEGA17 = pow(7, (R - 1) >> 17, R)               # a 2^17-th root of unity of Fr
REPRS, IDS = [False, True], ["canonical", "montgomery"]


def host_ctx(montgomery=False, field="bn254_fr"):
    ctx = ctypes.c_void_p()
    p = H2RParams(64, 256, _lib.FIELDS[field], -1)
    if montgomery:
        rep = _lib.H2RAdviceRepr()
        rep.struct_size, rep.flags = ctypes.sizeof(rep), _lib.H2R_ADVICE_MONTGOMERY
        assert lib().h2r_ctx_create_ex(ctypes.byref(p), ctypes.byref(rep), ctypes.byref(ctx)) == 0
    else:
        assert lib().h2r_ctx_create(ctypes.byref(p), ctypes.byref(ctx)) == 0
    return ctx


@pytest.fixture(scope="module", params=REPRS, ids=IDS)
def twin(request):
    t = Twin(request.param)
    yield t
    lib().h2r_ctx_destroy(t.ctx)


class Twin:
    """One circuit's transcript run by h2r_transcript_eval, next to the model's."""

    def __init__(self, montgomery):
        self.montgomery, self.ctx = montgomery, host_ctx(montgomery)
        self.nbytes = lib().h2r_transcript_state_bytes()

    def new(self):
        self.state = (ctypes.c_uint8 * self.nbytes)(*([0xAB] * self.nbytes))
        assert lib().h2r_transcript_eval(self.ctx, 0, self.state, None, 0, None) == 0
        self.model = T.Transcript()
        return self

    def absorb(self, items):
        raw = b"".join(bytes([1 if k == "point" else 2]) + T.item_repr_bytes(k, v, self.montgomery) for k, v in items)
        before = bytes(self.state)
        rc = lib().h2r_transcript_eval(self.ctx, 1, self.state, raw, len(raw), None)
        st, _, _ = self.model.round(items, common=True)
        assert rc == st, (rc, st)
        if rc:
            assert bytes(self.state) == before, "a status leaves the state untouched"
        self.check_state()
        return rc

    def squeeze(self):
        out = (ctypes.c_uint64 * 4)()
        assert lib().h2r_transcript_eval(self.ctx, 2, self.state, None, 0, out) == 0
        got, want = sum(int(out[k]) << (64 * k) for k in range(4)), self.model.squeeze()
        assert got == T.to_repr(want, R, self.montgomery), (self.model.absorbed, got, want)
        self.check_state()
        return want

    def check_state(self):
        raw = bytes(self.state)
        done, block = self.model.pending()
        assert int.from_bytes(raw[64:72], "little") == done and int.from_bytes(raw[72:80], "little") == len(block)
        assert raw[80:80 + len(block)] == block

    def derive(self, c, mult, log2_pow):
        out = (ctypes.c_uint64 * 4)()
        raw = b"".join(T.to_repr(v, R, self.montgomery).to_bytes(32, "little") for v in (c, mult)) + log2_pow.to_bytes(4, "little")
        assert lib().h2r_transcript_eval(self.ctx, 3, None, raw, len(raw), out) == 0
        return T.from_repr(sum(int(out[k]) << (64 * k) for k in range(4)), R, self.montgomery)

    def encode(self, kind, v):
        out = (ctypes.c_uint64 * 4)()
        raw = T.item_repr_bytes(kind, v, self.montgomery)
        rc = lib().h2r_transcript_eval(self.ctx, 4 if kind == "point" else 5, None, raw, len(raw), out)
        return rc, bytes(out)


# ---- the host twin against the model -----------------------------------------------------------------------------------------------------
def test_one_point_then_squeezes_cross_the_first_block(twin):
    """65 bytes, then one byte per squeeze: the 62nd, 63rd and 64th challenges are finalised on 127, 128 and 129 bytes."""
    t = twin.new()
    t.absorb([("point", (1, 2))])
    sizes = []
    for _ in range(72):
        t.squeeze()
        sizes.append(t.model.absorbed)
    assert sizes[61:64] == [127, 128, 129]


def test_three_points_then_squeezes_cross_the_second_block(twin):
    """195 bytes: the 60th to 62nd challenges are finalised on 255, 256 and 257 bytes."""
    t = twin.new()
    t.absorb([("point", (Q - 1, 3)), ("point", (5, Q - 1)), ("point", (0, 1))])
    sizes = []
    for _ in range(66):
        t.squeeze()
        sizes.append(t.model.absorbed)
    assert sizes[59:62] == [255, 256, 257]


def test_items_that_straddle_and_that_end_on_the_boundary(twin):
    t = twin.new()
    t.absorb([("scalar", 0), ("scalar", 1), ("scalar", R - 1)])
    t.squeeze()
    assert t.model.absorbed == 100
    t.absorb([("point", (Q - 1, Q - 2))])                  # bytes 100..164: over the boundary at 128
    assert t.model.pending()[0] == 128
    for _ in range(58):
        t.squeeze()
    t.absorb([("scalar", R - 1)])                          # ends exactly on 256: the second block is full and waits
    assert t.model.absorbed == 256 and t.model.pending() == (128, t.model.tail[128:])
    t.squeeze()
    t.absorb([("scalar", 3), ("point", (2, 5))])
    t.squeeze()


def test_a_squeeze_is_the_first_operation(twin):
    t = twin.new()
    first = t.squeeze()
    h = T.new_hash()
    h.update(b"\x00")
    assert first == int.from_bytes(h.digest(), "little") % R
    t.squeeze()
    t.absorb([("scalar", first)])
    t.squeeze()


def test_edge_values_and_statuses(twin):
    t = twin.new()
    for v in (0, 1, Q - 1):
        for y in (1, 2, Q - 1, Q - 2):                     # a y of either parity
            t.absorb([("point", (v, y))])
            rc, enc = t.encode("point", (v, y))
            assert rc == 0 and enc == T.proof_bytes("point", (v, y)) and enc[31] >> 7 == y & 1
    for s in (0, 1, R - 1):
        t.absorb([("scalar", s)])
        assert t.encode("scalar", s) == (0, s.to_bytes(32, "little"))
    t.squeeze()
    for bad, want in (([("point", (Q, 1))], SHAPE), ([("point", (1, Q))], SHAPE), ([("point", (1, (1 << 256) - 1))], SHAPE),
                      ([("scalar", R)], SHAPE), ([("scalar", (1 << 256) - 1)], SHAPE), ([("point", (0, 0))], ASSERTION),
                      ([("scalar", 1), ("point", (0, 0)), ("scalar", R)], ASSERTION), ([("scalar", 1), ("scalar", R), ("point", (0, 0))], SHAPE)):
        assert t.absorb(bad) == want                       # ... and the state is as it was (Twin.absorb)
        assert t.encode(*bad[-1])[0] == T.item_status(*bad[-1])
    t.squeeze()
    # a list that does not parse
    for raw in (b"\x03" + bytes(32), b"\x02" + bytes(31), b"\x01" + bytes(32), b"\x00"):
        assert lib().h2r_transcript_eval(t.ctx, 1, t.state, raw, len(raw), None) == SHAPE
    assert lib().h2r_transcript_eval(t.ctx, 6, t.state, b"", 0, None) in (SHAPE, NULL)
    assert lib().h2r_transcript_eval(t.ctx, 2, None, None, 0, (ctypes.c_uint64 * 4)()) == NULL
    assert lib().h2r_transcript_eval(None, 0, t.state, None, 0, None) == NULL


def test_random_mixed_item_lists(twin):
    rng = random.Random("transcript/host/random/%d" % twin.montgomery)
    t = twin.new()
    for _ in range(40):
        items = []
        for _ in range(rng.randrange(0, 5)):
            if rng.randrange(2):
                items.append(("point", (rng.randrange(Q), rng.randrange(Q))))
            else:
                items.append(("scalar", rng.randrange(R)))
        if items:
            t.absorb(items)
        for _ in range(rng.randrange(0, 3)):
            t.squeeze()


def test_derived_values(twin):
    t = twin.new()
    t.absorb([("scalar", 11)])
    for c in (t.squeeze(), 0, 1, R - 1):
        for log2_pow in (0, 1, 17):
            for mult in (1, OMEGA17, R - 1, 0):
                assert twin.derive(c, mult, log2_pow) == mult * pow(c, 1 << log2_pow, R) % R
    raw = bytes(64) + (25).to_bytes(4, "little")
    assert lib().h2r_transcript_eval(twin.ctx, 3, None, raw, len(raw), (ctypes.c_uint64 * 4)()) == SHAPE    # log2_pow > 24
    raw = R.to_bytes(32, "little") + bytes(32) + bytes(4)
    assert lib().h2r_transcript_eval(twin.ctx, 3, None, raw, len(raw), (ctypes.c_uint64 * 4)()) == SHAPE


def test_a_field_without_a_curve_is_refused():
    ctx = host_ctx(field="bn254_fq")
    state = (ctypes.c_uint8 * lib().h2r_transcript_state_bytes())()
    assert lib().h2r_transcript_eval(ctx, 0, state, None, 0, None) == UNSUP
    lib().h2r_ctx_destroy(ctx)


# ---- h2r_transcript_round's refusals -----------------------------------------------------------------------------------------------------
SB = None


def _cfg(num_items=2, num_squeeze=2, num_derive=1, flags=_lib.H2R_TRANSCRIPT_INIT, reserved=0, struct_size=None):
    cfg = _lib.H2RTranscriptConfig()
    cfg.struct_size = ctypes.sizeof(cfg) if struct_size is None else struct_size
    cfg.num_items, cfg.num_squeeze, cfg.num_derive, cfg.flags, cfg.reserved = num_items, num_squeeze, num_derive, flags, reserved
    return cfg


def _items(*specs):
    arr = (_lib.H2RTranscriptItem * max(len(specs), 1))()
    for d, (base, stride, count, kind, flags) in zip(arr, specs):
        d.base, d.elem_stride, d.count, d.kind, d.flags = base, stride, count, kind, flags
    return arr


def _derive(src=0, mult=1, log2_pow=17):
    arr = (_lib.H2RTranscriptDerive * 1)()
    arr[0].src, arr[0].log2_pow = src, log2_pow
    for k in range(4):
        arr[0].mult[k] = (mult >> (64 * k)) & (2 ** 64 - 1)
    return arr


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_refusals_next_to_a_valid_twin(montgomery):
    """The valid twin reaches the last check (a host-only ctx: H2R_E_UNSUPPORTED); each refusal changes one thing."""
    ctx = host_ctx(montgomery)
    batch, sb = 3, lib().h2r_transcript_state_bytes()
    POINT, SCALAR, COMMON = _lib.H2R_TRANSCRIPT_POINT, _lib.H2R_TRANSCRIPT_SCALAR, _lib.H2R_TRANSCRIPT_COMMON
    # the layout: points [batch][5] written, one scalar shared and common; then states, challenges, derived, proof, status
    pts, sc = BASE, BASE + 0x1000
    states, ch, dv, proof, status = BASE + 0x2000, BASE + 0x3000, BASE + 0x4000, BASE + 0x5000, BASE + 0x6000
    stride = 256
    good = dict(cfg=_cfg(), items=_items((pts, 5 * 64, 5, POINT, 0), (sc, 0, 1, SCALAR, COMMON)), derive=_derive(mult=T.to_repr(OMEGA17, R, montgomery)),
                states=states, batch=batch, ch=ch, dv=dv, proof=proof, stride=stride, off=32, status=status)

    def call(ctx_=ctx, **kw):
        a = dict(good, **kw)
        return lib().h2r_transcript_round(ctx_, ctypes.byref(a["cfg"]) if a["cfg"] is not None else None, a["items"], a["derive"], a["states"], a["batch"],
                                          a["ch"], a["dv"], a["proof"], a["stride"], a["off"], a["status"], None)

    assert call() == UNSUP                                                    # the twin: everything but the device is right
    assert call(status=None) == UNSUP                                         # status is optional
    assert call(cfg=_cfg(flags=0)) == UNSUP
    assert call(cfg=_cfg(0, 1, 0), items=None, derive=None, dv=None, proof=None) == UNSUP   # a round that only squeezes
    assert call(cfg=_cfg(2, 0, 0), ch=None, dv=None, derive=None) == UNSUP                  # a round that only absorbs
    assert call(items=_items((pts, 5 * 64, 5, POINT, COMMON), (sc, 0, 1, SCALAR, COMMON)), proof=None) == UNSUP   # nothing written: no proof needed
    assert call(off=stride - 5 * 32) == UNSUP                                 # the round's bytes end exactly at the stride
    # NULL pointers come first
    assert call(ctx_=None) == NULL
    assert call(cfg=None) == NULL
    assert call(states=None) == NULL
    assert call(items=None) == NULL
    assert call(derive=None) == NULL
    assert call(ch=None) == NULL                                              # a squeeze count with nowhere to go
    assert call(dv=None) == NULL
    assert call(proof=None) == NULL                                           # a written item
    assert call(items=_items((None, 5 * 64, 5, POINT, 0), (sc, 0, 1, SCALAR, COMMON))) == NULL
    assert call(cfg=_cfg(reserved=1), states=None) == NULL
    # struct_size and flags before the shapes
    assert call(cfg=_cfg(struct_size=20)) == UNSUP and call(cfg=_cfg(struct_size=28, reserved=1)) == UNSUP
    assert call(cfg=_cfg(flags=2)) == UNSUP and call(cfg=_cfg(flags=3, num_squeeze=9)) == UNSUP
    # shapes: the counts, reserved, the items, the derived values
    many = _items(*[(pts, 0, 1, POINT, COMMON)] * 65)
    assert call(cfg=_cfg(num_items=65), items=many) == SHAPE and call(cfg=_cfg(num_items=64), items=many) == UNSUP
    assert call(cfg=_cfg(num_squeeze=9)) == SHAPE and call(cfg=_cfg(num_squeeze=8)) == UNSUP
    assert call(cfg=_cfg(num_derive=17)) == SHAPE
    assert call(cfg=_cfg(reserved=7)) == SHAPE
    for bad in ((pts, 5 * 64, 5, 0, 0), (pts, 5 * 64, 5, 3, 0), (pts, 5 * 64, 5, POINT, 2), (pts, 5 * 64, 0, POINT, 0),
                (pts, 0, _lib.H2R_TRANSCRIPT_MAX_COUNT + 1, POINT, COMMON)):
        assert call(items=_items(bad, (sc, 0, 1, SCALAR, COMMON))) == SHAPE, bad
    res = _items((pts, 5 * 64, 5, POINT, 0), (sc, 0, 1, SCALAR, COMMON))
    res[1].reserved = 1
    assert call(items=res) == SHAPE
    assert call(derive=_derive(src=2)) == SHAPE and call(derive=_derive(src=1)) == UNSUP
    assert call(derive=_derive(log2_pow=25)) == SHAPE and call(derive=_derive(log2_pow=24)) == UNSUP
    assert call(derive=_derive(mult=R)) == SHAPE
    # alignment and strides
    for k in ("states", "ch", "dv", "proof", "stride", "off"):
        assert call(**{k: good[k] + 8}) == SHAPE, k
    assert call(items=_items((pts + 8, 5 * 64, 5, POINT, 0), (sc, 0, 1, SCALAR, COMMON))) == SHAPE
    assert call(items=_items((pts, 5 * 64 + 8, 5, POINT, 0), (sc, 0, 1, SCALAR, COMMON))) == SHAPE
    assert call(items=_items((pts, 5 * 64 - 16, 5, POINT, 0), (sc, 0, 1, SCALAR, COMMON))) == SHAPE   # a stride smaller than the item
    assert call(items=_items((pts + 16, 5 * 64 + 16, 5, POINT, 0), (sc + 16, 0, 1, SCALAR, COMMON))) == UNSUP
    # the proof: the offset plus the round's bytes within the stride
    assert call(off=stride - 5 * 32 + 16) == SHAPE and call(stride=5 * 32 + 16) == SHAPE and call(stride=5 * 32 + 32) == UNSUP
    # batch 0
    assert call(batch=0) == SHAPE
    # overlaps: an output with an item, an output with an output; adjacent is not overlapping
    assert call(states=pts + batch * 5 * 64 - 16) == SHAPE and call(states=pts + batch * 5 * 64) == UNSUP
    assert call(ch=sc) == SHAPE and call(ch=sc + 16) == SHAPE and call(ch=sc + 32) == UNSUP
    assert call(dv=pts) == SHAPE
    assert call(proof=pts - 32 - 5 * 32 + 16) == SHAPE and call(proof=pts - 32 - (batch - 1) * stride - 5 * 32) == UNSUP
    assert call(status=sc + 31) == SHAPE and call(status=sc + 32) == UNSUP
    assert call(ch=states + batch * sb - 16) == SHAPE and call(ch=states + batch * sb) == UNSUP
    assert call(dv=ch + batch * 2 * 32 - 16) == SHAPE and call(dv=ch + batch * 2 * 32) == UNSUP
    assert call(proof=states) == SHAPE and call(status=dv + 16) == SHAPE
    lib().h2r_ctx_destroy(ctx)
    # a field without a curve: after the shape checks, before the host-only ctx (which every ctx here is)
    other = host_ctx(montgomery, "bn254_fq")
    assert call(ctx_=other, derive=_derive()) == UNSUP
    plain = dict(cfg=_cfg(2, 2, 0), derive=None, dv=None)
    assert call(ctx_=other, **plain) == UNSUP
    assert call(ctx_=other, batch=0, **plain) == SHAPE
    lib().h2r_ctx_destroy(other)
