"""CPU-side checks of the key generation exports on a host-only ctx: h2r_keygen_vk_repr against the hashlib model
(tests/keygen_ref.py) in both representations, on edge configurations and on digests where a wide reduction goes wrong; every serialised
field and every byte of every commitment reaches the digest; every refusal of the three entry points next to a valid twin that ends in
H2R_E_UNSUPPORTED (the last check: a host-only ctx does no device work); the packaged delta of every field against the model's."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import keygen_ref as KR
import permutation_ref as PR
import prover_chain_ref as CR
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
from test_transcript_host import host_ctx
from transcript_ref import Q, R, to_repr

NULL, SHAPE, UNSUP = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED
BASE = 0x100000                                  # never dereferenced: the checks are host arithmetic on the addresses
REPRS, IDS = [False, True], ["canonical", "montgomery"]
FIELD = "bn254_fr"
ARGS = ("field", "log_n", "blinding_factors", "num_fixed", "column_src", "chunk_len", "lookup_mask", "gate_fixed", "lookup_advice", "lookup_tag",
        "lookup_enable", "table_tag", "table_value", "omega", "delta", "extended_k", "points")


def points_of(rng, count, bound=Q):
    return [(rng.randrange(bound), rng.randrange(bound)) for _ in range(count)]


def model9(rng, bound=Q):
    """message()'s arguments of the k = 9 model circuit's configuration with synthetic commitments, as a dict."""
    cfg = CR.config(R, 9)
    return dict(zip(ARGS, KR.config_args(FIELD, cfg, R, points_of(rng, cfg.num_fixed + cfg.m + 1, bound))))


def struct_of(a, montgomery):
    cfg = _lib.H2RVerifyScalarsConfig(struct_size=ctypes.sizeof(_lib.H2RVerifyScalarsConfig), log_n=a["log_n"], blinding_factors=a["blinding_factors"],
                                      num_fixed=a["num_fixed"], num_columns=len(a["column_src"]), chunk_len=a["chunk_len"], lookup_mask=a["lookup_mask"])
    for name in ("omega", "delta"):
        v = to_repr(a[name], R, montgomery)
        getattr(cfg, name)[:] = [(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    for name in ("gate_fixed", "column_src", "lookup_advice", "lookup_tag", "lookup_enable"):
        for i, v in enumerate(a[name]):
            getattr(cfg, name)[i] = v
    cfg.table_tag, cfg.table_value = a["table_tag"], a["table_value"]
    return cfg


def point_bytes(points, montgomery):
    return b"".join(to_repr(v, Q, montgomery).to_bytes(32, "little") for xy in points for v in xy)


def call(ctx, a, montgomery, cfg=None, points=None):
    """(code, the integer in the ctx's representation)."""
    out = (ctypes.c_uint64 * 4)()
    cfg = struct_of(a, montgomery) if cfg is None else cfg
    rc = lib().h2r_keygen_vk_repr(ctx, ctypes.byref(cfg), a["extended_k"], point_bytes(a["points"], montgomery) if points is None else points, out)
    return rc, sum(int(out[k]) << (64 * k) for k in range(4))


def lib_value(ctx, a, montgomery):
    rc, v = call(ctx, a, montgomery)
    assert rc == 0
    return v


@pytest.fixture(scope="module", params=REPRS, ids=IDS)
def ctx(request):
    c = host_ctx(request.param)
    c.montgomery = request.param
    yield c
    lib().h2r_ctx_destroy(c)


def test_the_model_is_hashlib_over_the_stated_bytes():
    """A pin of the MODEL alone: the byte layout DESIGN states."""
    a = model9(random.Random("keygen/host/layout"))
    msg = KR.message(**a)
    assert len(msg) == 130 + 64 * 21 and msg[:4] == bytes(4) and msg[4:8] == bytes([9, 0, 0, 0]) and msg[12:16] == bytes([15, 0, 0, 0]) and msg[16:20] == bytes([5, 0, 0, 0])
    assert msg[28:36] == bytes([0, 1, 2, 3, 4, 0, 0, 0]) and msg[36:45] == bytes(range(9)) and msg[45:50] == bytes([0, 1, 2, 3, 0])
    assert msg[50:55] == bytes([11] * 4 + [13]) and msg[55:60] == bytes([12] * 4 + [14]) and msg[60:62] == bytes([9, 10])
    assert msg[62:94] == a["omega"].to_bytes(32, "little") and msg[94:126] == a["delta"].to_bytes(32, "little") and msg[126:130] == bytes([12, 0, 0, 0])
    assert msg[130:162] == a["points"][0][0].to_bytes(32, "little") and msg[-32:] == a["points"][-1][1].to_bytes(32, "little")
    assert len(KR.PERSON) == 16 and KR.vk_repr(R, **a) < R


def test_the_k9_configuration_is_the_model(ctx):
    a = model9(random.Random("keygen/host/k9"))
    assert lib_value(ctx, a, ctx.montgomery) == to_repr(KR.vk_repr(R, **a), R, ctx.montgomery)


def test_both_representations_give_one_integer():
    a = model9(random.Random("keygen/host/reprs"))
    ca, cb = host_ctx(False), host_ctx(True)
    va, vb = lib_value(ca, a, False), lib_value(cb, a, True)
    assert va == KR.vk_repr(R, **a) and vb == va * (1 << 256) % R
    lib().h2r_ctx_destroy(ca)
    lib().h2r_ctx_destroy(cb)


def test_edge_configurations(ctx):
    rng = random.Random("keygen/host/edges")
    for F, src in ((0, (0, 1, 2, 3, 4)), (15, (3,)), (0, (4,)), (16, (4, 2, 0, 1, 3)), (15, (4, 2, 0))):
        a = model9(rng)
        a.update(num_fixed=F, column_src=list(src), points=points_of(rng, F + len(src) + 1))
        assert lib_value(ctx, a, ctx.montgomery) == to_repr(KR.vk_repr(R, **a), R, ctx.montgomery), (F, src)
    a = model9(rng)
    a.update(points=[(0, 0)] * 21, blinding_factors=2 ** 32 - 1, chunk_len=2 ** 32 - 1, lookup_mask=2 ** 32 - 1, gate_fixed=[255] * 9, table_tag=255, extended_k=27)
    assert lib_value(ctx, a, ctx.montgomery) == to_repr(KR.vk_repr(R, **a), R, ctx.montgomery)


def test_the_wide_reduce_on_crafted_digests(ctx):
    """Keys found by search (G's abscissa counts up) whose digest halves d0 + 2^256 d1 sit where a reduction goes wrong: both halves >= r,
    both < r, either half within 2^-16 of 2^256 or below 2^240."""
    a = model9(random.Random("keygen/host/crafted"))
    a.update(num_fixed=0, column_src=[0], points=[(1, 2), (0, 3)])
    prefix = KR.message(**a)[:-64]
    want = {"both>=r": lambda d0, d1: d0 >= R and d1 >= R, "both<r": lambda d0, d1: d0 < R and d1 < R,
            "d1 top ones": lambda d0, d1: d1 >> 240 == 0xFFFF, "d1 top zeros": lambda d0, d1: d1 >> 240 == 0,
            "d0 top ones": lambda d0, d1: d0 >> 240 == 0xFFFF, "d0 top zeros": lambda d0, d1: d0 >> 240 == 0}
    found = {}
    tail = (3).to_bytes(32, "little")
    for x in range(1 << 21):
        d = KR.digest(prefix + x.to_bytes(32, "little") + tail)
        d0, d1 = int.from_bytes(d[:32], "little"), int.from_bytes(d[32:], "little")
        for name, pred in want.items():
            if name not in found and pred(d0, d1):
                found[name] = x
        if len(found) == len(want):
            break
    assert len(found) == len(want), found
    for x in found.values():
        a["points"][1] = (x, 3)
        d = int.from_bytes(KR.digest(KR.message(**a)), "little")
        assert KR.vk_repr(R, **a) == d % R != d % (1 << 256) % R
        assert lib_value(ctx, a, ctx.montgomery) == to_repr(d % R, R, ctx.montgomery)


def test_every_field_and_every_commitment_byte_reaches_the_digest():
    rng = random.Random("keygen/host/fields")
    c = host_ctx(False)
    a = model9(rng, bound=1 << 248)              # (a flipped bit of the top byte stays below q)
    seen = {lib_value(c, a, False)}
    count = 1

    def changed(**kw):
        nonlocal count
        b = dict(a)
        b.update(kw)
        v = lib_value(c, b, False)
        assert v == KR.vk_repr(R, **b), kw
        seen.add(v)
        count += 1

    for name in ("log_n", "blinding_factors", "num_fixed", "chunk_len", "lookup_mask", "table_tag", "table_value", "extended_k"):
        if name == "num_fixed":
            changed(num_fixed=14, points=a["points"][1:])
            changed(num_fixed=14, points=a["points"][:-2] + a["points"][-1:])
        else:
            changed(**{name: a[name] + 1})
    for name in ("column_src", "gate_fixed", "lookup_advice", "lookup_tag", "lookup_enable"):
        for i in range(len(a[name])):
            v = list(a[name])
            v[i] = (v[i] + 1) % 5 if name == "column_src" else v[i] ^ 0x80
            changed(**{name: v})
    changed(column_src=[0, 1, 2, 3], points=a["points"][:19] + a["points"][20:])      # one column less: its commitment leaves with it
    changed(omega=a["omega"] ^ 1)
    changed(delta=a["delta"] ^ (1 << 200))
    for i in range(len(a["points"])):
        for j in range(2):
            for byte in range(32):
                pts = [list(p) for p in a["points"]]
                pts[i][j] ^= 1 << (8 * byte)
                changed(points=[tuple(p) for p in pts])
    assert len(seen) == count and count > 21 * 64
    # the field index: a field with a curve is the only one served, so the model alone shows it in the bytes
    assert KR.message(**dict(a, field=1))[:4] == bytes([1, 0, 0, 0])
    lib().h2r_ctx_destroy(c)


def test_vk_repr_refusals(ctx):
    a = model9(random.Random("keygen/host/refusals"))
    cfg, pts, out = struct_of(a, ctx.montgomery), point_bytes(a["points"], ctx.montgomery), (ctypes.c_uint64 * 4)()
    f = lib().h2r_keygen_vk_repr
    assert f(ctx, ctypes.byref(cfg), 12, pts, out) == 0
    assert f(None, ctypes.byref(cfg), 12, pts, out) == NULL and f(ctx, None, 12, pts, out) == NULL
    assert f(ctx, ctypes.byref(cfg), 12, None, out) == NULL and f(ctx, ctypes.byref(cfg), 12, pts, None) == NULL
    bad = struct_of(a, ctx.montgomery)
    bad.struct_size -= 4
    assert f(ctx, ctypes.byref(bad), 12, pts, out) == UNSUP
    for ext in (8, 28):
        assert f(ctx, ctypes.byref(cfg), ext, pts, out) == SHAPE
    raw = lambda v: [(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    for name, value, ext in (("log_n", 0, 12), ("log_n", 25, 27), ("num_fixed", 17, 12), ("num_columns", 0, 12), ("num_columns", 9, 12),
                             ("column_src", 5, 12), ("omega", raw(R), 12), ("delta", raw(R + 5), 12)):
        bad = struct_of(a, ctx.montgomery)
        if name == "column_src":
            bad.column_src[1] = value
        elif name in ("omega", "delta"):
            getattr(bad, name)[:] = value
        else:
            setattr(bad, name, value)
        assert f(ctx, ctypes.byref(bad), ext, pts, out) == SHAPE, (name, value)
    assert f(ctx, ctypes.byref(cfg), 12, pts[:32] + Q.to_bytes(32, "little") + pts[64:], out) == SHAPE          # a coordinate >= q
    for field in ("bn254_fq", "pasta_fp", "pasta_fq"):                                                         # no curve: no coordinates' field
        c = host_ctx(False, field)
        assert f(c, ctypes.byref(cfg), 12, pts, out) == UNSUP
        lib().h2r_ctx_destroy(c)


# ---- the two device entry points: the refusals ----------------------------------------------------------------------------------------------
def lookup_cfg(ctx):
    cfg = _lib.H2RLookupConfig()
    assert lib().h2r_lookup_config_default(ctx, 0, ctypes.byref(cfg)) == 0
    return cfg


def fixed_call(ctx, cfg=True, kinds=BASE, rows=100, first_row=0, log_n=10, usable=1018, out=BASE + 0x100000, col_stride=1024 * 32, status=BASE + 0x10,
               ws=BASE + 0x800000, layout=None):
    lc = lookup_cfg(ctx) if cfg is True else cfg
    return lib().h2r_keygen_fixed_columns(ctx, ctypes.byref(lc) if lc is not None else None, layout, kinds, rows, first_row, log_n, usable, out, col_stride,
                                          status, ws, None)


def test_fixed_columns_refusals(ctx):
    assert fixed_call(ctx) == UNSUP and fixed_call(ctx, rows=0, kinds=None) == UNSUP and fixed_call(ctx, first_row=918) == UNSUP
    assert lib().h2r_keygen_fixed_columns(None, None, None, None, 0, 0, 10, 1018, None, 0, None, None, None) == NULL
    for kw in (dict(cfg=None), dict(kinds=None), dict(out=None), dict(status=None), dict(ws=None)):
        assert fixed_call(ctx, **kw) == NULL, kw
    lc = lookup_cfg(ctx)
    n_rows = lc.n_rows
    for kw in (dict(log_n=0), dict(log_n=25, usable=1018), dict(usable=0), dict(usable=1024), dict(first_row=919), dict(rows=1019), dict(usable=n_rows - 1, rows=1),
               dict(col_stride=1024 * 32 - 32), dict(col_stride=1024 * 32 + 8), dict(out=BASE + 0x100008)):
        assert fixed_call(ctx, **kw) == SHAPE, kw
    assert fixed_call(ctx, usable=n_rows, rows=1) == UNSUP                                  # a table that just fits
    lc.n_rows = 0
    assert fixed_call(ctx, cfg=lc) == SHAPE and lib().h2r_keygen_fixed_workspace_bytes(ctypes.byref(lc)) == 0
    assert lib().h2r_keygen_fixed_workspace_bytes(None) == 0
    assert lib().h2r_keygen_fixed_workspace_bytes(ctypes.byref(lookup_cfg(ctx))) >= 256 * 13 * 32 + 8 * n_rows
    lay = _lib.H2RAdviceLayout()
    assert lib().h2r_advice_layout_default(ctypes.byref(lay)) == 0 and fixed_call(ctx, layout=ctypes.byref(lay)) == UNSUP
    lay.column_of[7][0] = 1                                                                # no permutation
    assert fixed_call(ctx, layout=ctypes.byref(lay)) == SHAPE


def sigma_call(ctx, column_src=(0, 1, 2, 3, 4), copies=BASE, n_copies=50, first_row=0, log_n=10, usable=1018, out=BASE + 0x100000, col_stride=1024 * 32,
               status=BASE + 0x10, ws=BASE + 0x800000, n_extra=0, struct_size=None, delta=None, omega=None, null_cfg=False, info_size=None):
    cfg = _lib.H2RPermutationConfig(struct_size=ctypes.sizeof(_lib.H2RPermutationConfig) if struct_size is None else struct_size, chunk_len=2,
                                    num_columns=len(column_src), n_extra=n_extra)
    for c, s in enumerate(column_src[:8]):
        cfg.column_src[c] = s
    om = PR.domain(R, log_n)[0] if 0 < log_n <= 28 else 1
    for name, v in (("delta", _lib.FIELD_DELTA[FIELD] if delta is None else delta), ("omega", om if omega is None else omega)):
        v = to_repr(v, R, ctx.montgomery) if v < R else v
        getattr(cfg, name)[:] = [(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    info = _lib.H2RKeygenSigmaInfo(struct_size=ctypes.sizeof(_lib.H2RKeygenSigmaInfo) if info_size is None else info_size)
    return lib().h2r_keygen_sigma_columns(ctx, None if null_cfg else ctypes.byref(cfg), copies, n_copies, first_row, log_n, usable, out, col_stride, status, ws,
                                          ctypes.byref(info), None)


def test_sigma_columns_refusals(ctx):
    assert sigma_call(ctx) == UNSUP and sigma_call(ctx, n_copies=0, copies=None) == UNSUP and sigma_call(ctx, column_src=(4, 2, 0)) == UNSUP
    assert sigma_call(ctx, column_src=tuple(range(8)), n_extra=3) == UNSUP       # (extra columns: no pair names them)
    assert sigma_call(ctx, column_src=(3,)) == UNSUP and sigma_call(ctx, log_n=1, usable=1, col_stride=64) == UNSUP
    for kw in (dict(null_cfg=True), dict(copies=None), dict(out=None), dict(status=None), dict(ws=None)):
        assert sigma_call(ctx, **kw) == NULL, kw
    assert sigma_call(ctx, struct_size=8) == UNSUP and sigma_call(ctx, info_size=8) == UNSUP
    for kw in (dict(column_src=()), dict(column_src=(0,) * 9), dict(column_src=(0, 8)), dict(column_src=(0, 1, 0)), dict(column_src=(5, 5)), dict(log_n=0), dict(log_n=25),
               dict(usable=0), dict(usable=1024), dict(delta=R), dict(omega=R + 1), dict(omega=PR.domain(R, 9)[0]), dict(omega=1), dict(n_copies=2 ** 31 + 1),
               dict(col_stride=1024 * 32 - 32), dict(col_stride=1024 * 32 + 8), dict(out=BASE + 8), dict(ws=BASE + 4), dict(copies=BASE + 4)):
        assert sigma_call(ctx, **kw) == SHAPE, kw
    w = lib().h2r_keygen_sigma_workspace_bytes
    assert w(0, 5, 10) == 0 and w(25, 5, 10) == 0 and w(10, 0, 10) == 0 and w(10, 9, 10) == 0 and w(10, 5, 2 ** 31 + 1) == 0
    assert w(10, 5, 0) >= 2 * 4 * 5 * 1024 and w(10, 5, 100) >= w(10, 5, 0) + 4 * 4 * 200 and w(10, 5, 10 ** 6) == w(10, 5, 5 * 512)
    assert w(17, 5, 400000) < 64 << 20


@pytest.mark.parametrize("field", sorted(_lib.FIELD_DELTA))
def test_the_packaged_delta_is_the_models(field):
    from pyref import FIELD_MODULI
    P = FIELD_MODULI[field]
    two_adicity = ((P - 1) & -(P - 1)).bit_length() - 1
    for k in {1, min(9, two_adicity), min(17, two_adicity), two_adicity}:
        assert _lib.FIELD_DELTA[field] == PR.domain(P, k)[1]
    assert sorted(_lib.FIELD_DELTA) == sorted(_lib.FIELDS)
