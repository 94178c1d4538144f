"""CPU-side checks of the generator of the blinding values on a host-only ctx: the host twin h2r_random_eval -- the
very functions random_kernel inlines -- against hashlib (tests/create_proof_ref.py) on the seeds, circuits, rows and tags where a
hand-written BLAKE2b or a wide reduction goes wrong, and every refusal of h2r_random_columns next to a valid twin that ends in
H2R_E_UNSUPPORTED (its last check: a host-only ctx does no device work)."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
from test_transcript_host import host_ctx
from transcript_ref import R, to_repr

NULL, SHAPE, UNSUP = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED
BASE = 0x100000                                  # never dereferenced: the checks are host arithmetic on the addresses
SEEDS = [bytes(32), b"\xff" * 32, bytes(random.Random("random/host/seed").randrange(256) for _ in range(32))]
EDGES = [0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1]
REPRS, IDS = [False, True], ["canonical", "montgomery"]


@pytest.fixture(scope="module", params=REPRS, ids=IDS)
def ctx(request):
    c = host_ctx(request.param)
    c.montgomery = request.param
    yield c
    lib().h2r_ctx_destroy(c)


def eval_(ctx, seed, circuit, tag, row):
    out = (ctypes.c_uint64 * 4)()
    assert lib().h2r_random_eval(ctx, seed, circuit, tag, row, out) == 0
    return sum(int(out[k]) << (64 * k) for k in range(4))


def check(ctx, seed, circuit, tag, row):
    want = C.random_element(seed, circuit, tag, row)
    assert eval_(ctx, seed, circuit, tag, row) == to_repr(want, R, ctx.montgomery), (seed.hex(), circuit, tag, row)
    return want


def test_the_model_is_hashlib_over_the_stated_message():
    """A pin of the MODEL alone (it passes without the library): the 56 message bytes as DESIGN states them and the tag table.  The library
    is held to this model by every other test of the file."""
    seed = SEEDS[2]
    msg = C.message(seed, 0x0102030405060708, 0x0A0B0C0D, 0x1112131415161718)
    assert len(msg) == 56 and msg[:32] == seed and msg[32:40] == bytes(range(8, 0, -1)) and msg[40:48] == bytes([0x0D, 0x0C, 0x0B, 0x0A, 0, 0, 0, 0])
    assert msg[48:] == bytes(range(0x18, 0x10, -1))
    assert sorted(set(C.TAGS)) == C.TAGS and len(C.TAGS) == 29 and C.tag(C.KIND_RANDOM_POLY) == 0x500


@pytest.mark.parametrize("seed", SEEDS, ids=["zeros", "ones", "random"])
def test_eval_is_the_model_on_edge_circuits_and_rows(ctx, seed):
    values = [check(ctx, seed, circuit, C.tag(C.KIND_ADVICE, 1), row) for circuit in EDGES for row in EDGES]
    assert len(set(values)) == len(values) and all(v < R for v in values)


def test_eval_is_the_model_on_every_tag(ctx):
    values = [check(ctx, SEEDS[2], 3, t, 1018) for t in C.TAGS + [2 ** 32 - 1]]
    assert len(set(values)) == len(values)


def test_each_argument_reaches_the_message(ctx):
    base = (SEEDS[2], 1, 2, 3)
    seen = {check(ctx, *base)}
    for i in range(32):                                                      # every seed byte
        s = bytearray(SEEDS[2])
        s[i] ^= 0x80
        seen.add(check(ctx, bytes(s), 1, 2, 3))
    for circuit, tag, row in ((1 + 2 ** 63, 2, 3), (1, 2 + 2 ** 31, 3), (1, 2, 3 + 2 ** 63), (2, 1, 3), (1, 3, 2), (3, 2, 1)):
        seen.add(check(ctx, SEEDS[2], circuit, tag, row))
    assert len(seen) == 39


def test_the_wide_reduce_on_crafted_digests(ctx):
    """Rows found by search whose digest halves d0 + 2^256 d1 sit where a reduction goes wrong: both halves >= r, both < r, d1 within 2^-16
    of 2^256 (its top 16 bits ones) and d1 < 2^240; the low half likewise."""
    seed, t = SEEDS[2], C.tag(C.KIND_PERM_Z, 2)
    want = {"both>=r": lambda d0, d1: d0 >= R and d1 >= R, "both<r": lambda d0, d1: d0 < R and d1 < R,
            "d1 top ones": lambda d0, d1: d1 >> 240 == 0xFFFF, "d1 top zeros": lambda d0, d1: d1 >> 240 == 0,
            "d0 top ones": lambda d0, d1: d0 >> 240 == 0xFFFF, "d0 top zeros": lambda d0, d1: d0 >> 240 == 0}
    found = {}
    for row in range(1 << 20):
        d = C.digest(seed, 0, t, row)
        d0, d1 = int.from_bytes(d[:32], "little"), int.from_bytes(d[32:], "little")
        for name, pred in want.items():
            if name not in found and pred(d0, d1):
                found[name] = row
        if len(found) == len(want):
            break
    assert len(found) == len(want), found
    for row in found.values():
        v = check(ctx, seed, 0, t, row)
        d = int.from_bytes(C.digest(seed, 0, t, row), "little")
        assert v == d % R and v != d % (1 << 256) % R


def test_one_seed_gives_one_value_in_both_representations():
    a, b = host_ctx(False), host_ctx(True)
    for row in (0, 1, 1023):
        va, vb = eval_(a, SEEDS[1], 5, C.tag(C.KIND_LOOKUP_Z, 4), row), eval_(b, SEEDS[1], 5, C.tag(C.KIND_LOOKUP_Z, 4), row)
        assert va < R and vb < R and vb == va * (1 << 256) % R
    lib().h2r_ctx_destroy(a)
    lib().h2r_ctx_destroy(b)


# ---- h2r_random_columns: the refusals -----------------------------------------------------------------------------------------------------
def call(ctx, num_cols=2, row_begin=4, row_end=10, first_circuit=0, reserved=0, batch=3, struct_size=None, cols=None, null_cfg=False, null_cols=False):
    cfg = _lib.H2RRandomConfig(struct_size=ctypes.sizeof(_lib.H2RRandomConfig) if struct_size is None else struct_size, num_cols=num_cols,
                               row_begin=row_begin, row_end=row_end, first_circuit=first_circuit, reserved=reserved)
    cfg.seed[:] = SEEDS[2]
    cols = cols if cols is not None else [(BASE + c * 0x10000, 1024 * 32, C.TAGS[c % len(C.TAGS)], 0) for c in range(min(num_cols, 70))]
    desc = (_lib.H2RRandomColumn * max(len(cols), 1))()
    for d, (base, stride, tag, res) in zip(desc, cols):
        d.base, d.elem_stride, d.tag, d.reserved = base, stride, tag, res
    return lib().h2r_random_columns(ctx, None if null_cfg else ctypes.byref(cfg), None if null_cols else desc, batch, None)


def test_a_valid_call_ends_at_the_host_only_ctx(ctx):
    assert call(ctx) == UNSUP
    assert call(ctx, num_cols=64) == UNSUP and call(ctx, num_cols=1) == UNSUP
    assert call(ctx, cols=[(BASE, 0, 0, 0), (BASE + 0x1000, 6 * 32, 1, 0)]) == UNSUP              # a shared column; a stride of exactly the rows written
    assert call(ctx, first_circuit=2 ** 64 - 3) == UNSUP and call(ctx, num_cols=1, row_begin=2 ** 58 - 1, row_end=2 ** 58, cols=[(BASE, 32, 0, 0)]) == UNSUP


def test_an_empty_row_range_is_success_without_a_launch(ctx):
    assert call(ctx, row_begin=7, row_end=7) == 0 and call(ctx, row_begin=0, row_end=0) == 0


def test_every_refusal(ctx):
    assert lib().h2r_random_columns(None, None, None, 1, None) == NULL
    assert call(ctx, null_cfg=True) == NULL and call(ctx, null_cols=True) == NULL
    assert call(ctx, cols=[(BASE, 1024 * 32, 0, 0), (0, 1024 * 32, 1, 0)]) == NULL
    assert call(ctx, struct_size=ctypes.sizeof(_lib.H2RRandomConfig) - 8) == UNSUP
    for kw in (dict(num_cols=0), dict(num_cols=65), dict(row_begin=10, row_end=9), dict(reserved=1), dict(batch=0), dict(first_circuit=2 ** 64 - 2),
               dict(row_end=2 ** 58 + 1, cols=[(BASE, 0, 0, 0)] * 2),
               dict(cols=[(BASE + 8, 1024 * 32, 0, 0), (BASE + 0x10000, 1024 * 32, 1, 0)]),        # a base that is not 16-byte aligned
               dict(cols=[(BASE, 1024 * 32 + 8, 0, 0), (BASE + 0x10000, 1024 * 32, 1, 0)]),        # a stride likewise
               dict(cols=[(BASE, 1024 * 32, 0, 0), (BASE + 0x10000, 5 * 32, 1, 0)]),               # a stride below the six rows written
               dict(cols=[(BASE, 1024 * 32, 0, 0), (BASE + 0x10000, 1024 * 32, 1, 1)]),            # a column's reserved word
               dict(row_begin=7, row_end=7, reserved=1), dict(row_begin=7, row_end=7, num_cols=0)):  # an empty range is validated all the same
        assert call(ctx, **kw) == SHAPE, kw


@pytest.mark.parametrize("field", ["bn254_fq", "pasta_fp", "pasta_fq"])
def test_a_field_without_wide_reduce_constants_is_refused(field):
    c = host_ctx(False, field)
    out = (ctypes.c_uint64 * 4)()
    assert call(c) == SHAPE and call(c, row_begin=7, row_end=7) == SHAPE
    assert lib().h2r_random_eval(c, SEEDS[0], 0, 0, 0, out) == SHAPE
    assert lib().h2r_random_eval(None, SEEDS[0], 0, 0, 0, out) == NULL and lib().h2r_random_eval(c, None, 0, 0, 0, out) == NULL
    lib().h2r_ctx_destroy(c)
