"""CPU-side checks of the KZG setup exports on a host-only ctx, both representations: the host twin
h2r_fixed_base_eval -- the very functions the kernels inline -- byte for byte against tests/msm_ref.py, h2r_g2_mul against
tests/pairing_ref.py, the generator constant, and every refusal of the device exports next to a valid twin that ends in
H2R_E_UNSUPPORTED: the host-only ctx is refused last."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_ref as M
import pairing_ref as P
import permutation_ref as PR
import setup_ref as S
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
from test_transcript_host import host_ctx

Q, R = M.Q, M.R_ORDER
NULL, SHAPE, UNSUP, ASSERTION = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED, _lib.H2R_E_ASSERTION
BASE = 0x100000                                  # never dereferenced: the checks are host arithmetic on the addresses
REPRS, IDS = [False, True], ["canonical", "montgomery"]
A = 0x1F2E3D4C5B6A79881726354453627180


@pytest.fixture(scope="module", params=REPRS, ids=IDS)
def ctx(request):
    c = host_ctx(request.param)
    yield c, request.param
    lib().h2r_ctx_destroy(c)


def u64s(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def pt_words(p):
    return u64s(M.words(p[0]) + M.words(p[1]))


def fb_eval(c, op, base, arg):
    out = u64s([0xEE] * 8)
    rc = lib().h2r_fixed_base_eval(c, op, pt_words(base), u64s(arg), out)
    return rc, (sum(out[k] << (64 * k) for k in range(4)), sum(out[4 + k] << (64 * k) for k in range(4)))


BASES = [("G", M.G), ("[a]G", M.mul_g(A)), ("identity", M.IDENT)]


@pytest.mark.parametrize("name,base", BASES, ids=[n for n, _ in BASES])
def test_table_entries_and_the_digit_walk(ctx, name, base):
    c, _ = ctx
    for w in (0, 1, 8, 31):
        for d in (0, 1, 2, 127, 128, 255):
            rc, got = fb_eval(c, 0, base, [w, d])
            assert rc == 0 and got == M.mul(d << (8 * w), base), (w, d)
    if base == M.G:
        T = M.g_table()
        for w, d in ((0, 1), (3, 200), (31, 255), (17, 0)):
            assert fb_eval(c, 0, base, [w, d]) == (0, T[w][d])
    for k in S.edge_scalars(random.Random(3)):
        rc, got = fb_eval(c, 1, base, M.words(k))
        want = M.mul_g(k) if base == M.G else M.mul(k % R, base)       # a canonical scalar >= r multiplies like its residue
        assert rc == 0 and got == want, hex(k)
    assert fb_eval(c, 1, base, M.words(R)) == (0, M.IDENT)


def test_fixed_base_eval_refusals(ctx):
    c, mont = ctx
    f = lib().h2r_fixed_base_eval
    g, out, k = pt_words(M.G), u64s([0] * 8), u64s(M.words(5))
    assert f(c, 1, g, k, out) == 0                                         # the valid twin
    assert f(None, 1, g, k, out) == NULL and f(c, 1, None, k, out) == NULL and f(c, 1, g, None, out) == NULL and f(c, 1, g, k, None) == NULL
    assert f(c, 2, g, k, out) == SHAPE
    assert f(c, 0, g, u64s([31, 255]), out) == 0 and f(c, 0, g, u64s([32, 0]), out) == SHAPE and f(c, 0, g, u64s([0, 256]), out) == SHAPE
    assert f(c, 1, pt_words((Q, 2)), k, out) == SHAPE and f(c, 1, pt_words((1, Q)), k, out) == SHAPE
    assert f(c, 1, pt_words((1, 3)), k, out) == ASSERTION and f(c, 1, pt_words((0, 1)), k, out) == ASSERTION
    assert f(c, 1, pt_words((Q, 3)), k, out) == SHAPE                      # both faults: the range first
    other = host_ctx(mont, field="pasta_fp")
    assert f(other, 1, g, k, out) == UNSUP
    lib().h2r_ctx_destroy(other)


# ---- G2 -------------------------------------------------------------------------------------------------------------------------------------
def g2_call(c, raw, k):
    out = (ctypes.c_uint8 * 128)(*([0xEE] * 128))
    rc = lib().h2r_g2_mul(c, raw, u64s(M.words(k)), out)
    return rc, bytes(out)


def g2_model_bytes(p, mont):
    return bytes(128) if p is None else P.g2_bytes(p, mont)


def test_the_g2_generator_is_the_models(ctx):
    c, mont = ctx
    out = (ctypes.c_uint8 * 128)()
    assert lib().h2r_g2_generator(c, out) == 0 and bytes(out) == P.g2_bytes(P.G2, mont)
    assert lib().h2r_g2_generator(None, out) == NULL and lib().h2r_g2_generator(c, None) == NULL


def test_g2_mul_matches_the_model(ctx):
    c, mont = ctx
    g2 = P.g2_bytes(P.G2, mont)
    other = P.g2_mul(A, P.G2)
    for k in S.edge_scalars(random.Random(4)):
        assert g2_call(c, g2, k) == (0, g2_model_bytes(P.g2_mul(k, P.G2), mont)), hex(k)
    for k in (0, 1, 2, R - 1, R, R + 1, (1 << 256) - 1):
        assert g2_call(c, P.g2_bytes(other, mont), k) == (0, g2_model_bytes(P.g2_mul(k, other), mont)), hex(k)
        assert g2_call(c, bytes(128), k) == (0, bytes(128))              # the identity is a legal input
    assert g2_call(c, g2, R) == (0, bytes(128)) and g2_call(c, g2, 0) == (0, bytes(128))
    assert g2_call(c, g2, R - 1) == (0, P.g2_bytes(P.g2_neg(P.G2), mont))


def test_g2_mul_refusals(ctx):
    c, mont = ctx
    f = lib().h2r_g2_mul
    g2, k, out = P.g2_bytes(P.G2, mont), u64s(M.words(3)), (ctypes.c_uint8 * 128)(*([0xEE] * 128))
    assert f(c, g2, k, out) == 0                                           # the valid twin
    out = (ctypes.c_uint8 * 128)(*([0xEE] * 128))
    assert f(None, g2, k, out) == NULL and f(c, None, k, out) == NULL and f(c, g2, None, out) == NULL and f(c, g2, k, None) == NULL
    for j in range(4):
        bad = bytearray(g2)
        bad[32 * j:32 * j + 32] = Q.to_bytes(32, "little")
        assert f(c, bytes(bad), k, out) == SHAPE
    x, y = P.G2
    assert f(c, P.g2_bytes((x, P.f2add(y, (1, 0))), mont), k, out) == ASSERTION     # off E'
    assert f(c, P.g2_bytes(((1, 0), (2, 0)), mont), k, out) == ASSERTION            # G1's generator is not on the twist
    assert bytes(out) == b"\xee" * 128                                     # a refusal writes nothing
    other = host_ctx(mont, field="pasta_fp")
    assert f(other, g2, k, out) == UNSUP and lib().h2r_g2_generator(other, out) == UNSUP
    lib().h2r_ctx_destroy(other)


# ---- the device exports' refusals ---------------------------------------------------------------------------------------------------------
def test_fixed_base_table_refusals(ctx):
    c, mont = ctx
    f = lib().h2r_fixed_base_table
    g = M.point_bytes([M.G], mont)
    assert f(c, g, BASE, None) == UNSUP                                    # the valid twin: only the device is missing
    assert f(c, M.point_bytes([M.IDENT], mont), BASE, None) == UNSUP and f(c, M.point_bytes([M.mul_g(A)], mont), BASE, None) == UNSUP
    assert f(None, g, BASE, None) == NULL and f(c, None, BASE, None) == NULL and f(c, g, None, None) == NULL
    assert f(c, g, BASE + 8, None) == SHAPE
    assert f(c, Q.to_bytes(32, "little") + g[32:], BASE, None) == SHAPE and f(c, g[:32] + Q.to_bytes(32, "little"), BASE, None) == SHAPE
    assert f(c, M.point_bytes([(1, 3)], mont), BASE, None) == ASSERTION and f(c, M.point_bytes([(0, 1)], mont), BASE, None) == ASSERTION
    assert f(c, M.point_bytes([(1, 3)], mont), BASE + 8, None) == SHAPE    # the pointer before the point
    other = host_ctx(mont, field="pasta_fp")
    assert f(other, g, BASE, None) == UNSUP and f(other, M.point_bytes([(1, 3)], mont), BASE, None) == UNSUP
    lib().h2r_ctx_destroy(other)


def test_fixed_base_mul_refusals(ctx):
    c, mont = ctx
    T = _lib.H2R_FIXED_BASE_TABLE_BYTES

    def call(ctx_=c, table=BASE, scalars=BASE + 0x100000, n=1000, out=BASE + 0x200000):
        return lib().h2r_fixed_base_mul(ctx_, table, scalars, n, out, None)

    assert call() == UNSUP and call(n=1) == UNSUP and call(n=1 << 24, out=BASE + 0x40000000) == UNSUP       # valid twins
    assert call(ctx_=None) == NULL and call(table=None) == NULL and call(scalars=None) == NULL and call(out=None) == NULL
    assert call(n=0) == SHAPE and call(n=(1 << 24) + 1, out=BASE + 0x40000000) == SHAPE
    assert call(n=0, table=BASE + 8) == SHAPE
    assert call(table=BASE + 8) == SHAPE and call(scalars=BASE + 0x100008) == SHAPE and call(out=BASE + 0x200008) == SHAPE
    assert call(out=BASE + 0x100000 + 32 * 1000 - 16) == SHAPE and call(out=BASE + 0x100000 + 32 * 1000) == UNSUP      # over the scalars' last bytes
    assert call(out=BASE + 0x100000 - 64 * 1000 + 16) == SHAPE and call(out=BASE + 0x100000) == SHAPE                  # from below; in place
    assert call(out=BASE + T - 16) == SHAPE and call(out=BASE + T) == UNSUP                                            # over the table's last bytes
    assert call(table=BASE + 0x200000 + 64 * 1000 - 16) == SHAPE and call(table=BASE + 0x200000 + 64 * 1000) == UNSUP
    other = host_ctx(mont, field="pasta_fp")
    assert call(ctx_=other) == UNSUP and call(ctx_=other, n=0) == SHAPE
    lib().h2r_ctx_destroy(other)


def rep(v, mont):
    return v * M.R256 % R if mont else v


def test_setup_scalars_refusals(ctx):
    c, mont = ctx
    w4 = PR.domain(R, 4)[0]

    def call(ctx_=c, cfg=True, size=None, mode=_lib.H2R_SETUP_LAGRANGE, log_n=4, n=0, reserved=0, tau=rep(5, mont), omega=rep(w4, mont), out=BASE):
        sc = _lib.H2RSetupConfig(ctypes.sizeof(_lib.H2RSetupConfig) if size is None else size, mode, log_n, reserved, n)
        sc.tau[:], sc.omega[:] = M.words(tau), M.words(omega)
        return lib().h2r_kzg_setup_scalars(ctx_, ctypes.byref(sc) if cfg else None, out, None)

    P0 = dict(mode=_lib.H2R_SETUP_POWERS, log_n=0)
    assert call() == UNSUP                                                 # the valid twins: only the device is missing
    assert call(n=1, **P0) == UNSUP and call(n=1 << 24, **P0) == UNSUP and call(n=1000, omega=0, **P0) == UNSUP
    assert call(n=7, tau=0, **P0) == UNSUP and call(n=7, tau=rep(1, mont), **P0) == UNSUP and call(tau=0) == UNSUP
    assert call(log_n=1, omega=rep(R - 1, mont)) == UNSUP and call(log_n=24, omega=rep(PR.domain(R, 24)[0], mont)) == UNSUP
    assert call(ctx_=None) == NULL and call(cfg=False) == NULL and call(out=None) == NULL
    assert call(size=80) == UNSUP and call(mode=2) == UNSUP and call(size=80, log_n=0) == UNSUP       # struct_size and mode before the shape
    assert call(mode=2, out=BASE + 8) == UNSUP
    assert call(reserved=1) == SHAPE and call(log_n=0) == SHAPE and call(log_n=25) == SHAPE and call(n=16) == SHAPE
    assert call(n=0, **P0) == SHAPE and call(n=(1 << 24) + 1, **P0) == SHAPE and call(n=16, mode=_lib.H2R_SETUP_POWERS, log_n=4) == SHAPE
    assert call(tau=R) == SHAPE and call(omega=R) == SHAPE and call(n=16, tau=R, **P0) == SHAPE and call(n=16, omega=R, **P0) == SHAPE
    assert call(omega=rep(5, mont)) == SHAPE and call(omega=rep(PR.domain(R, 3)[0], mont)) == SHAPE and call(omega=rep(PR.domain(R, 5)[0], mont)) == SHAPE
    # tau inside the domain: upstream's formula divides by zero there
    assert call(tau=rep(pow(w4, 3, R), mont)) == SHAPE and call(tau=rep(1, mont)) == SHAPE and call(tau=rep(R - 1, mont)) == SHAPE
    assert call(tau=rep(PR.domain(R, 5)[0], mont)) == UNSUP                # a root of unity outside this domain is legal
    assert call(out=BASE + 8) == SHAPE and call(n=16, out=BASE + 8, **P0) == SHAPE
    other = host_ctx(mont, field="pasta_fp")                               # the scalars need no curve: any field's own roots
    assert call(ctx_=other, n=16, tau=5, omega=0, **P0) == UNSUP and call(ctx_=other, n=0, tau=5, omega=0, **P0) == SHAPE
    lib().h2r_ctx_destroy(other)


def test_the_package_constants():
    assert _lib.FIELD_ROOT_OF_UNITY["bn254_fr"] == (28, PR.domain(R, 28)[0])
    assert _lib.CURVE_GENERATOR["bn254_fr"] == (Q, M.G) and M.on_curve(M.G)
    assert _lib.H2R_FIXED_BASE_TABLE_BYTES == 32 * 256 * 64
