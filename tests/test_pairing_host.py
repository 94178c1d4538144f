"""CPU-side checks of the pairing exports on a host-only ctx, both representations: the host twin h2r_pairing_eval --
the very functions the kernel inlines -- and h2r_pairing_prepare byte for byte against the plain model (tests/pairing_ref.py), and every
refusal of the three exports; h2r_pairing_products refuses a host-only ctx last."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_ref as M
import pairing_ref as P
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
from test_transcript_host import host_ctx

Q = P.Q
NULL, SHAPE, UNSUP, ASSERTION = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED, _lib.H2R_E_ASSERTION
BASE = 0x100000                                  # never dereferenced: the checks are host arithmetic on the addresses
REPRS, IDS = [False, True], ["canonical", "montgomery"]
Z2 = P.Z2


@pytest.fixture(scope="module", params=REPRS, ids=IDS)
def ctx(request):
    c = host_ctx(request.param)
    yield c, request.param
    lib().h2r_ctx_destroy(c)


@pytest.fixture(scope="module")
def keys():
    """tables of G2 and of three multiples, made once by the model"""
    rng = random.Random(2)
    pts = [P.G2] + [P.g2_mul(rng.randrange(1, P.R), P.G2) for _ in range(3)]
    return pts, [P.prepare(p) for p in pts]


def ev(c, op, raw, out_len=384):
    out = (ctypes.c_uint8 * out_len)(*([0xEE] * out_len))
    rc = lib().h2r_pairing_eval(c, op, raw, len(raw), out, out_len)
    return rc, bytes(out)


def operands(rng):
    """zero, one, q - 1 everywhere, single-coefficient and sparse elements, random ones"""
    single = [[((Q - 1, 5) if j == k else Z2) for j in range(6)] for k in range(6)]
    sparse = [[(3, 0), (rng.randrange(Q), rng.randrange(Q)), Z2, (rng.randrange(Q), rng.randrange(Q)), Z2, Z2],
              [(rng.randrange(Q), 0), Z2, Z2, (0, rng.randrange(Q)), Z2, Z2]]
    rnd = [[(rng.randrange(Q), rng.randrange(Q)) for _ in range(6)] for _ in range(4)]
    return [[Z2] * 6, P.ONE, [(Q - 1, Q - 1)] * 6] + single + sparse + rnd


def test_fq12_product_inverse_frobenius(ctx):
    c, mont = ctx
    vals = operands(random.Random(11))
    for i, a in enumerate(vals):
        for b in (vals[(5 * i + 3) % len(vals)], vals[(i + 1) % len(vals)], a):
            rc, out = ev(c, 0, P.fq12_bytes(a, mont) + P.fq12_bytes(b, mont))
            assert rc == 0 and out == P.fq12_bytes(P.mul12(a, b), mont), (i, a, b)
        rc, out = ev(c, 1, P.fq12_bytes(a, mont))
        if all(x == Z2 for x in a):
            assert rc == SHAPE and out == b"\xee" * 384
        else:
            inv = P.fq12_from_bytes(out, mont)
            assert rc == 0 and out == P.fq12_bytes(P.inv12(a), mont) and P.mul12(a, inv) == P.ONE
        for k in (0, 1, 2, 3, 6, 11):
            rc, out = ev(c, 2, bytes([k]) + P.fq12_bytes(a, mont))
            assert rc == 0 and out == P.fq12_bytes(P.frob12(a, k), mont), (i, k)
    a = vals[-1]
    rc, out = ev(c, 2, bytes([1]) + P.fq12_bytes(a, mont))
    assert P.fq12_from_bytes(out, mont) == P.pow12(a, Q)                 # the Frobenius map is the power by q


def miller_input(J, mask, pts, tabs, mont):
    return bytes([J, mask]) + b"".join(M.point_bytes([pts[j]], mont) + P.table_bytes(tabs[j], mont) for j in range(J))


def test_prepare_matches_the_model(ctx, keys):
    c, mont = ctx
    pts, tabs = keys
    for p, tab in zip(pts[:2], tabs[:2]):
        out = (ctypes.c_uint8 * P.TABLE_BYTES)()
        assert lib().h2r_pairing_prepare(c, P.g2_bytes(p, mont), out) == 0
        assert bytes(out) == P.table_bytes(tab, mont) and len(tab) == _lib.H2R_PAIRING_STEPS


@pytest.mark.parametrize("J", [1, 2, 4])
def test_miller_value_every_mask(ctx, keys, J):
    c, mont = ctx
    _, tabs = keys
    rng = random.Random(J)
    sets = [[M.mul_g(rng.randrange(1, P.R)) for _ in range(J)],
            [M.G if j % 2 == 0 else M.neg(M.G) for j in range(J)],              # P = (1, 2) and its negative
            [M.IDENT if j == 0 else M.mul_g(7 + j) for j in range(J)],          # (0, 0) operands
            [M.IDENT] * J]
    for pts in sets:
        for mask in range(1 << J):
            eff = [M.neg(p) if (mask >> j) & 1 else p for j, p in enumerate(pts)]
            want = P.miller(list(zip(eff, tabs)))
            rc, out = ev(c, 3, miller_input(J, mask, pts, tabs, mont))
            assert rc == 0 and out == P.fq12_bytes(want, mont), (J, mask, pts)
    assert P.miller([(M.IDENT, tabs[0])] * J) == P.ONE


def test_final_exponentiation_and_the_whole_check(ctx, keys):
    c, mont = ctx
    g2s, tabs = keys
    rng = random.Random(5)
    for f in (P.ONE, [(rng.randrange(Q), rng.randrange(Q)) for _ in range(6)], [(2, 0), Z2, Z2, (0, 1), Z2, Z2], P.miller([(M.G, tabs[0])])):
        rc, out = ev(c, 4, P.fq12_bytes(f, mont))
        assert rc == 0 and out == P.fq12_bytes(P.final_exp(f), mont)
    # e(a G, Q) e(-a' G, G2) with Q = k G2: one exactly when a k = a'
    k = 0x1234567
    tab_k = P.prepare(P.g2_mul(k, P.G2))
    for a, a2, mask in ((5, 5 * k, 2), (5, 5 * k + 1, 2), (9, P.R - 9 * k, 0)):
        pts = [M.mul_g(a), M.mul_g(a2 % P.R)]
        ts = [tab_k, tabs[0]]
        eff = [M.neg(p) if (mask >> j) & 1 else p for j, p in enumerate(pts)]
        accept, gt = P.check(list(zip(eff, ts)))
        rc, out = ev(c, 5, miller_input(2, mask, pts, ts, mont), 385)
        assert rc == 0 and out[0] == int(accept) and out[1:] == P.fq12_bytes(gt, mont)
        assert accept == ((a * k - (a2 if mask else -a2)) % P.R == 0)
    rc, out = ev(c, 5, miller_input(1, 0, [M.IDENT], tabs[:1], mont), 385)
    assert rc == 0 and out[0] == 1 and out[1:] == P.fq12_bytes(P.ONE, mont)


def test_operand_status(ctx, keys):
    c, mont = ctx
    _, tabs = keys
    good = M.point_bytes([M.mul_g(3)], mont)
    off = M.point_bytes([(1, 3)], mont)
    big = Q.to_bytes(32, "little") + good[32:]
    tb = [P.table_bytes(t, mont) for t in tabs[:2]]
    for op, n in ((3, 384), (5, 385)):
        assert ev(c, op, bytes([2, 0]) + good + tb[0] + off + tb[1], n) == (ASSERTION, b"\xee" * n)
        assert ev(c, op, bytes([2, 0]) + big + tb[0] + good + tb[1], n) == (SHAPE, b"\xee" * n)
        assert ev(c, op, bytes([2, 0]) + off + tb[0] + big + tb[1], n) == (SHAPE, b"\xee" * n)       # both faults: H2R_E_SHAPE wins
        assert ev(c, op, bytes([2, 0]) + good + tb[0] + good[:32] + Q.to_bytes(32, "little") + tb[1], n)[0] == SHAPE


def test_eval_refusals(ctx, keys):
    c, mont = ctx
    _, tabs = keys
    one = P.fq12_bytes(P.ONE, mont)
    out = (ctypes.c_uint8 * 385)()
    L = lib().h2r_pairing_eval
    assert L(None, 0, one + one, 768, out, 384) == NULL
    assert L(c, 0, None, 768, out, 384) == NULL
    assert L(c, 0, one + one, 768, None, 384) == NULL
    assert L(c, 6, one, 384, out, 384) == SHAPE
    for op, n in ((0, 768), (1, 384), (2, 385), (4, 384)):
        raw = (bytes([1]) if op == 2 else b"") + one * (2 if op == 0 else 1)
        assert L(c, op, raw, n, out, 384) == 0
        assert L(c, op, raw, n - 32, out, 384) == SHAPE and L(c, op, raw, n, out, 383) == SHAPE
        bad = bytearray(raw)
        bad[n - 32:n] = Q.to_bytes(32, "little")
        assert L(c, op, bytes(bad), n, out, 384) == SHAPE                    # a coordinate >= q
    assert L(c, 2, bytes([12]) + one, 385, out, 384) == SHAPE
    good = miller_input(1, 0, [M.G], tabs[:1], mont)
    assert L(c, 3, good, len(good), out, 384) == 0
    assert L(c, 3, good, len(good), out, 385) == SHAPE and L(c, 5, good, len(good), out, 384) == SHAPE
    assert L(c, 3, good, len(good) - 1, out, 384) == SHAPE and L(c, 3, good, 1, out, 384) == SHAPE
    for head in ((0, 0), (5, 0), (1, 2)):                                     # J = 0, J > 4, a mask bit at or above J
        assert L(c, 3, bytes(head) + good[2:], len(good), out, 384) == SHAPE
    bad = bytearray(good)
    bad[-32:] = Q.to_bytes(32, "little")
    assert L(c, 3, bytes(bad), len(bad), out, 384) == SHAPE                   # a table entry >= q
    other = host_ctx(mont, field="pasta_fp")
    assert L(other, 0, one + one, 768, out, 384) == UNSUP
    tab = (ctypes.c_uint8 * P.TABLE_BYTES)()
    assert lib().h2r_pairing_prepare(other, P.g2_bytes(P.G2, mont), tab) == UNSUP
    lib().h2r_ctx_destroy(other)


def test_prepare_refusals(ctx):
    c, mont = ctx
    prep = lib().h2r_pairing_prepare
    tab = (ctypes.c_uint8 * P.TABLE_BYTES)(*([0xEE] * P.TABLE_BYTES))
    g2 = P.g2_bytes(P.G2, mont)
    assert prep(None, g2, tab) == NULL and prep(c, None, tab) == NULL and prep(c, g2, None) == NULL
    for k in range(4):
        bad = bytearray(g2)
        bad[32 * k:32 * k + 32] = Q.to_bytes(32, "little")
        assert prep(c, bytes(bad), tab) == SHAPE
    assert prep(c, bytes(128), tab) == ASSERTION                              # the identity
    x, y = P.G2
    assert prep(c, P.g2_bytes((x, P.f2add(y, (1, 0))), mont), tab) == ASSERTION   # off E'
    assert prep(c, P.g2_bytes(((1, 0), (2, 0)), mont), tab) == ASSERTION          # G1's generator is not on the twist
    assert bytes(tab) == b"\xee" * P.TABLE_BYTES                               # a refusal writes nothing


def test_products_refusals(ctx):
    """every refusal next to a valid twin that ends in H2R_E_UNSUPPORTED: the host-only ctx is refused last"""
    c, mont = ctx
    T = P.TABLE_BYTES

    def call(ctx_=c, cfg=True, size=None, J=2, mask=2, reserved=0, tables=BASE, points=BASE + 0x100000, stride=128, batch=16, gt=BASE + 0x200000,
             accept=BASE + 0x300000, status=BASE + 0x400000):
        pc = _lib.H2RPairingConfig(ctypes.sizeof(_lib.H2RPairingConfig) if size is None else size, J, mask, reserved)
        return lib().h2r_pairing_products(ctx_, ctypes.byref(pc) if cfg else None, tables, points, stride, batch, gt, accept, status, None)

    assert call() == UNSUP                                                   # the valid twin: only the device is missing
    assert call(gt=None) == UNSUP and call(accept=None) == UNSUP and call(status=None) == UNSUP and call(batch=0) == UNSUP
    assert call(stride=0) == UNSUP and call(J=4, mask=15, stride=256) == UNSUP and call(J=1, mask=1, stride=64) == UNSUP
    assert call(ctx_=None) == NULL and call(cfg=False) == NULL and call(tables=None) == NULL and call(points=None) == NULL
    assert call(size=12) == UNSUP and call(size=12, J=0) == UNSUP            # struct_size before the shape
    assert call(J=0, mask=0) == SHAPE and call(J=5, mask=0, stride=320) == SHAPE
    assert call(mask=4) == SHAPE and call(J=1, mask=2) == SHAPE and call(reserved=1) == SHAPE
    assert call(tables=BASE + 8) == SHAPE and call(points=BASE + 0x100008) == SHAPE and call(stride=136) == SHAPE and call(gt=BASE + 0x200008) == SHAPE
    assert call(stride=64) == SHAPE and call(J=4, mask=0, stride=128) == SHAPE            # a stride below 64 num_pairs
    assert call(gt=BASE + 2 * T - 16) == SHAPE                                # gt over the tables' last bytes
    assert call(gt=BASE + 2 * T) == UNSUP
    assert call(gt=BASE + 0x100000 + 15 * 128 + 112) == SHAPE                 # gt over the last point
    assert call(accept=BASE + 0x200000 + 16 * 384 - 1) == SHAPE               # accept inside gt
    assert call(status=BASE + 0x300000 + 15) == SHAPE                         # status inside accept
    assert call(status=BASE + 0x100000) == SHAPE and call(accept=BASE + 5) == SHAPE
    other = host_ctx(mont, field="pasta_fp")
    assert call(ctx_=other) == UNSUP
    lib().h2r_ctx_destroy(other)
