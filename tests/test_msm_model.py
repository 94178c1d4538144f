"""The plain model of the commitments (tests/msm_ref.py) against itself and against known values of bn256 G1; no library, no GPU."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_ref as M

TWO_G = (0x030644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd3, 0x15ed738c0e0a7c92e7845f96b2ae9c0a68a6a449e3538fc7ff3ebf7a5a18a2c4)


def test_two_g_is_the_known_point():
    assert M.on_curve(M.G) and M.on_curve(TWO_G)
    assert M.mul(2, M.G) == TWO_G == M.add(M.G, M.G) == M.mul_g(2)


def test_group_order():
    assert M.mul(M.R_ORDER, M.G) == M.IDENT
    assert M.mul(M.R_ORDER - 1, M.G) == M.neg(M.G)
    assert M.add(M.G, M.neg(M.G)) == M.IDENT and M.add(M.IDENT, M.G) == M.G == M.add(M.G, M.IDENT)
    assert M.mul(0, M.G) == M.IDENT and M.mul(5, M.IDENT) == M.IDENT


def test_fixed_base_table_equals_double_and_add():
    rng = random.Random("msm/model/table")
    for k in [0, 1, 255, 256, M.R_ORDER - 1, M.R_ORDER, M.R_ORDER + 1, (1 << 256) - 1] + [rng.getrandbits(256) for _ in range(8)]:
        assert M.mul_g(k) == M.mul(k % M.R_ORDER, M.G), k
        assert M.on_curve(M.mul_g(k))


def test_structured_closed_form_equals_naive_msm():
    rng = random.Random("msm/model/structured")
    n, a0, d = 64, rng.randrange(M.R_ORDER), rng.randrange(M.R_ORDER)
    bases = M.structured_bases(n, a0, d)
    assert all(M.on_curve(p) for p in bases)
    assert bases[0] == M.mul_g(a0) and bases[5] == M.mul_g(a0 + 5 * d)
    scalars = [rng.randrange(M.R_ORDER) for _ in range(n)]
    assert M.structured_sum(scalars, a0, d) == M.naive_msm(scalars, bases)
    tiled = [bases[i % 16] for i in range(n)]
    assert M.structured_sum(scalars, a0, d, period=16) == M.naive_msm(scalars, tiled)


def test_byte_forms_round_trip():
    pts = [M.G, TWO_G, M.IDENT]
    for mont in (False, True):
        assert M.points_from_bytes(M.point_bytes(pts, mont), mont) == pts
    assert M.scalar_bytes([1], True) == (M.R256 % M.R_ORDER).to_bytes(32, "little")
