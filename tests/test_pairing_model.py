"""CPU: the plain model of the pairing check (tests/pairing_ref.py) against itself and against arithmetic facts: the
integer identities behind the final exponentiation, the 102 steps of a table, e(G1, G2) of order r, bilinearity, the device's
decomposition against the plain power, a second route for the Miller value with no table, and the KZG check with only [tau]G2 known."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_ref as M
import pairing_ref as P

Q, R, U = P.Q, P.R, P.U


@pytest.fixture(scope="module")
def g():
    """(the table of G2, e(G1, G2))"""
    tab = P.prepare(P.G2)
    return tab, P.final_exp(P.miller([(M.G, tab)]))


def test_integer_identities():
    assert Q == 36 * U ** 4 + 36 * U ** 3 + 24 * U ** 2 + 6 * U + 1 and R == 36 * U ** 4 + 36 * U ** 3 + 18 * U ** 2 + 6 * U + 1
    assert P.LOOP == 29793968203157093288 and P.LOOP.bit_length() == 65 and bin(P.LOOP).count("1") - 1 == 36
    assert U.bit_length() == 63 and bin(U).count("1") == 28
    hard = (Q ** 4 - Q ** 2 + 1) // R
    assert (Q ** 4 - Q ** 2 + 1) % R == 0 and (Q ** 6 - 1) * (Q ** 2 + 1) * hard == P.EXP and (Q ** 12 - 1) % R == 0
    assert hard == Q ** 3 + (6 * U ** 2 + 1) * Q ** 2 + (-36 * U ** 3 - 18 * U ** 2 - 12 * U + 1) * Q + (-36 * U ** 3 - 30 * U ** 2 - 18 * U - 2)
    assert Q % 4 == 3 and Q % 6 == 1                       # i^2 = -1 is a non-residue; (q - 1) / 6 is an integer
    assert P.f2mul(P.B2, P.XI) == (3, 0)


def test_the_generator_and_the_table(g):
    tab, _ = g
    assert P.g2_on_curve(P.G2) and P.g2_mul(R, P.G2) is None and P.g2_mul(R - 1, P.G2) == P.g2_neg(P.G2)
    assert len(tab) == P.STEPS == 102 == 64 + 36 + 2
    other = P.g2_mul(0xDEADBEEF, P.G2)
    assert P.g2_on_curve(other) and len(P.prepare(other)) == 102
    assert P.g2_frob(P.g2_frob(P.g2_frob(P.G2))) != P.G2 and P.g2_on_curve(P.g2_frob(P.G2))
    # pi(Q) = [q]Q on G2: the trace-zero subgroup
    assert P.g2_frob(P.G2) == P.g2_mul(Q % R, P.G2)


def test_fq12_arithmetic():
    rng = random.Random(3)
    for _ in range(3):
        a, b, c = ([(rng.randrange(Q), rng.randrange(Q)) for _ in range(6)] for _ in range(3))
        assert P.mul12(a, b) == P.mul12(b, a) and P.mul12(P.mul12(a, b), c) == P.mul12(a, P.mul12(b, c))
        assert P.mul12(a, P.inv12(a)) == P.ONE
        assert P.frob12(a, 1) == P.pow12(a, Q) and P.frob12(a, 2) == P.frob12(P.frob12(a, 1), 1) and P.frob12(a, 3) == P.frob12(P.frob12(a, 2), 1)
        assert P.frob12(a, 6) == P.conj12(a) and P.frob12(a, 12) == a
        assert P.frob12(P.mul12(a, b), 1) == P.mul12(P.frob12(a, 1), P.frob12(b, 1))
    w = [P.Z2, (1, 0)] + [P.Z2] * 4
    assert P.pow12(w, 6) == [P.XI] + [P.Z2] * 5
    sparse = [(5, 0), P.Z2, P.Z2, (0, 7), P.Z2, P.Z2]
    assert P.mul12(sparse, P.inv12(sparse)) == P.ONE


def test_final_exp_chain_is_the_plain_power(g):
    tab, _ = g
    rng = random.Random(4)
    inputs = [[(rng.randrange(Q), rng.randrange(Q)) for _ in range(6)] for _ in range(2)]
    inputs += [P.ONE, [(2, 0), P.Z2, P.Z2, (0, 1), P.Z2, P.Z2], [P.Z2, (1, 0)] + [P.Z2] * 4, P.line(tab[0], M.G), P.miller([(M.mul_g(77), tab)])]
    for f in inputs:
        assert P.final_exp_chain(f) == P.final_exp(f)


def test_order_and_bilinearity(g):
    tab, e = g
    assert e != P.ONE and P.pow12(e, R) == P.ONE
    assert P.mul12(e, P.conj12(e)) == P.ONE                  # unitary
    rng = random.Random(1)
    a, b = rng.randrange(R), rng.randrange(R)
    assert P.pairing(M.mul_g(a), P.g2_mul(b, P.G2)) == P.pow12(e, a * b % R)
    assert P.pairing(M.neg(M.G), P.G2) == P.conj12(e) and P.pairing(M.G, P.g2_neg(P.G2)) == P.conj12(e)
    assert P.miller([(M.IDENT, tab)]) == P.ONE and P.miller([]) == P.ONE


def test_a_second_route_for_the_miller_value(g):
    tab, _ = g
    rng = random.Random(6)
    other = P.g2_mul(rng.randrange(R), P.G2)
    for p, q2, t in ((M.G, P.G2, tab), (M.mul_g(rng.randrange(R)), P.G2, tab), (M.neg(M.G), other, P.prepare(other))):
        assert P.miller_untwisted(p, q2) == P.miller([(p, t)])


def test_the_kzg_check_knows_only_tau_g2(g):
    tab, _ = g
    rng = random.Random(8)
    tau, a = rng.randrange(R), rng.randrange(1, R)
    tab_tau = P.prepare(P.g2_mul(tau, P.G2))
    L = M.mul_g(a)
    Rp = M.mul(tau, L)
    assert P.check([(L, tab_tau), (M.neg(Rp), tab)])[0]
    assert not P.check([(L, tab_tau), (M.neg(M.add(Rp, M.G)), tab)])[0]
    assert not P.check([(L, tab_tau), (Rp, tab)])[0]                              # the mask matters
    # an identity L or R: accepted only together
    assert P.check([(M.IDENT, tab_tau), (M.IDENT, tab)]) == (True, P.ONE)
    assert not P.check([(M.IDENT, tab_tau), (M.neg(Rp), tab)])[0] and not P.check([(L, tab_tau), (M.IDENT, tab)])[0]
    # one squaring for all pairs: the product's Miller value times the single ones' agree after the final exponentiation only
    both = P.final_exp(P.miller([(L, tab_tau), (M.G, tab)]))
    assert both == P.mul12(P.final_exp(P.miller([(L, tab_tau)])), P.final_exp(P.miller([(M.G, tab)])))
