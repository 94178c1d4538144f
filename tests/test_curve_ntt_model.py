"""The plain model of the transform over curve points (tests/curve_ntt_ref.py) against itself: the definition and the logarithm route agree,
the closed form for arithmetic-progression bases holds, forward undoes inverse, and the transformed key commits Lagrange-form columns to
what the monomial key commits their coefficients to.  No library, no device."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve_ntt_ref as C
import msm_ref as M
import ntt_ref as NR

R = M.R_ORDER


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_the_two_routes_agree(k):
    n = 1 << k
    rng = random.Random("curve_ntt/model/routes/%d" % k)
    logs = [rng.randrange(R) for _ in range(n)]
    logs[rng.randrange(n)] = 0                                   # the identity among the inputs
    points, omega = M.mul_g_batch(logs), C.omega_of(k)
    for inverse in (True, False):
        assert C.naive(points, omega, inverse) == C.by_logs(logs, omega, inverse), (k, inverse)


@pytest.mark.parametrize("k", [1, 3, 4])
def test_the_closed_form_of_structured_bases(k):
    n, a0, d = 1 << k, 0x1234567890abcdef, 0xfedcba987654321
    omega = C.omega_of(k)
    logs = [(a0 + j * d) % R for j in range(n)]
    assert M.structured_bases(n, a0, d) == M.mul_g_batch(logs)
    assert C.closed_form_logs(n, a0, d, omega, list(range(n))) == C.logs_transform(logs, omega, True)
    if k <= 3:
        assert C.naive(M.structured_bases(n, a0, d), omega, True) == M.mul_g_batch(C.closed_form_logs(n, a0, d, omega, list(range(n))))


def test_forward_after_inverse_is_the_identity():
    k = 3
    rng = random.Random("curve_ntt/model/roundtrip")
    points = M.mul_g_batch([rng.randrange(1, R) for _ in range(1 << k)])
    points[5] = M.IDENT
    omega = C.omega_of(k)
    assert C.naive(C.naive(points, omega, True), omega, False) == points
    logs = [rng.randrange(R) for _ in range(1 << 6)]
    assert C.logs_transform(C.logs_transform(logs, C.omega_of(6), True), C.omega_of(6), False) == logs


def test_the_commitment_identity_for_bases_that_are_no_powers_of_a_tau():
    """sum_i f(omega^i) L_i = sum_j f_j g_j with L the inverse transform of g: linear algebra, whatever the bases are."""
    k = 3
    n = 1 << k
    rng = random.Random("curve_ntt/model/commit")
    g = M.mul_g_batch([rng.randrange(1, R) for _ in range(n)])
    omega = C.omega_of(k)
    lagrange = C.naive(g, omega, True)
    coeffs = [rng.randrange(R) for _ in range(n)]
    evals = NR.forward(coeffs, k, omega, 1, R)
    assert [NR.horner(coeffs, pow(omega, i, R), R) for i in range(n)] == evals
    assert M.naive_msm(evals, lagrange) == M.naive_msm(coeffs, g)
