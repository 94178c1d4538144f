"""The plain model of the evaluation domain's transforms (tests/ntt_ref.py) against its own definition, on the three fields that have 2^k
domains: the recursive transform equals the O(n^2) sum, inverse undoes forward, a forward output is the polynomial's value at g * omega^j
(Horner), and the closed form that tests/test_ntt_gpu.py uses where 2^20 terms are too many equals the model where they are not.  No device."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import ntt_ref as NR
from pyref import FIELD_MODULI

FIELDS = NR.FIELDS_WITH_DOMAINS


def shifts(P, rng):
    return [1, NR.cube_root_of_unity(P), rng.randrange(2, P)]


@pytest.mark.parametrize("field", FIELDS)
def test_domain_roots(field):
    P = FIELD_MODULI[field]
    for k in (1, 2, 8, 21):
        w = NR.omega_of(P, k)
        assert pow(w, 1 << (k - 1), P) == P - 1                      # primitive: omega^(n / 2) = -1
    assert NR.omega_of(P, 8) == pow(NR.omega_of(P, 10), 4, P)         # the smaller domain's generator is a power of the larger one's
    z = NR.cube_root_of_unity(P)
    assert z != 1 and pow(z, 3, P) == 1
    with pytest.raises(ValueError):
        NR.omega_of(FIELD_MODULI["bn254_fq"], 2)                      # p - 1 = 2 * odd: no domain beyond two points
    assert NR.omega_of(FIELD_MODULI["bn254_fq"], 1) == FIELD_MODULI["bn254_fq"] - 1


@pytest.mark.parametrize("field", FIELDS)
def test_recursive_equals_naive(field):
    P = FIELD_MODULI[field]
    rng = random.Random(field)
    for k in range(0, 9):
        n = 1 << k
        w = NR.omega_of(P, k) if k else 1
        x = [rng.randrange(P) for _ in range(n)]
        assert NR.ntt(x, w, P) == NR.dft_naive(x, w, P), k
    x = [rng.randrange(P) for _ in range(4)] + [0] * 12               # zero padding and a coset: forward is the naive sum of the shifted coefficients
    g, w = rng.randrange(2, P), NR.omega_of(P, 4)
    assert NR.forward(x[:4], 4, w, g, P) == NR.dft_naive([c * pow(g, i, P) % P for i, c in enumerate(x)], w, P)


@pytest.mark.parametrize("field", FIELDS)
def test_inverse_undoes_forward(field):
    P = FIELD_MODULI[field]
    rng = random.Random(field + "inv")
    for k in (1, 2, 5, 9):
        w = NR.omega_of(P, k)
        x = [rng.randrange(P) for _ in range(1 << k)]
        for g in shifts(P, rng):
            assert NR.inverse(NR.forward(x, k, w, g, P), k, w, g, P) == x, (k, g)
            assert NR.forward(NR.inverse(x, k, w, g, P), k, w, g, P) == x, (k, g)
        short = x[:1 << (k - 1)]                                     # fewer coefficients than points: they come back zero-padded
        g = rng.randrange(2, P)
        assert NR.inverse(NR.forward(short, k, w, g, P), k, w, g, P) == short + [0] * len(short)


@pytest.mark.parametrize("field", FIELDS)
def test_forward_is_evaluation(field):
    P = FIELD_MODULI[field]
    rng = random.Random(field + "horner")
    for (k_in, k_out) in [(3, 3), (4, 7), (0, 5), (9, 11)]:
        w = NR.omega_of(P, k_out)
        x = [rng.randrange(P) for _ in range(1 << k_in)]
        for g in shifts(P, rng):
            out = NR.forward(x, k_out, w, g, P)
            for j in [0, 1, (1 << k_out) - 1] + [rng.randrange(1 << k_out) for _ in range(8)]:
                assert out[j] == NR.horner(x, g * pow(w, j, P) % P, P), (k_in, k_out, j)


@pytest.mark.parametrize("field", FIELDS)
def test_closed_form_of_geometric_inputs(field):
    P = FIELD_MODULI[field]
    rng = random.Random(field + "geo")
    k, n = 8, 256
    w = NR.omega_of(P, k)
    for g in shifts(P, rng):
        a, b = rng.randrange(2, P), rng.randrange(2, P)
        x = [(pow(a, i, P) + pow(b, i, P)) % P for i in range(n)]
        js = list(range(n))
        assert NR.geometric_forward([a, b], js, k, w, g, P) == NR.forward(x, k, w, g, P)
    xs = [rng.randrange(1, P) for _ in range(33)]
    assert all(x * y % P == 1 for x, y in zip(xs, NR.batch_inverse(xs, P)))
