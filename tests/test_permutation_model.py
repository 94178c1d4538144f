"""The plain model of the permutation argument (tests/permutation_ref.py) against the properties halo2's argument has [3P, DESIGN.md section
2e]: distinct labels, Z_0[0] = 1, the sets chain, a satisfied assignment ends at 1 and a damaged one does not; the domain helper gives an
omega of exact order 2^k and refuses a field without such a subgroup.  No device work."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import permutation_ref as PR
from pyref import FIELD_MODULI

M, U = 6, 200


def _synthetic(P, seed):
    rng = random.Random(seed)
    omega, delta = PR.domain(P, 8)
    v, pairs = PR.satisfying_cells(rng, M, U, 40, P)
    assert len(pairs) >= 40
    sigma = PR.sigma_from_pairs(pairs, M, U, delta, omega, P)
    cells = [[v[c][i] for c in range(5)] for i in range(U)]
    return rng, omega, delta, cells, [v[5]], pairs, sigma


@pytest.mark.parametrize("chunk", [1, 2, 6])
def test_satisfied_cycles_end_at_one(chunk):
    P = FIELD_MODULI["bn254_fr"]
    rng, omega, delta, cells, extra, pairs, sigma = _synthetic(P, 5 + chunk)
    lab = PR.labels(M, U, delta, omega, P)
    flat = [x for col in lab for x in col]
    assert len(set(flat)) == M * U                                           # the labels are pairwise distinct
    assert sorted(x for col in sigma for x in col) == sorted(flat)           # sigma permutes them
    assert sum(1 for c in range(M) for i in range(U) if sigma[c][i] != lab[c][i]) >= len(pairs)
    beta, gamma = rng.randrange(1, P), rng.randrange(P)
    Z = PR.product(cells, extra, sigma, [0, 1, 2, 3, 4, 5], chunk, delta, omega, beta, gamma, U, P)
    assert len(Z) == (M + chunk - 1) // chunk and all(len(z) == U + 1 for z in Z)
    assert Z[0][0] == 1
    for s in range(1, len(Z)):
        assert Z[s][0] == Z[s - 1][U]                                        # the sets chain
    assert Z[-1][U] == 1
    if len(Z) > 1:
        assert any(z[U] != 1 for z in Z[:-1])                                # (no set is satisfied on its own: cycles cross the columns)
    for s, z in enumerate(Z):                                                # the recurrence itself, without a division
        cs = range(s * chunk, min(M, (s + 1) * chunk))
        v = PR.columns(cells, extra, [0, 1, 2, 3, 4, 5], U)
        for i in (0, 1, U // 2, U - 1):
            n = d = 1
            for c in cs:
                n = n * (v[c][i] + beta * lab[c][i] + gamma) % P
                d = d * (v[c][i] + beta * sigma[c][i] + gamma) % P
            assert z[i + 1] * d % P == z[i] * n % P


def test_a_changed_cell_does_not_end_at_one():
    P = FIELD_MODULI["bn254_fr"]
    rng, omega, delta, cells, extra, pairs, sigma = _synthetic(P, 99)
    beta, gamma = rng.randrange(1, P), rng.randrange(P)
    row, col = pairs[3][0], pairs[3][1]
    assert col < 5
    cells[row][col] = (cells[row][col] + 1) % P
    for chunk in (1, 2, 6):
        Z = PR.product(cells, extra, sigma, [0, 1, 2, 3, 4, 5], chunk, delta, omega, beta, gamma, U, P)
        assert Z[0][0] == 1 and Z[-1][U] != 1


def test_zero_denominator_ends_the_columns():
    P = FIELD_MODULI["bn254_fr"]
    rng, omega, delta, cells, extra, pairs, sigma = _synthetic(P, 7)
    beta = rng.randrange(1, P)
    gamma = -(cells[17][2] + beta * sigma[2][17]) % P                        # column 2 lies in set 1 of chunk 2
    Z = PR.product(cells, extra, sigma, [0, 1, 2, 3, 4, 5], 2, delta, omega, beta, gamma, U, P)
    assert Z[0] is not None and Z[1] is None and Z[2] is None


def test_first_row_and_pairs_outside_the_image():
    P = FIELD_MODULI["pasta_fp"]
    omega, delta = PR.domain(P, 5)
    pairs = [(3, 0, 1, 1), (4, 2, PR.H2R_COPY_SRC[0], 5), (9, 4, 3, 0)]
    sigma = PR.sigma_from_pairs(pairs, 5, 26, delta, omega, P)
    lab = PR.labels(5, 26, delta, omega, P)
    moved = {(c, i) for c in range(5) for i in range(26) if sigma[c][i] != lab[c][i]}
    assert moved == {(0, 3), (1, 1), (4, 9)}                                 # one cycle of three cells; the operand pair is dropped
    v = PR.columns([[1, 2, 3, 4, 5], [6, 7, 8, 9, 10]], None, [4, 0], 26, first_row=7)
    assert v[0][7:9] == [5, 10] and v[1][7:9] == [1, 6] and sum(v[0]) == 15 and sum(v[1]) == 7


@pytest.mark.parametrize("field", ["bn254_fr", "pasta_fp", "pasta_fq"])
def test_domain_has_exact_order(field):
    P = FIELD_MODULI[field]
    for k in (1, 8, 13, 17):
        omega, delta = PR.domain(P, k)
        assert pow(omega, 1 << k, P) == 1 and pow(omega, 1 << (k - 1), P) != 1
        S = ((P - 1) & -(P - 1)).bit_length() - 1
        assert pow(delta, (P - 1) >> S, P) == 1 and delta != 1              # delta lies in the odd-order subgroup: delta^c is never a power of omega


def test_domain_refuses_a_field_without_the_subgroup():
    P = FIELD_MODULI["bn254_fq"]
    assert (P - 1) % 4 == 2
    PR.domain(P, 1)
    with pytest.raises(ValueError):
        PR.domain(P, 2)
