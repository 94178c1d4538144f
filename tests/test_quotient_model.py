"""The plain model of the vanishing argument's quotient (tests/quotient_ref.py) against the prover's own soundness
condition, CPU only: for a circuit whose constraints hold the numerator is divisible by X^n - 1, so h is a polynomial of degree < 4n (every
constraint has degree <= 5, the extended domain has 8n points) and its coefficients of index >= 4n vanish; after any single fault they do
not.  The term order is pinned by a case small enough to work out by hand."""
import copy
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import quotient_ref as QR
from pyref import FIELD_MODULI

P_FR = FIELD_MODULI["bn254_fr"]


def high_coefficients(circ):
    c = circ.cfg
    return QR.coefficients(c, circ.h(), circ.P)[4 * c.n:]


@pytest.fixture(scope="module")
def circuits():
    return {k: QR.satisfying_circuit(random.Random("quotient/%d" % k), P_FR, k) for k in (4, 5)}


@pytest.mark.parametrize("k", [4, 5])
def test_a_satisfied_circuit_has_a_polynomial_quotient(circuits, k):
    circ = circuits[k]
    c = circ.cfg
    assert (c.log_ext, c.u, len(c.sets), c.args) == (k + 3, (1 << k) - 6, 3, [0, 1, 2, 3, 4])
    assert circ.constrained and circ.pairs and any(circ.lag["fixed"][7][:c.u])          # range-constrained cells, copy cycles, se_next rows
    h = circ.h()
    coeffs = QR.coefficients(c, h, circ.P)
    assert not any(coeffs[4 * c.n:])
    assert any(coeffs[3 * c.n:4 * c.n])                                                  # ... and the bound is no looser than it has to be


@pytest.mark.parametrize("chunk_len,mask", [(1, 0), (3, 1 << 2), (6, 31)])
def test_other_set_sizes_and_lookup_masks(chunk_len, mask):
    circ = QR.satisfying_circuit(random.Random("quotient/sets/%d" % chunk_len), P_FR, 4, chunk_len=chunk_len, lookup_mask=mask)
    assert len(circ.cfg.sets) == {1: 6, 3: 2, 6: 1}[chunk_len]
    if chunk_len <= 3:
        assert not any(high_coefficients(circ))
    else:   # six columns in one set: degree 8 > the domain allows; only the evaluation is defined, which the device tests compare
        assert len(circ.h()) == circ.cfg.N


def _fault_gate_cell(f, rng):
    c = f.cfg
    row = next(i for i in range(c.u) if f.lag["fixed"][0][i])                            # a row whose sa is nonzero: cell a counts
    f.lag["advice"][0][row] = (f.lag["advice"][0][row] + 1) % f.P


def _fault_copy_cell(f, rng):
    row, col, _, _ = f.pairs[0]
    assert col < 5
    f.lag["advice"][col][row] = (f.lag["advice"][col][row] + 1) % f.P
    f.solve_s_const()                                                                    # the gate holds again: only the copy constraint is broken


def _fault_out_of_range(f, rng):
    in_cycle = {(col, row) for (row, col, _, _) in f.pairs} | {(sc, sr) for (_, _, sr, sc) in f.pairs}
    col, row = next(cell for cell in f.constrained if cell not in in_cycle)
    f.lag["advice"][col][row] = 1 << max(f.lcfg.bit_lens)                                # one past the widest range; A' / S' / Z left alone
    f.solve_s_const()


def _fault_swap_a_perm(f, rng):
    ap = f.lag["lookup_a_perm"][0]
    i = next(i for i in range(f.cfg.u - 1) if ap[i] != ap[i + 1])
    ap[i], ap[i + 1] = ap[i + 1], ap[i]


def _fault_z0_first(f, rng):
    f.lag["perm_z"][0][0] = 2


def _fault_z_last(f, rng):
    f.lag["perm_z"][-1][f.cfg.u] = 2


FAULTS = [_fault_gate_cell, _fault_copy_cell, _fault_out_of_range, _fault_swap_a_perm, _fault_z0_first, _fault_z_last]


@pytest.mark.parametrize("fault", FAULTS, ids=[f.__name__[7:] for f in FAULTS])
def test_a_single_fault_leaves_no_polynomial(circuits, fault):
    f = copy.deepcopy(circuits[4])
    fault(f, random.Random(fault.__name__))
    assert any(high_coefficients(f))


# ---- the term order, by hand ----------------------------------------------------------------------------------------------------------------
# F_17, k = 1 (n = 2), log_ext = 2 (N = 4, r = 2), no blinding rows (u = 1); omega_ext = 4 (4^2 = -1), zeta = 3, delta = 2; one permutation
# column (advice column 0), one set; lookup argument 0 on advice column 1.  Fixed columns 0..8 = the gate's, 9 / 10 = tag / enable, 11 / 12 =
# table tag / value.  Points X_j = 3 * 4^j = 3, 12, 14, 5; X_j^2 - 1 = 8, 7, 8, 7 with inverses 15, 5.
HAND_P = 17
HAND_CFG = QR.Config(1, 2, 0, 4, 3, 2, 13, range(9), [0], 1, 1, (1, 0, 0, 0, 0), (9, 0, 0, 0, 0), (10, 0, 0, 0, 0), 11, 12)
HAND_COLS = dict(
    advice=[[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16], [2, 4, 6, 8]], extra=[], perm_z=[[3, 5, 7, 9]],
    lookup_a_perm=[[2, 3, 5, 7]] + [None] * 4, lookup_s_perm=[[11, 13, 1, 4]] + [None] * 4, lookup_z=[[6, 10, 12, 14]] + [None] * 4,
    fixed=[[1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 6], [4, 5, 6, 7], [5, 6, 7, 8], [6, 7, 8, 9], [7, 8, 9, 10], [8, 9, 10, 11], [9, 10, 11, 12],
           [1, 0, 2, 1], [1, 1, 0, 1], [3, 2, 1, 0], [4, 5, 6, 7]],
    sigma=[[10, 11, 12, 13]], l=[[2, 3, 4, 5], [6, 7, 8, 9], [10, 11, 12, 13]])
HAND_CH = (2, 3, 5, 7)   # theta, beta, gamma, y


def test_the_term_order_by_hand():
    """Point j = 1 (X = 12; rotations by r = 2: +1 row -> index 3, -1 row -> index 3): every term worked out from the definition."""
    P = HAND_P
    gate = (2 * 2 + 3 * 6 + 4 * 10 + 5 * 14 + 6 * 4 + 7 * (2 * 6) + 8 * (10 * 14) + 9 * 8 + 10) % P      # s_i v_i, s_mul_ab ab, s_mul_cd cd, se_next e<+1>, s_const
    perm = [3 * (1 - 5) % P,                                                             # l0 (1 - Z_0)
            7 * (5 * 5 - 5) % P,                                                         # l_last (Z^2 - Z)
            11 * (9 * (2 + 3 * 11 + 5) - 5 * (2 + 1 * 3 * 12 + 5)) % P]                  # l_active (Z<+1> (v + beta sigma + gamma) - Z (v + delta^0 beta X + gamma))
    A, S = 2 * 0 + 1 * 6, 2 * 2 + 5                                                       # theta tag + enable v_1; theta table_tag + table_value
    look = [3 * (1 - 10) % P,                                                            # l0 (1 - Z)
            7 * (10 * 10 - 10) % P,                                                      # l_last (Z^2 - Z)
            11 * (14 * (3 + 3) * (13 + 5) - 10 * (A + 3) * (S + 5)) % P,                 # l_active (Z<+1> (A' + beta)(S' + gamma) - Z (A + beta)(S + gamma))
            3 * (3 - 13) % P,                                                            # l0 (A' - S')
            11 * (3 - 13) * (3 - 7) % P]                                                 # l_active (A' - S')(A' - A'<-1>)
    want = [gate] + perm + look
    assert want == [14, 5, 4, 14, 7, 1, 1, 4, 15]
    assert QR.terms(HAND_CFG, HAND_COLS, HAND_CH, 1, P) == want
    acc = 0
    for t in want:
        acc = (acc * 7 + t) % P
    assert acc == 2 and QR.vanishing_inverses(HAND_CFG, P) == [15, 5]   # 14, 1, 11, 6, 15, 4, 12, 3, 2
    assert QR.quotient(HAND_CFG, HAND_COLS, HAND_CH, P)[1] == 2 * 5 % P == 10
    # a swapped pair of terms, or Horner from the other end, gives another value: the order is observable
    swapped = want[:1] + [want[2], want[1]] + want[3:]
    acc2 = 0
    for t in swapped:
        acc2 = (acc2 * 7 + t) % P
    assert acc2 != acc


def test_the_whole_hand_case():
    assert QR.quotient(HAND_CFG, HAND_COLS, HAND_CH, HAND_P) == HAND_H


HAND_H = [None] * 4   # filled below from the definition written out once more, point by point, without quotient_ref.terms


def _hand_point(j):
    P, c, N, r = HAND_P, HAND_COLS, 4, 2
    th, be, ga, y = HAND_CH
    X = 3 * pow(4, j, P) % P
    nx, pv = (j + r) % N, (j - r) % N
    a = [col[j] for col in c["advice"]]
    f = [col[j] for col in c["fixed"]]
    l0, ll, la = (col[j] for col in c["l"])
    z, ap, sp, lz = c["perm_z"][0], c["lookup_a_perm"][0], c["lookup_s_perm"][0], c["lookup_z"][0]
    ts = [f[0] * a[0] + f[1] * a[1] + f[2] * a[2] + f[3] * a[3] + f[4] * a[4] + f[5] * a[0] * a[1] + f[6] * a[2] * a[3] + f[7] * c["advice"][4][nx] + f[8],
          l0 * (1 - z[j]), ll * (z[j] * z[j] - z[j]),
          la * (z[nx] * (a[0] + be * c["sigma"][0][j] + ga) - z[j] * (a[0] + be * X + ga)),
          l0 * (1 - lz[j]), ll * (lz[j] * lz[j] - lz[j]),
          la * (lz[nx] * (ap[j] + be) * (sp[j] + ga) - lz[j] * (th * f[9] + f[10] * a[1] + be) * (th * f[11] + f[12] + ga)),
          l0 * (ap[j] - sp[j]), la * (ap[j] - sp[j]) * (ap[j] - ap[pv])]
    acc = 0
    for t in ts:
        acc = (acc * y + t) % P
    return acc * pow(X * X - 1, -1, P) % P


HAND_H[:] = [_hand_point(j) for j in range(4)]
