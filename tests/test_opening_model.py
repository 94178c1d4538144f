"""The plain model of the openings (tests/opening_ref.py) against its own conditions, CPU only: the division really
divides, the remainder is the batched evaluation, the fold with x^n evaluates like the whole h, and -- the verifier's identity -- on a
circuit whose constraints hold the constraint expression at a random x, computed from evaluations alone and folded with y, equals
h(x) * (x^n - 1); after a single fault it does not."""
import copy
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import ntt_ref as NR
import opening_ref as OR
import quotient_ref as QR
from pyref import FIELD_MODULI

P_FR = FIELD_MODULI["bn254_fr"]
K = 5


def poly_mul_linear(W, z, P):
    """W * (X - z), len(W) + 1 coefficients."""
    out = [0] * (len(W) + 1)
    for i, w in enumerate(W):
        out[i + 1] = (out[i + 1] + w) % P
        out[i] = (out[i] - z * w) % P
    return out


@pytest.mark.parametrize("n", [1, 2, 7, 64])
@pytest.mark.parametrize("z", [0, 1, P_FR - 1, None])
def test_the_division_divides(n, z):
    rng = random.Random("opening/division/%d/%s" % (n, z))
    z = rng.randrange(P_FR) if z is None else z
    g = [rng.randrange(P_FR) for _ in range(n)]
    W, rem = OR.kate_division(g, z, P_FR)
    assert len(W) == n and W[-1] == 0
    back = poly_mul_linear(W, z, P_FR)
    back[0] = (back[0] + rem) % P_FR
    assert back == g + [0]                                    # coefficient by coefficient; the top one is the 0 of W[n - 1]
    assert rem == OR.evaluate(g, z, P_FR)


@pytest.mark.parametrize("v", [0, 1, None])
def test_the_remainder_is_the_batched_evaluation(v):
    rng = random.Random("opening/witness/%s" % v)
    v = rng.randrange(P_FR) if v is None else v
    n, masks = 33, [0b011, 0b001, 0b010, 0b011, 0b001]        # point 2 of three has no column
    cols = [[rng.randrange(P_FR) for _ in range(n)] for _ in masks]
    points = [rng.randrange(P_FR) for _ in range(3)]
    wit = OR.witness(cols, masks, points, v, P_FR)
    assert wit[2] is None
    for p in range(2):
        sel = [c for c, m in enumerate(masks) if (m >> p) & 1]
        W, rem = wit[p]
        assert rem == sum(pow(v, idx, P_FR) * OR.evaluate(cols[c], points[p], P_FR) for idx, c in enumerate(sel)) % P_FR
        if v == 0:                                            # 0^0 = 1: only the first column of the point is left
            assert (W, rem) == OR.kate_division(cols[sel[0]], points[p], P_FR)
    assert OR.queries(masks, 3) == [(0, 0), (0, 1), (1, 0), (2, 1), (3, 0), (3, 1), (4, 0)]


def coefficient_form(circ):
    """Every Lagrange column of a circuit in coefficient form (n coefficients), by group."""
    c, P = circ.cfg, circ.P
    w = c.omega(P)
    return {name: [None if col is None else NR.inverse(col, c.k, w, 1, P) for col in group] for name, group in circ.lag.items()}


def h_coefficients(circ):
    """The prover's h: the 4n low coefficients of the quotient on the extended domain (all there are when the constraints hold)."""
    return QR.coefficients(circ.cfg, circ.h(), circ.P)[:4 * circ.cfg.n]


def open_circuit(circ, x, hc=None):
    """The evaluations a verifier is given, by the model: opening_ref.query_plan's queries on the coefficient forms and the folded h."""
    c, P = circ.cfg, circ.P
    coeff = coefficient_form(circ)
    hc = h_coefficients(circ) if hc is None else hc
    coeff["h"] = [OR.fold([hc[i * c.n:(i + 1) * c.n] for i in range(4)], pow(x, c.n, P), P)]
    pts = OR.points_of(c, x, P)
    plan = OR.query_plan(c)
    values = [OR.evaluate(coeff[group][i], pts[p], P) for group, i, mask in plan for p in range(4) if (mask >> p) & 1]
    return OR.evals_of(plan, values)


@pytest.fixture(scope="module")
def circuit():
    return QR.satisfying_circuit(random.Random("opening/%d" % K), P_FR, K)


@pytest.fixture(scope="module")
def x():
    return random.Random("opening/x").randrange(P_FR)


def test_the_fold_evaluates_like_the_whole_h(circuit, x):
    c, P = circuit.cfg, circuit.P
    full = QR.coefficients(c, circuit.h(), P)
    assert not any(full[4 * c.n:]) and any(full[3 * c.n:4 * c.n])
    hc = full[:4 * c.n]
    folded = OR.fold([hc[i * c.n:(i + 1) * c.n] for i in range(4)], pow(x, c.n, P), P)
    assert len(folded) == c.n and OR.evaluate(folded, x, P) == OR.evaluate(hc, x, P)
    assert OR.fold([hc[:c.n], hc[c.n:2 * c.n]], 0, P) == hc[:c.n]                     # s = 0: the first column, 0^0 = 1


def test_the_verifiers_identity_on_a_satisfied_circuit(circuit, x):
    c = circuit.cfg
    assert (len(c.sets), c.args, c.n_extra) == (3, [0, 1, 2, 3, 4], 1)
    plan = OR.query_plan(c)
    assert sum(bin(m).count("1") for _, _, m in plan) == 5 + 1 + 1 + (2 + 3 + 3) + 5 * (2 + 2 + 1) + 15 + 6 + 3 + 1
    evals = open_circuit(circuit, x)
    lhs, rhs = OR.identity_sides(c, evals, circuit.ch, x, circuit.P)
    assert lhs == rhs and lhs != 0
    # the rotated evaluations are read where they belong: each of them changed alone breaks the identity
    for group, i, rot in (("advice", 4, 1), ("perm_z", 0, OR.LAST), ("perm_z", 2, 1), ("lookup_a_perm", 3, -1), ("lookup_z", 1, 1), ("h", 0, 0), ("l", 2, 0)):
        bad = copy.deepcopy(evals)
        bad[group][i][rot] = (bad[group][i][rot] + 1) % circuit.P
        lhs, rhs = OR.identity_sides(c, bad, circuit.ch, x, circuit.P)
        assert lhs != rhs, (group, i, rot)


def _fault_gate_cell(f):
    row = next(i for i in range(f.cfg.u) if f.lag["fixed"][0][i])                      # a row whose sa is nonzero: cell a counts
    f.lag["advice"][0][row] = (f.lag["advice"][0][row] + 1) % f.P


def _fault_copy_cell(f):
    row, col, _, _ = f.pairs[0]
    f.lag["advice"][col][row] = (f.lag["advice"][col][row] + 1) % f.P
    f.solve_s_const()                                                                  # the gate holds again: only the copy constraint is broken


def _fault_swap_a_perm(f):
    ap = f.lag["lookup_a_perm"][0]
    i = next(i for i in range(f.cfg.u - 1) if ap[i] != ap[i + 1])
    ap[i], ap[i + 1] = ap[i + 1], ap[i]


def _fault_z_last(f):
    f.lag["perm_z"][-1][f.cfg.u] = 2


FAULTS = [_fault_gate_cell, _fault_copy_cell, _fault_swap_a_perm, _fault_z_last]


@pytest.mark.parametrize("fault", FAULTS, ids=[f.__name__[7:] for f in FAULTS])
def test_a_single_cell_fault_breaks_the_identity(circuit, x, fault):
    """The prover keeps the 4n low coefficients of whatever the quotient came out as; the numerator is no multiple of X^n - 1 any more."""
    f = copy.deepcopy(circuit)
    fault(f)
    lhs, rhs = OR.identity_sides(f.cfg, open_circuit(f, x), f.ch, x, f.P)
    assert lhs != rhs
