"""The verifier's identity at a random point, on the recorded circuits of tests/test_prover_chain_gpu.py (k = 10, the extended domain 2^13,
three circuits).  After the chain has produced h, every column goes to coefficient form (lagrange_to_coeff), the
pieces of h are folded with x^n (EvaluationDomain.fold) and everything is evaluated at x and its rotations (open_eval) with this circuit's
query pattern (opening_ref.query_plan).  From the returned evaluations ALONE the host computes the constraint expression at x
(opening_ref.constraint_at_point), folds it with y and compares with h(x) * (x^n - 1).

That goes through every export from the advice image to the quotient by the route a verifier takes -- another one than the row checks,
the Z[u] = 1 statuses and "no coefficient of h of index >= 4n".  What it establishes is that the kernels' conventions agree with each
other at a random point, not that the query order is upstream halo2's transcript order: the order is the caller's."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import advice_ref as AR
import opening_ref as OR
import quotient_ref as QR
from test_prover_chain_gpu import B, N_ROWS, Chain, H  # noqa: F401  (H: the module's fixture)
from test_lookup_product import in_repr

R256 = 1 << 256


def ints_of_words(t, P, montgomery):
    """int64 [..., 4] device tensor of elements in the chip's representation -> nested lists of canonical integers."""
    a = t.cpu().numpy()
    flat = a.reshape(-1, 4).view(np.uint64).tolist()
    vals = [w0 | w1 << 64 | w2 << 128 | w3 << 192 for w0, w1, w2, w3 in flat]
    assert all(v < P for v in vals), "not the canonical representative"
    if montgomery:
        rinv = pow(R256, -1, P)
        vals = [v * rinv % P for v in vals]
    return np.array(vals, dtype=object).reshape(a.shape[:-1]).tolist()


def open_chain(c, out, xs):
    """The evaluations of one chain run at the per-circuit points of xs: ([per circuit the flat values of the query list], the plan, h(x) of
    the whole 4n-coefficient h by the same export)."""
    P, cfg, dom, mont = c.P, c.cfg, c.dom, c.mont
    coeff = {name: dom.lagrange_to_coeff(t) for name, t in out["lag"].items()}
    coeff["fixed"], coeff["sigma"] = dom.lagrange_to_coeff(c.fixed_dev), dom.lagrange_to_coeff(c.sigma_dev)
    coeff["l"] = dom.lagrange_to_coeff(c.columns_tensor(QR.vanishing_lagrange(cfg)))
    hc = dom.extended_to_coeff(out["h"])                                                  # [B, 2^13, 32]: the 4n low coefficients are h's pieces
    pieces = hc[:, :4 * N_ROWS].unflatten(1, (4, N_ROWS))
    folded, st = dom.fold(pieces, in_repr([pow(x, N_ROWS, P) for x in xs], P, mont))
    assert st.cpu().tolist() == [0] * B and tuple(folded.shape) == (B, N_ROWS, 32)
    coeff["h"] = folded.unsqueeze(1)
    plan = OR.query_plan(cfg)
    assert len(plan) == 5 + 3 + 15 + 15 + 5 + 3 + 1
    columns = [(coeff[group][i] if group in QR.KEY else coeff[group][:, i], mask) for group, i, mask in plan]
    points = [in_repr(OR.points_of(cfg, x, P), P, mont) for x in xs]
    evals, st = dom.open_eval(columns, points)
    assert st.cpu().tolist() == [0] * B
    whole, st = dom.open_eval([(hc[:, :4 * N_ROWS], 1)], [[p[0]] for p in points])        # n_coeffs = 2^12
    assert st.cpu().tolist() == [0] * B
    return ints_of_words(evals, P, mont), plan, [row[0] for row in ints_of_words(whole, P, mont)]


def sides(c, plan, values, b, x):
    return OR.identity_sides(c.cfg, OR.evals_of(plan, values), tuple(v[b] for v in c.ch), x, c.P)


@pytest.mark.parametrize("field,montgomery", [("bn254_fr", False), ("bn254_fr", True), ("pasta_fq", True)], ids=["bn254_fr-canonical", "bn254_fr-montgomery", "pasta_fq-montgomery"])
def test_the_verifiers_identity_on_recorded_circuits(H, field, montgomery):
    c = Chain(H, field, montgomery)
    out = c.run()
    assert out["status"] == [0] * B and out["st_pz"] == [0] * B and out["st_lz"] == [0] * B
    rng = random.Random("open/chain/" + field)
    xs = [rng.randrange(c.P) for _ in range(B)]
    values, plan, whole = open_chain(c, out, xs)
    assert len(values[0]) == sum(bin(m).count("1") for _, _, m in plan) == 6 + 8 + 25 + 24
    for b in range(B):
        lhs, rhs = sides(c, plan, values[b], b, xs[b])
        assert lhs == rhs and lhs != 0, "circuit %d" % b
        assert values[b][-1] == whole[b], "the folded h at x is not the whole h at x (circuit %d)" % b
    # one changed evaluation: each of the rotated ones, the folded h and a key column's, alone
    flat = [(g, i, OR.POINT_ROT[p]) for g, i, m in plan for p in range(4) if (m >> p) & 1]
    for probe in (("advice", 4, 1), ("perm_z", 0, OR.LAST), ("perm_z", 2, 1), ("lookup_a_perm", 3, -1), ("lookup_z", 0, 1), ("sigma", 4, 0), ("h", 0, 0)):
        bad = list(values[1])
        bad[flat.index(probe)] = (bad[flat.index(probe)] + 1) % c.P
        lhs, rhs = sides(c, plan, bad, 1, xs[1])
        assert lhs != rhs, probe


def test_one_changed_advice_cell_breaks_the_identity(H):
    c = Chain(H, "bn254_fr")
    row, col = next((r, q) for (r, q, _, _) in c.inside if c.kinds[r] == AR.ROW_MUL_ADD)     # a cell that a copy pair names, on a row without a lookup
    out = c.run(image_fault=(1, row, col))
    xs = [random.Random("open/chain/fault").randrange(c.P) for _ in range(B)]
    values, plan, _ = open_chain(c, out, xs)
    for b in range(B):
        lhs, rhs = sides(c, plan, values[b], b, xs[b])
        assert (lhs == rhs) == (b != 1), "circuit %d" % b
