"""Commitments and openings together (CommitKey.commit over EvaluationDomain.open_witness; DESIGN.md sections 2h and 2i): the KZG opening
identity with a KNOWN tau in place of a pairing.  With bases [tau^i]G a commitment is C_f = [f(tau)]G, so for every point p that some
column's mask queries, the device's W_p, batch_eval_p and commitments satisfy, in the plain model (tests/msm_ref.py),
    [tau - z_p] C_{W_p}  ==  sum_{c in Q_p} v^idx(c) C_c  -  [batch_eval_p]G.
The columns, masks and points are those of tests/test_open_gpu.py; one changed coefficient on the device breaks the identity."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import msm_ref as M
from pyref import FIELD_MODULI
from test_open_gpu import KEY, MASKS, column_tensor, domain, make_case, scalars

N, BATCH = 1500, 2
P = FIELD_MODULI["bn254_fr"]
CACHE = {}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def setup_once():
    if not CACHE:
        assert P == M.R_ORDER
        rng = random.Random("commit/chain")
        tau = rng.randrange(2, P)
        CACHE["tau"] = tau
        CACHE["bases"] = M.mul_g_batch([pow(tau, i, P) for i in range(N)])
        CACHE["points"] = [[rng.randrange(P) for _ in range(4)] for _ in range(BATCH)]
        CACHE["vs"] = [rng.randrange(P) for _ in range(BATCH)]
    return CACHE


def host_points(t, montgomery):
    """int64 [..., 2, 4] on the device -> nested lists of affine points."""
    a = t.cpu().numpy()
    pts = M.points_from_bytes(a.tobytes(), montgomery)
    return [pts[i * a.shape[1]:(i + 1) * a.shape[1]] for i in range(a.shape[0])]


def identity_holds(C, CW, be, e, p, z, v, tau):
    """[tau - z] C_W == sum v^idx C_c - [batch_eval]G for circuit e, point p."""
    sel = [c for c, m in enumerate(MASKS) if (m >> p) & 1]
    rhs = M.jmul_g(-be % P)
    for idx, c in enumerate(sel):
        rhs = M.jadd(rhs, M.jmul(pow(v, idx, P), C[e][c]))
    return M.mul((tau - z) % P, CW[e][p]) == M.to_affine(rhs)


@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
def test_kzg_opening_identity_with_a_known_tau(H, montgomery):
    cs = setup_once()
    tau, points, vs = cs["tau"], cs["points"], cs["vs"]
    dom = domain(H, "bn254_fr", montgomery)
    cols, of, qs, evals = make_case("commit/chain", P, N, BATCH, MASKS, points, KEY)
    tensors = [column_tensor(cols[c][0], P, montgomery) if c == KEY else column_tensor(cols[c], P, montgomery, BATCH) for c in range(len(MASKS))]
    ck = H.CommitKey(dom.chip, torch.frombuffer(bytearray(M.point_bytes(cs["bases"], montgomery)), dtype=torch.uint8).reshape(N, 64).cuda())
    C_dev = ck.commit(tensors)
    W, be_dev, st = dom.open_witness(list(zip(tensors, MASKS)), [scalars(row, P, montgomery) for row in points], scalars(vs, P, montgomery))
    CW_dev = ck.commit([W[:, p] for p in range(4)])
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0] * BATCH
    C, CW = host_points(C_dev, montgomery), host_points(CW_dev, montgomery)
    rinv = pow(1 << 256, -1, P) if montgomery else 1
    be = [[int.from_bytes(be_dev[e, p].cpu().numpy().tobytes(), "little") * rinv % P for p in range(4)] for e in range(BATCH)]
    # the commitments are the model's: C_c = [f_c(tau)]G (one column per kind is enough; the identity below covers the rest)
    assert C[0][0] == M.mul_g(sum(a * pow(tau, i, P) for i, a in enumerate(of(0, 0))) % P)
    assert C[0][KEY] == C[1][KEY]
    checked = 0
    for e in range(BATCH):
        for p in range(4):
            if not any((m >> p) & 1 for m in MASKS):
                assert CW[e][p] == M.IDENT                        # no column queries the point: W stays zero, its commitment the identity
                continue
            assert identity_holds(C, CW, be[e][p], e, p, points[e][p], vs[e], tau), (e, p)
            checked += 1
    assert checked == 3 * BATCH
    # one changed coefficient of one column on the device: its commitment no longer opens
    bad = tensors[0].clone()
    bad[0, 7, 0] ^= 1
    C_bad = host_points(ck.commit([bad] + tensors[1:]), montgomery)
    assert C_bad[0][0] != C[0][0] and C_bad[1] == C[1]
    assert not identity_holds(C_bad, CW, be[0][0], 0, 0, points[0][0], vs[0], tau)
    assert identity_holds(C_bad, CW, be[1][0], 1, 0, points[1][0], vs[1], tau)
