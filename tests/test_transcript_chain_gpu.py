"""The transcript's outputs plug into the stages where they lie: commit two columns, write the commitments tensor as it
is, squeeze, and hand the device tensors to EvaluationDomain.fold (scalars), open_eval (points from a derive round) and open_witness (vs).
Between the commit and the last stage the test body holds no .cpu(), no .item() and no synchronisation.  Afterwards the same stage calls are
made with the plain model's Python integers (tests/transcript_ref.py over tests/msm_ref.py's commitments): the results are byte-equal, and
the proof buffer is the model's proof.  Batch 3, n = 64, a CommitKey of 64 model points with known logarithms."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import msm_ref as M
import transcript_ref as T

Q, R = T.Q, T.R
BATCH, N = 3, 64
A0, D = 0x1234567890abcdef1122334455667788, 0x0fedcba987654321ffeeddccbbaa9988   # the bases: P_i = [A0 + i D]G
OMEGA = pow(7, (R - 1) >> 6, R)                                                   # the 2^6 domain's generator


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


@pytest.fixture(scope="module")
def model():
    """The bases, the scalars of the two columns per circuit, and the model's commitments."""
    rng = random.Random("transcript/chain")
    bases = M.structured_bases(N, A0, D)
    cols = [[[rng.randrange(R) for _ in range(N)] for _ in range(BATCH)] for _ in range(2)]
    commits = [[M.structured_sum(cols[c][e], A0, D) for c in range(2)] for e in range(BATCH)]
    return bases, cols, commits


def ints_of(t):
    """The integers of an int64 [..., 4] tensor, nested like its leading dimensions."""
    def rec(a):
        return sum(int(a[k]) << (64 * k) for k in range(4)) if a.ndim == 1 else [rec(x) for x in a]
    return rec(t.cpu().numpy().view("uint64"))


@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
def test_the_chain_from_commit_to_witness_without_the_host(H, model, montgomery):
    bases, cols, commits = model
    chip = H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)
    rep = lambda v: T.to_repr(v, R, montgomery)
    ck = H.CommitKey(chip, torch.frombuffer(bytearray(M.point_bytes(bases, montgomery)), dtype=torch.uint8).reshape(N, 64).cuda())
    stack = torch.frombuffer(bytearray(b"".join(M.scalar_bytes(cols[c][e], montgomery) for e in range(BATCH) for c in range(2))),
                             dtype=torch.uint8).reshape(BATCH, 2, N, 32).cuda()
    columns = [(stack[:, 0], 0b11), (stack[:, 1], 0b01)]
    dom = H.EvaluationDomain(chip, 1, 1, rep(R - 1), rep(1))                  # fold and the openings use no root of unity
    tr = H.Transcript(chip, BATCH, (2 + 3) * 32)

    # ---- the device chain: nothing here waits for the GPU or reads from it ----
    pts_out = ck.commit([stack[:, 0], stack[:, 1]])
    ch1, _ = tr.write_points(pts_out, squeeze=2)
    folded, st_fold = dom.fold(stack, ch1[:, 1])                             # a strided view: made contiguous on the device
    _, points = tr.round([], squeeze=1, derive=[(0, rep(1), 0), (0, rep(OMEGA), 0)])
    evals, st_eval = dom.open_eval(columns, points)
    ch3, _ = tr.write_scalars(evals, squeeze=1)
    W, be, st_wit = dom.open_witness(columns, points, ch3[:, 0])
    # ---- from here on the host looks ----
    torch.cuda.synchronize()
    for st in (st_fold, st_eval, st_wit):
        assert st.cpu().tolist() == [0] * BATCH

    assert M.points_from_bytes(pts_out.cpu().numpy().tobytes(), montgomery) == [p for row in commits for p in row]
    models = [T.Transcript() for _ in range(BATCH)]
    x01 = [m.round([("point", p) for p in commits[e]], 2)[1] for e, m in enumerate(models)]
    x1 = [c[1] for c in x01]
    x2 = [m.round([], 1)[1][0] for m in models]
    want_points = [[rep(x), rep(x * OMEGA % R)] for x in x2]
    assert ints_of(ch1) == [[rep(x) for x in c] for c in x01] and ints_of(points) == want_points

    ref_folded, _ = dom.fold(stack, [rep(x) for x in x1])
    ref_evals, _ = dom.open_eval(columns, want_points)
    assert torch.equal(folded, ref_folded) and torch.equal(evals, ref_evals)
    v = [m.round([("scalar", T.from_repr(s, R, montgomery)) for s in ints_of(ref_evals)[e]], 1)[1][0] for e, m in enumerate(models)]
    assert ints_of(ch3) == [[rep(x)] for x in v]
    ref_W, ref_be, _ = dom.open_witness(columns, want_points, [rep(x) for x in v])
    assert torch.equal(W, ref_W) and torch.equal(be, ref_be)
    proof = tr.proof().cpu().numpy()
    for e, m in enumerate(models):
        assert proof[e].tobytes() == m.proof and len(m.proof) == 5 * 32, e
