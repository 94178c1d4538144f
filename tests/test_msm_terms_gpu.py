"""h2r_msm_terms on the device (prover.msm_terms) byte for byte against the plain model (tests/msm_ref.py), bn254_fr
(bn256 G1) in both representations: out[e] = sum_t s[e][t] P[e][t] over bases that differ per circuit.  Every base has a known discrete
logarithm (P_i = [A0 + i D]G), so a sum's expectation is ONE scalar multiplication; T runs over the lane stride's wrap (256), ragged last
rounds and the call's maximum of 4,096 terms, the scalars and the bases come per circuit or shared, and the output lies between sentinel-filled guards."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import msm_ref as M

REPRS, IDS = [False, True], ["canonical", "montgomery"]
SENTINEL, GUARD = 0xAB, 2
A0, D = 0x1234567890abcdef1122334455667788, 0x0fedcba987654321ffeeddccbbaa9988
R = M.R_ORDER
TS = [1, 2, 63, 64, 65, 255, 256, 257, 600, 4096]                               # 4096: the call's maximum, 16 terms per lane
CACHE = {}


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def structured(n):
    if "bases" not in CACHE:
        CACHE["bases"] = M.structured_bases(3 * max(TS), A0, D)
    return CACHE["bases"][:n], [(A0 + i * D) % R for i in range(n)]


def dev_bytes(raw, shape):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(shape).cuda()


def run(H, montgomery, scalars, bases, T, batch, shared_s, shared_b, status=None):
    """scalars: [batch or 1][T] integers, bases: [batch or 1][T] points -> the device's out [batch] as points, between checked guards."""
    chip = H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)
    s = dev_bytes(b"".join(M.scalar_bytes(row, montgomery) for row in scalars), (len(scalars), T, 32))
    b = dev_bytes(b"".join(M.point_bytes(row, montgomery) for row in bases), (len(bases), T, 64))
    buf = torch.full((batch + 2 * GUARD, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    st = None if status is None else torch.tensor(status, dtype=torch.uint8, device="cuda")
    H.prover.msm_terms(chip, s, b, T, batch, 0 if shared_s else T * 32, 0 if shared_b else T * 64, buf[GUARD:GUARD + batch], st)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + batch:] == SENTINEL).all(), "a write outside out[e]"
    if st is not None:
        assert st.cpu().tolist() == list(status), "the status is never written"
    return [None if status is not None and status[e] else M.points_from_bytes(bytes(raw[GUARD + e]), montgomery)[0] for e in range(batch)], raw[GUARD:GUARD + batch]


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("T", TS)
def test_sums_over_structured_bases(H, montgomery, T):
    rng = random.Random("msm_terms/%d" % T)                                      # (the same inputs in both representations)
    for batch in (1, 3):
        pts, logs = structured(batch * T)
        for shared_s, shared_b in ((False, False), (True, False), (False, True), (True, True)):
            ns, nb = (1 if shared_s else batch), (1 if shared_b else batch)
            scalars = [[rng.randrange(R) for _ in range(T)] for _ in range(ns)]
            scalars[0][0] = 0
            scalars[-1][T - 1] = R - 1
            got, _ = run(H, montgomery, scalars, [pts[e * T:(e + 1) * T] for e in range(nb)], T, batch, shared_s, shared_b)
            for e in range(batch):
                srow, lrow = scalars[0 if shared_s else e], logs[(0 if shared_b else e) * T:][:T]
                want = M.mul_g(sum(s * l for s, l in zip(srow, lrow)) % R)
                assert got[e] == want, (T, batch, shared_s, shared_b, e)


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_edge_scalars_and_base_pairs(H, montgomery):
    rng = random.Random("msm_terms/edge")
    P1, P2 = M.mul_g(rng.randrange(R)), M.mul_g(rng.randrange(R))
    edge = [0, 1, R - 1, R, (1 << 256) - 1]
    cases = [([s], [P1]) for s in edge]
    cases += [([1, 1], [P1, P1]), ([1, 1], [P1, M.neg(P1)]), ([5, 5], [P1, P1]), ([7, R - 7], [P1, P1]), ([3, 4], [M.IDENT, P2]), ([3, 4], [P1, M.IDENT]),
              ([0, 0], [P1, P2]), ([9], [M.IDENT]), (edge, [P1, P2, P1, P2, P1])]
    for scalars, bases in cases:
        got, _ = run(H, montgomery, [scalars], [bases], len(scalars), 1, False, False)
        assert got[0] == M.naive_msm(scalars, bases), (scalars, bases)
    # 257 copies of one point and 257 alternating signs: doublings inside the tree, the identity out of it
    got, _ = run(H, montgomery, [[1] * 257], [[P1] * 257], 257, 1, False, False)
    assert got[0] == M.mul(257, P1)
    got, raw = run(H, montgomery, [[1] * 256], [[P1, M.neg(P1)] * 128], 256, 1, False, False)
    assert got[0] == M.IDENT and not raw.any()


def test_a_flagged_circuit_is_skipped(H):
    pts, logs = structured(3 * 65)
    scalars = [[t + 1 + e for t in range(65)] for e in range(3)]
    got, raw = run(H, True, scalars, [pts[e * 65:(e + 1) * 65] for e in range(3)], 65, 3, False, False, status=[0, 9, 0])
    assert (raw[1] == SENTINEL).all(), "a circuit flagged on entry keeps its bytes"
    for e in (0, 2):
        assert got[e] == M.mul_g(sum(s * l for s, l in zip(scalars[e], logs[e * 65:(e + 1) * 65])) % R)
