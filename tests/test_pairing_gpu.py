"""h2r_pairing_products on the device (prover.PairingKey, prover.pairing_check) against the plain model of
tests/pairing_ref.py, both representations.  Expected values come from known logarithms: circuit e pairs P_ej = [a_ej]G1 with the key's
[b_j]G2, so its product is g^(sum_j +-a_ej b_j) with g = e(G1, G2) made once per module; a handful of circuits also go through the model's
Miller loop and final exponentiation directly.  A workgroup serves 8 circuits: batches of 1, 7, 8, 9 and 17; 1, 2 and 4 pairs; every
negate_mask at two pairs; sentinel-filled outputs with guard rows; a padding row between circuits; identity operands; a status on entry, a
coordinate = q, an off-curve point and both in one circuit of a full workgroup; gt or accept left out; two calls on one stream."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import msm_ref as M
import pairing_ref as P
from test_create_proof_gpu import H   # noqa: F401  (the fixture)

REPRS, IDS = [False, True], ["canonical", "montgomery"]
SENTINEL = 0xAB
WG = 8                                                   # circuits of a workgroup
E_SHAPE, E_ASSERTION = P.E_SHAPE, P.E_ASSERTION
RNG = random.Random("pairing/gpu")
BS = [1] + [RNG.randrange(2, P.R) for _ in range(3)]     # the key's points [b_j]G2; b_0 = 1: G2 itself
AS = [[RNG.randrange(1, P.R) for _ in range(4)] for _ in range(2 * WG + 1)]   # circuit e's logarithms, whatever the batch
CACHE = {}


def g_pow(k):
    """g^k, g = e(G1, G2)"""
    if "g" not in CACHE:
        CACHE["g"] = P.pairing(M.G, P.G2)
    k %= P.R
    if k not in CACHE:
        CACHE[k] = P.pow12(CACHE["g"], k) if k else P.ONE
    return CACHE[k]


def key(H, montgomery, J):
    if (montgomery, J) not in CACHE:
        chip = CACHE.setdefault(("chip", montgomery), None) or H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)
        CACHE[("chip", montgomery)] = chip
        pts = [P.g2_mul(b, P.G2) for b in BS[:J]]
        CACHE[(montgomery, J)] = H.prover.PairingKey(chip, [P.g2_bytes(p, montgomery) for p in pts])
    return CACHE[(montgomery, J)]


def logs(batch, J, accepting=()):
    """a[e][j]; for e in `accepting` (J >= 2) the last one is solved so that sum_j a_ej b_j = 0 under mask 0"""
    a = [list(AS[e][:J]) for e in range(batch)]
    for e in accepting:
        a[e][J - 1] = -sum(x * b for x, b in zip(a[e][:J - 1], BS)) * pow(BS[J - 1], -1, P.R) % P.R
    return a


def points_tensor(pts, montgomery, pad_rows=0):
    """uint8 [batch, J (+ pad_rows of sentinel bytes), 64]"""
    raw = b"".join(M.point_bytes(row, montgomery) + bytes([SENTINEL]) * (64 * pad_rows) for row in pts)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(len(pts), len(pts[0]) + pad_rows, 64).cuda()


def run(H, pkey, points, mask=0, status_in=None, want_gt=True, want_accept=True):
    """pairing_check into sentinel-filled outputs inside guard rows -> (accept list, gt rows, status list)"""
    batch = int(points.shape[0])
    gt_buf = torch.full((batch + 2, 384), SENTINEL, dtype=torch.uint8, device="cuda")
    acc_buf = torch.full((batch + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    status = torch.tensor(status_in or [0] * batch, dtype=torch.uint8, device="cuda")
    gt, accept = gt_buf[1:batch + 1] if want_gt else None, acc_buf[16:16 + batch] if want_accept else None
    out = H.prover.pairing_check(pkey, points, mask, status, out=(accept, gt))
    torch.cuda.synchronize()
    assert out[0] is accept and out[1] is gt
    g, a = gt_buf.cpu().numpy(), acc_buf.cpu().tolist()
    assert bytes(g[0]) == bytes(g[-1]) == bytes([SENTINEL]) * 384 and a[:16] == a[16 + batch:] == [SENTINEL] * 16, "a guard byte was written"
    return a[16:16 + batch], [bytes(r) for r in g[1:batch + 1]], status.cpu().tolist()


def expected(a, J, mask, montgomery):
    """(accept list, gt rows) from the logarithms"""
    ks = [sum((-x if (mask >> j) & 1 else x) * BS[j] for j, x in enumerate(row[:J])) % P.R for row in a]
    return [int(k == 0) for k in ks], [P.fq12_bytes(g_pow(k), montgomery) for k in ks]


def points_of(a):
    return [[M.mul_g(x) if x else M.IDENT for x in row] for row in a]


@pytest.mark.parametrize("J", [1, 2, 4])
@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_batches_around_a_workgroup(H, montgomery, J):
    pkey = key(H, montgomery, J)
    for batch in (1, WG - 1, WG, WG + 1, 2 * WG + 1):
        a = logs(batch, J, accepting=[e for e in (0, WG - 1, WG, 2 * WG) if e < batch] if J > 1 else ())
        accept, gt, status = run(H, pkey, points_tensor(points_of(a), montgomery))
        want_accept, want_gt = expected(a, J, 0, montgomery)
        assert status == [0] * batch and accept == want_accept and gt == want_gt, (J, batch)
        assert J == 1 or sum(accept) == len([e for e in (0, WG - 1, WG, 2 * WG) if e < batch])


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_the_models_own_walk(H, montgomery):
    """a handful of circuits through the model's Miller loop and final exponentiation, not through logarithms"""
    pkey = key(H, montgomery, 2)
    tabs = [P.prepare(P.g2_mul(b, P.G2)) for b in BS[:2]]
    a = logs(3, 2, accepting=[1])
    pts = points_of(a)
    accept, gt, status = run(H, pkey, points_tensor(pts, montgomery), 0)
    for e in range(3):
        ok, want = P.check(list(zip(pts[e], tabs)))
        assert status[e] == 0 and accept[e] == int(ok) == int(e == 1) and gt[e] == P.fq12_bytes(want, montgomery)
    assert bytes(pkey.tables.cpu().numpy()) == b"".join(P.table_bytes(t, montgomery) for t in tabs)


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_every_negate_mask_and_a_padding_row(H, montgomery):
    pkey = key(H, montgomery, 2)
    batch = WG + 1
    a = logs(batch, 2)
    a[3][1] = a[3][0] * BS[0] * pow(BS[1], -1, P.R) % P.R          # accepted under masks 1 and 2 only
    for pad in (0, 1):
        points = points_tensor(points_of(a), montgomery, pad_rows=pad)[:, :2]
        for mask in range(4):
            accept, gt, status = run(H, pkey, points, mask)
            want_accept, want_gt = expected(a, 2, mask, montgomery)
            assert status == [0] * batch and accept == want_accept and gt == want_gt, (pad, mask)
            assert accept[3] == int(mask in (1, 2))


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_identity_operands(H, montgomery):
    pkey = key(H, montgomery, 2)
    a = logs(WG, 2)
    a[1][0] = 0                                                      # the identity in the first place, in the second, in both
    a[4][1] = 0
    a[6] = [0, 0]
    accept, gt, status = run(H, pkey, points_tensor(points_of(a), montgomery), 2)
    want_accept, want_gt = expected(a, 2, 2, montgomery)
    assert status == [0] * WG and accept == want_accept and gt == want_gt
    assert accept[6] == 1 and gt[6] == P.fq12_bytes(P.ONE, montgomery) and sum(accept) == 1


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_statuses(H, montgomery):
    pkey = key(H, montgomery, 2)
    a = logs(WG, 2, accepting=[2, 5])
    pts = points_of(a)
    clean = run(H, pkey, points_tensor(pts, montgomery))
    assert clean[0] == [0, 0, 1, 0, 0, 1, 0, 0]
    untouched = bytes([SENTINEL]) * 384

    def rest(got, e):
        return [x[:e] + x[e + 1:] for x in got]

    # a status set on entry: accept 0, gt untouched, the byte not cleared, neighbours byte-equal
    got = run(H, pkey, points_tensor(pts, montgomery), status_in=[0, 0, 0, 0, 0, 7, 0, 0])
    assert got[2][5] == 7 and got[0][5] == 0 and got[1][5] == untouched and rest(got, 5) == rest(clean, 5)
    # a coordinate = q; an off-curve point; both in one circuit: H2R_E_SHAPE wins, whichever pair holds which
    good = M.point_bytes([pts[2][0]], montgomery)
    big_x, big_y = P.Q.to_bytes(32, "little") + good[32:], good[:32] + P.Q.to_bytes(32, "little")
    off = M.point_bytes([(pts[2][0][0], pts[2][0][1] ^ 1)], montgomery)
    for first, second, want in ((big_x, None, E_SHAPE), (None, big_y, E_SHAPE), (off, None, E_ASSERTION), (None, off, E_ASSERTION),
                                (off, big_x, E_SHAPE), (big_y, off, E_SHAPE)):
        points = points_tensor(pts, montgomery)
        for j, raw in ((0, first), (1, second)):
            if raw is not None:
                points[2, j] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        got = run(H, pkey, points)
        assert got[2] == [0, 0, want, 0, 0, 0, 0, 0] and got[0][2] == 0 and got[1][2] == untouched and rest(got, 2) == rest(clean, 2)


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_outputs_left_out_and_two_calls_on_one_stream(H, montgomery):
    pkey = key(H, montgomery, 2)
    a = logs(WG + 1, 2, accepting=[0, WG])
    points = points_tensor(points_of(a), montgomery)
    want_accept, want_gt = expected(a, 2, 0, montgomery)
    accept, gt, status = run(H, pkey, points, want_gt=False)
    assert accept == want_accept and status == [0] * (WG + 1)
    accept, gt, status = run(H, pkey, points, want_accept=False)
    assert gt == want_gt and status == [0] * (WG + 1)
    # a flagged circuit with no status array: no verdict but 0, nothing else written
    bad = points.clone()
    bad[0, 0, :32] = torch.frombuffer(bytearray(P.Q.to_bytes(32, "little")), dtype=torch.uint8).cuda()
    acc, g = H.prover.pairing_check(pkey, bad, 0, None)
    torch.cuda.synchronize()
    assert acc.cpu().tolist() == [0] + want_accept[1:] and bytes(g[0].cpu().numpy()) == bytes(384) and [bytes(r) for r in g[1:].cpu().numpy()] == want_gt[1:]
    # two calls, no synchronisation in between: other points, other mask, the second reads the first's status
    status = torch.zeros(WG + 1, dtype=torch.uint8, device="cuda")
    first = H.prover.pairing_check(pkey, bad, 0, status)
    second = H.prover.pairing_check(pkey, points, 1, status)
    torch.cuda.synchronize()
    want2_accept, want2_gt = expected(a, 2, 1, montgomery)
    assert status.cpu().tolist() == [E_SHAPE] + [0] * WG
    assert first[0].cpu().tolist() == [0] + want_accept[1:] and [bytes(r) for r in first[1][1:].cpu().numpy()] == want_gt[1:]
    assert second[0].cpu().tolist() == [0] + want2_accept[1:] and [bytes(r) for r in second[1][1:].cpu().numpy()] == want2_gt[1:]
    assert bytes(second[1][0].cpu().numpy()) == bytes(384), "the circuit the first call flagged is skipped by the second"


def test_wrapper_refusals(H):
    pkey = key(H, False, 2)
    from halo2_rsa_amd._lib import H2RError
    points = points_tensor(points_of(logs(2, 2)), False)
    for bad in (points.cpu(), points[:, :1], points.to(torch.int32)):
        with pytest.raises(H2RError):
            H.prover.pairing_check(pkey, bad)
    with pytest.raises(H2RError):
        H.prover.pairing_check(pkey, points, 4)                         # a mask bit at or above the pairs
    with pytest.raises(H2RError):
        H.prover.PairingKey(pkey.chip, [bytes(128)])                     # the identity is no key
    with pytest.raises(H2RError):
        H.prover.PairingKey(pkey.chip, [])
