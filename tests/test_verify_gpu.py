"""prover.verify on the device: verify_proof's accumulators through the pairing check to a verdict per circuit, with
the fixtures of tests/test_verify_proof_gpu.py.  The device is given [tau]G2 only; the expected verdict is the model's V.accepts(L, R, TAU),
which knows tau.  The three k = 9 proofs are accepted; one flipped bit per proof section in circuit 1; combine's fold through pairing_check
at batch 1; no host access; the proofs tiled to 65 circuits with the last two changed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pairing_ref as P
import test_create_proof_gpu as CP
import test_verify_proof_gpu as VP
import verify_proof_ref as V
from test_create_proof_gpu import H, TAU   # noqa: F401  (H: the fixture)
from test_create_proof_model import flips, sections

B = CP.B
REPRS, IDS = [False, True], ["canonical", "montgomery"]
CACHE = {}


def pairing_key(H, vk, montgomery):
    """the KZG key: [tau]G2 and G2 -- all the device learns of tau"""
    if "tau_g2" not in CACHE:
        CACHE["tau_g2"] = P.g2_mul(TAU, P.G2)
    return H.prover.PairingKey(vk.chip, [P.g2_bytes(CACHE["tau_g2"], montgomery), P.g2_bytes(P.G2, montgomery)])


def verdicts(H, vk, pkey, proofs, inst):
    accept, status = H.prover.verify(vk, pkey, proofs, inst)
    torch.cuda.synchronize()
    return accept.cpu().tolist(), status.cpu().tolist()


def model_verdict(proof, e):
    st, L, Rp = VP.model(proof, e)
    return (0 if st else int(V.accepts(L, Rp, TAU))), st


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_the_three_proofs_and_one_flipped_bit_per_section(H, montgomery):
    vk, proofs, inst = VP.setup(H, montgomery)
    pkey = pairing_key(H, vk, montgomery)
    assert verdicts(H, vk, pkey, proofs, inst) == ([1] * B, [0] * B)
    # outputs of the caller's, a status on entry
    accept = torch.full((B,), 0xAB, dtype=torch.uint8, device="cuda")
    status = torch.tensor([0, 5, 0], dtype=torch.uint8, device="cuda")
    out = H.prover.verify(vk, pkey, proofs, inst, out=(accept, status))
    torch.cuda.synchronize()
    assert out[0] is accept and out[1] is status and accept.cpu().tolist() == [1, 0, 1] and status.cpu().tolist() == [0, 5, 0]
    # other instances on circuit 0: a rejection without a status
    other = inst.clone()
    other[0] = inst[1]
    assert verdicts(H, vk, pkey, proofs, other) == ([0, 1, 1], [0] * B)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    seen = set()
    for name, byte, bit in flips(CP.model9()[0].cfg):
        bad = bytearray(host[1])
        bad[byte + bit // 8] ^= 1 << (bit % 8)
        accept, status = verdicts(H, vk, pkey, VP.with_bytes(proofs, 1, 0, bytes(bad)), inst)
        want, want_st = model_verdict(bytes(bad), 1)
        assert (accept[0], accept[2], status[0], status[2]) == (1, 1, 0, 0), "%s: circuit 0 or 2 changed" % name
        assert (accept[1], status[1]) == (want, want_st), name
        assert accept[1] == 0, "%s is accepted" % name
        seen.add(status[1])
    assert 0 in seen                                             # some flips decode: rejected by the pairing alone


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_combines_fold_through_the_pairing_check(H, montgomery):
    vk, proofs, inst = VP.setup(H, montgomery)
    pkey = pairing_key(H, vk, montgomery)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    off = sections(CP.model9()[0].cfg)["evals"][0] + 5
    bad = bytearray(host[1])
    bad[off] ^= 1

    def fold(p):
        left, right, status = H.prover.verify_proof(vk, p, inst)
        Ls, Rs = H.prover.combine(left, right, status, VP.COMBINE_SEED, vk.chip)
        accept, gt = H.prover.pairing_check(pkey, torch.stack((Ls, Rs))[None], 0b10)
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * B
        assert (bytes(gt[0].cpu().numpy()) == P.fq12_bytes(P.ONE, montgomery)) == bool(accept.cpu().tolist()[0])
        return accept.cpu().tolist()

    assert fold(proofs) == [1]                                   # the clean batch
    assert fold(VP.with_bytes(proofs, 1, 0, bytes(bad))) == [0]  # one bad circuit of status 0


def test_no_host_access(H):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("the installed torch has no torch.cuda.set_sync_debug_mode")
    vk, proofs, inst = VP.setup(H, True)
    pkey = pairing_key(H, vk, True)
    assert verdicts(H, vk, pkey, proofs, inst) == ([1] * B, [0] * B)   # untimed first call: code objects, allocator
    torch.cuda.set_sync_debug_mode("error")
    try:
        accept, status = H.prover.verify(vk, pkey, proofs, inst)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert accept.cpu().tolist() == [1] * B and status.cpu().tolist() == [0] * B


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_a_batch_across_workgroup_boundaries(H, montgomery):
    """The three proofs tiled to 65 circuits (verify_proof's workgroups hold 64, the pairing's 8), one evaluation bit flipped in the last two."""
    vk, proofs, inst = VP.setup(H, montgomery)
    pkey = pairing_key(H, vk, montgomery)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    batch = 65
    off = sections(CP.model9()[0].cfg)["evals"][0] + 5
    tiled, tiled_inst = proofs.repeat(22, 1)[:batch].contiguous(), inst.repeat(22, 1, 1)[:batch].contiguous()
    want = []
    for e in range(batch):
        raw = bytearray(host[e % B])
        if e in (63, 64):
            raw[off] ^= 1
            tiled = VP.with_bytes(tiled, e, 0, bytes(raw))
        want.append(model_verdict(bytes(raw), e % B)[0])
    assert want == [1] * 63 + [0, 0]
    assert verdicts(H, vk, pkey, tiled, tiled_inst) == (want, [0] * batch)
