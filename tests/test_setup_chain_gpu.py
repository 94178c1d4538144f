"""The four calls of the reference's bench in one chain on the device: prover.setup -> keygen -> create_proof ->
verify, on the k = 9 fixtures of tests/test_create_proof_gpu.py.  The parameters of a known tau give the proofs of the host-built key of
the same tau byte for byte; their own pairing key accepts them; the pairing key of tau + 1 rejects them without a status; downsize is setup
at the smaller size.  One pass runs under torch.cuda.set_sync_debug_mode("error"): setup, create_proof and verify make no host access
(keygen synchronises by design, section 2p, and PairingKey uploads its tables: both are built outside that window)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_create_proof_gpu as CP
import test_prover_chain_model as PM
from test_create_proof_gpu import H   # noqa: F401  (the fixture)

B = CP.B
REPRS, IDS = [False, True], ["canonical", "montgomery"]


def chain(H, montgomery):
    """(host key, image, params, the key keygen makes over params, the copy pairs)"""
    circ, _, kinds, _, _ = CP.model9()
    _, _, pairs, _ = PM.Chain().image(PM.BASE)
    host_key, image = CP.setup9(H, montgomery)
    chip, dom, cfg = host_key.chip, host_key.dom, circ.cfg
    params = H.prover.setup(chip, CP.K9, tau=CP.rep(CP.TAU, montgomery))
    assert params.omega == dom.omega                             # halo2's root of the 2^9 domain on both sides
    host_pairs = np.array(list(pairs), dtype=np.uint32).reshape(-1, 4)
    key = H.prover.keygen(chip, dom, params.g, host_key.la, np.asarray(kinds, dtype=np.uint8), host_pairs, cfg.blinding_factors, column_src=cfg.column_src,
                          chunk_len=cfg.chunk_len, vk_repr=CP.rep(CP.VK, montgomery), lagrange_key=params.g_lagrange)
    return host_key, image, params, key


def verdicts(H, vk, pkey, proofs, inst):
    accept, status = H.prover.verify(vk, pkey, proofs, inst)
    torch.cuda.synchronize()
    return accept.cpu().tolist(), status.cpu().tolist()


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_setup_keygen_create_proof_verify(H, montgomery):
    host_key, image, params, key = chain(H, montgomery)
    chip, inst = host_key.chip, CP.instances_tensor(montgomery)
    torch.cuda.synchronize()
    assert torch.equal(params.g.bases.reshape(-1), host_key.ck.bases.reshape(-1)) and torch.equal(params.g_lagrange.bases.reshape(-1), host_key.lk.bases.reshape(-1))
    want, st0 = H.prover.create_proof(host_key, image, B, seed=CP.SEED, instances=inst)
    proofs, st1 = H.prover.create_proof(key, image, B, seed=CP.SEED, instances=inst)
    torch.cuda.synchronize()
    assert st0.cpu().tolist() == st1.cpu().tolist() == [0] * B and torch.equal(proofs, want)
    assert bytes(proofs[1].cpu().numpy()) == CP.model9()[4][1]
    vk = key.verifying_key()
    assert verdicts(H, vk, params.pairing_key(), proofs, inst) == ([1] * B, [0] * B)
    # the pairing key of another tau: every circuit rejected, by the pairing alone
    other = H.prover.setup(chip, CP.K9, tau=CP.rep(CP.TAU + 1, montgomery))
    assert other.s_g2 != params.s_g2 and other.g2 == params.g2
    assert verdicts(H, vk, other.pairing_key(), proofs, inst) == ([0] * B, [0] * B)
    # downsize: the first 2^8 powers, the Lagrange key of the smaller domain by the curve transform
    small, direct = params.downsize(8), H.prover.setup(chip, 8, tau=CP.rep(CP.TAU, montgomery))
    torch.cuda.synchronize()
    assert (small.k, small.n, small.g.n, small.g_lagrange.n, small.omega) == (8, 256, 256, 256, direct.omega)
    assert torch.equal(small.g.bases.reshape(-1), direct.g.bases.reshape(-1)) and torch.equal(small.g_lagrange.bases.reshape(-1), direct.g_lagrange.bases.reshape(-1))
    assert (small.g2, small.s_g2) == (direct.g2, direct.s_g2) == (params.g2, params.s_g2)


def test_no_host_access(H):
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "the installed torch has no torch.cuda.set_sync_debug_mode"
    host_key, image, params, key = chain(H, True)                # untimed first pass: code objects, allocator
    chip, inst = host_key.chip, CP.instances_tensor(True)
    vk, pkey = key.verifying_key(), params.pairing_key()
    H.prover.verify(vk, pkey, H.prover.create_proof(key, image, B, seed=CP.SEED, instances=inst)[0], inst)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = H.prover.setup(chip, CP.K9, tau=CP.rep(CP.TAU, True))
        proofs, status = H.prover.create_proof(key, image, B, seed=CP.SEED, instances=inst)
        accept, status = H.prover.verify(vk, pkey, proofs, inst)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert accept.cpu().tolist() == [1] * B and status.cpu().tolist() == [0] * B
    assert torch.equal(again.g.bases, params.g.bases) and torch.equal(again.g_lagrange.bases, params.g_lagrange.bases) and again.s_g2 == params.s_g2
