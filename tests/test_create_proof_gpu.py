"""prover.create_proof on the device against the plain models of tests/create_proof_ref.py.
Byte equality: the k = 9 `mul_mod-64x4-bn254` image of tests/test_prover_chain_model.py uploaded as three circuits, a key over [tau^i]G, a
fixed seed -- every circuit's proof bytes equal the model prover's, in both representations and whatever `group` is: any disagreement in
the order of the rounds, the tags, the tails or the framing fails it.  Recorded circuits: the k = 10 circuits of
tests/test_prover_chain_gpu.py's Chain with the image emit_modpow_advice writes, row-major and planar -- the model VERIFIER accepts all
three proofs, and with one image cell changed on circuit 1 the status is [0, H2R_E_ASSERTION, 0] and it accepts circuits 0 and 2 only.
No host access: create_proof under torch.cuda.set_sync_debug_mode("error").  The model's proofs are made once per module."""
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
import create_proof_ref as C
import msm_ref as M
import test_prover_chain_gpu as G
import test_prover_chain_model as PM
from test_lookup_product import bytes_of
from test_mockprover_ref import _mul_mod

P, B, K9 = C.R, 3, 9
SEED, VK = bytes(range(200, 232)), 0xC0FFEE
INSTANCES = [[5, 6], [7, 8], [C.R - 1, 0]]
TAU = random.Random("create_proof/gpu/tau").randrange(2, P)
CACHE = {}
REPRS, IDS = [False, True], ["canonical", "montgomery"]


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def rep(v, montgomery):
    return v * (1 << 256) % P if montgomery else v


def columns_tensor(cols, montgomery):
    return torch.from_numpy(np.stack([bytes_of(c, P, montgomery) for c in cols])).cuda()


def bases(n):
    if n not in CACHE:
        CACHE[n] = M.mul_g_batch([pow(TAU, i, P) for i in range(n)])
    return CACHE[n]


def commit_key(H, chip, n):
    return H.CommitKey(chip, torch.frombuffer(bytearray(M.point_bytes(bases(n), chip.montgomery)), dtype=torch.uint8).reshape(n, 64).cuda())


def instances_tensor(montgomery):
    raw = b"".join(rep(v, montgomery).to_bytes(32, "little") for row in INSTANCES for v in row)
    return torch.frombuffer(bytearray(raw), dtype=torch.int64).reshape(B, 2, 4).cuda()


def model9():
    """The k = 9 circuit, its model key and the model's three proofs (circuit e draws with index e), made once."""
    if "model9" not in CACHE:
        chain = PM.Chain()
        circ = chain.circuit(PM.BASE)
        rows, kinds, _, lcfg = chain.image(PM.BASE)
        key = C.Key(circ.cfg, circ.lag["fixed"], circ.lag["sigma"], circ.fixed_rows, lcfg, 0, VK)
        proofs = [C.prove(rows, key, SEED, e, TAU, INSTANCES[e]) for e in range(B)]
        assert len(set(proofs)) == B and all(C.verify(key, proofs[e], TAU, INSTANCES[e]) for e in (0, 2))
        CACHE["model9"] = (circ, rows, kinds, key, proofs)
    return CACHE["model9"]


def device_key(H, chip, la, cfg, fixed, sigma, kinds, first_row=0):
    m = chip.montgomery
    dom = H.EvaluationDomain(chip, cfg.k, cfg.log_ext, rep(cfg.omega_ext, m), rep(cfg.zeta, m))
    return H.prover.ProvingKey(chip, dom, commit_key(H, chip, cfg.n), la, columns_tensor(fixed, m), columns_tensor(sigma, m), kinds, cfg.blinding_factors,
                               rep(cfg.delta, m), cfg.gate_fixed, cfg.column_src, cfg.chunk_len, cfg.lookup_advice, cfg.lookup_tag, cfg.lookup_enable,
                               cfg.table_tag, cfg.table_value, rep(VK, m), first_row=first_row)


def setup9(H, montgomery):
    circ, rows, kinds, _, _ = model9()
    chip = H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)
    key = device_key(H, chip, H.LookupArgument(chip, rsa_chip=False), circ.cfg, circ.lag["fixed"], circ.lag["sigma"], np.asarray(kinds, dtype=np.uint8))
    _, _, _, _, im = _mul_mod(64, 4, "bn254_fr", 1000 * 64 + 4)
    assert im.rows == rows
    one = AR.image_to_repr(AR.image_bytes(im), len(rows), P, montgomery=montgomery)
    image = torch.from_numpy(np.stack([one] * B)).cuda()
    assert key.proof_bytes == len(model9()[4][0]) == 2944 and key.rows == len(rows) and tuple(image.shape) == (B, len(rows) * 160)
    return key, image


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_the_proof_bytes_are_the_model_provers(H, montgomery):
    key, image = setup9(H, montgomery)
    proof, status = H.prover.create_proof(key, image, B, seed=SEED, instances=instances_tensor(montgomery))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * B
    got = proof.cpu().numpy()
    sec, off = [], 0
    for name, _, count in C.proof_layout(model9()[0].cfg):
        sec.append((name, off, off + 32 * count))
        off += 32 * count
    for e in range(B):
        want = model9()[4][e]
        for name, a, b in sec:
            assert bytes(got[e, a:b]) == want[a:b], "circuit %d: section %s differs" % (e, name)
        assert bytes(got[e]) == want


def test_grouping_does_not_change_the_proofs(H):
    key, image = setup9(H, False)
    inst = instances_tensor(False)
    whole, st3 = H.prover.create_proof(key, image, B, seed=SEED, instances=inst, group=3)
    single, st1 = H.prover.create_proof(key, image, B, seed=SEED, instances=inst, group=1)
    pair, st2 = H.prover.create_proof(key, image, B, seed=SEED, instances=inst, group=2)
    torch.cuda.synchronize()
    assert torch.equal(whole, single) and torch.equal(whole, pair) and st1.cpu().tolist() == st2.cpu().tolist() == st3.cpu().tolist() == [0] * B
    assert bytes(whole[1].cpu().numpy()) == model9()[4][1]
    other, _ = H.prover.create_proof(key, image, B, seed=bytes(32), instances=inst)
    assert not torch.equal(other, whole) and torch.equal(other[:, :0], whole[:, :0])


def test_no_host_access(H):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("the installed torch has no torch.cuda.set_sync_debug_mode")
    key, image = setup9(H, True)
    inst = instances_tensor(True)
    H.prover.create_proof(key, image, B, seed=SEED, instances=inst)               # untimed first call: code objects, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        proof, status = H.prover.create_proof(key, image, B, seed=SEED, instances=inst, group=2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * B and bytes(proof[2].cpu().numpy()) == model9()[4][2]


@pytest.mark.parametrize("planar", [False, True], ids=["row-major", "planar"])
def test_recorded_circuits_verify(H, planar):
    from halo2_rsa_amd import _lib
    c = G.Chain(H, "bn254_fr", montgomery=planar, planar=planar)
    assert G.B == B
    key = device_key(H, c.chip, c.la, c.cfg, c.fixed, c.sigma, c.kinds)
    vk = C.Key(c.cfg, c.fixed, c.sigma, None, c.lcfg, 0, VK)
    inst = instances_tensor(planar)
    proof, status = H.prover.create_proof(key, c.emit(), B, seed=SEED, instances=inst)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * B
    got = proof.cpu().numpy()
    for e in range(B):
        assert C.verify(vk, bytes(got[e]), TAU, INSTANCES[e]), "circuit %d" % e
    assert not C.verify(vk, bytes(got[0]), TAU, INSTANCES[1])
    if planar:
        return
    # one image cell that a copy pair names, changed on circuit 1 before anything reads it: the permutation product tells
    row, col = next((r, q) for (r, q, _, _) in c.inside if c.kinds[r] == AR.ROW_MUL_ADD)
    image = c.emit()
    c.cell(image, 1, row, col)[0] ^= 1
    proof, status = H.prover.create_proof(key, image, B, seed=SEED, instances=inst)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, _lib.H2R_E_ASSERTION, 0]
    got = proof.cpu().numpy()
    assert [C.verify(vk, bytes(got[e]), TAU, INSTANCES[e]) for e in range(B)] == [True, False, True]
