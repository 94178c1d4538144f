"""prover.verify_proof and prover.combine on the device against the plain model of tests/verify_proof_ref.py.
The k = 9 `mul_mod-64x4-bn254` image of tests/test_create_proof_gpu.py as three circuits, a key over [tau^i]G, proofs from create_proof, both
representations: the accumulators of the accepting batch are byte-equal to the model's on those bytes and satisfy [tau] L = R; one flipped
bit per proof section in circuit 1 leaves circuits 0 and 2 as they were and makes circuit 1 what the model says (a status, or [tau] L != R);
a scalar = r, an abscissa = q, an abscissa of no point; a status set on entry; combine, also over 4,097 synthetic accumulators (two chunks
and the sum of the chunks' sums); the three proofs tiled to 65 circuits, a batch across a workgroup of 64, with circuits 63 and 64 changed;
no host access; and the k = 10 recorded circuits of tests/test_prover_chain_gpu.py with one changed image cell, judged where the proofs
lie.  The model's answers are made once per proof."""
import os
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
import test_create_proof_gpu as CP
import test_prover_chain_gpu as G
import verify_proof_ref as V
from test_create_proof_gpu import H, INSTANCES, SEED, TAU, VK   # noqa: F401  (H: the fixture)
from test_create_proof_model import flips, sections
from transcript_ref import E_ASSERTION, E_SHAPE, Q, R

B = CP.B
REPRS, IDS = [False, True], ["canonical", "montgomery"]
SENTINEL = 0xAB
COMBINE_SEED = bytes(range(60, 92))
A0, D = 0x2468ace013579bdf0f1e2d3c4b5a6978, 0x13579bdf2468ace08796a5b4c3d2e1f0     # the structured accumulators P_i = [A0 + i D]G
CHUNK = 4096                                                                     # combine sums a batch in chunks of H2R_VERIFY_MAX_TERMS
CACHE = {}


def setup(H, montgomery):
    """(verifying key, the device's proofs [3, 2944], the instances) of the k = 9 circuit; the proofs are create_proof's."""
    key, image = CP.setup9(H, montgomery)
    inst = CP.instances_tensor(montgomery)
    proofs, status = H.prover.create_proof(key, image, B, seed=SEED, instances=inst)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * B
    vk = key.verifying_key()
    assert vk.proof_bytes == key.proof_bytes and vk.num_evals == key.num_evals and vk.eval_plan == key.eval_plan and vk.open_plan == key.open_plan
    return vk, proofs, inst


def model_vk():
    if "vk" not in CACHE:
        CACHE["vk"] = V.VerifyingKey(CP.model9()[3], TAU)
    return CACHE["vk"]


def model(proof, e):
    """(status, L, R) of the model on one proof's bytes with the instances of the key's circuit e, made once per (bytes, e)."""
    if (proof, e) not in CACHE:
        CACHE[(proof, e)] = V.accumulate(model_vk(), proof, INSTANCES[e])
    return CACHE[(proof, e)]


def run(H, vk, proofs, inst, status_in=None):
    """verify_proof into sentinel-filled outputs -> (left bytes [B][64], right bytes, status list)."""
    batch = int(proofs.shape[0])
    left, right = (torch.full((batch, 64), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2))
    status = torch.tensor(status_in or [0] * batch, dtype=torch.uint8, device="cuda")
    out = H.prover.verify_proof(vk, proofs, inst, out=(left, right, status))
    torch.cuda.synchronize()
    assert out[0] is left and out[1] is right and out[2] is status
    return [bytes(r) for r in left.cpu().numpy()], [bytes(r) for r in right.cpu().numpy()], status.cpu().tolist()


def same_as_model(got, e, proof, montgomery, instances_of=None):
    """Circuit e's (left, right, status) against the model: byte-equal accumulators, or the model's status and untouched outputs.  Returns
    whether the circuit is accepted.  instances_of: the key's circuit whose instances e carries (e itself where the batch is the key's)."""
    left, right, status = got
    st, L, Rp = model(proof, e if instances_of is None else instances_of)
    assert status[e] == st, (e, status[e], st)
    if st:
        assert left[e] == right[e] == bytes([SENTINEL]) * 64, "a flagged circuit's accumulators stay as they were"
        return False
    assert left[e] == M.point_bytes([L], montgomery) and right[e] == M.point_bytes([Rp], montgomery), e
    return V.accepts(L, Rp, TAU)


def with_bytes(proofs, e, off, raw):
    t = proofs.clone()
    t[e, off:off + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    return t


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_the_accepting_batch(H, montgomery):
    vk, proofs, inst = setup(H, montgomery)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    assert host == CP.model9()[4], "create_proof's bytes are the model prover's"
    got = run(H, vk, proofs, inst)
    assert got[2] == [0] * B
    for e in range(B):
        assert same_as_model(got, e, host[e], montgomery), "circuit %d is not accepted" % e
        Lp, Rp = M.points_from_bytes(got[0][e], montgomery)[0], M.points_from_bytes(got[1][e], montgomery)[0]
        assert M.mul(TAU, Lp) == Rp and Lp != M.IDENT and not V.accepts(Lp, Rp, TAU + 1)
    # other instances on circuit 0: the same bytes, another transcript, a rejection without a status
    other = inst.clone()
    other[0] = inst[1]
    left, right, status = run(H, vk, proofs, other)
    assert status == [0] * B and (left[1:], right[1:]) == (got[0][1:], got[1][1:])
    assert not V.accepts(M.points_from_bytes(left[0], montgomery)[0], M.points_from_bytes(right[0], montgomery)[0], TAU)


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_one_flipped_bit_per_section_in_circuit_1(H, montgomery):
    vk, proofs, inst = setup(H, montgomery)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    good = run(H, vk, proofs, inst)
    cfg = CP.model9()[0].cfg
    wanted = ("advice", "A'", "permutation Z", "lookup Z", "random polynomial", "h piece", "evaluation advice 4 at point 1", "evaluation fixed 5 at point 0", "W 1")
    chosen = [f for f in flips(cfg) if f[0] in wanted]
    assert len(chosen) == len(wanted)
    outcomes = set()
    for name, byte, bit in chosen:
        bad = bytearray(host[1])
        bad[byte + bit // 8] ^= 1 << (bit % 8)
        got = run(H, vk, with_bytes(proofs, 1, 0, bytes(bad)), inst)
        for e in (0, 2):
            assert (got[0][e], got[1][e], got[2][e]) == (good[0][e], good[1][e], 0), "%s: circuit %d changed" % (name, e)
        assert not same_as_model(got, 1, bytes(bad), montgomery), "%s is accepted" % name
        outcomes.add(got[2][1])
    assert 0 in outcomes                                         # (at least the evaluations and the sign-preserving flips decode)


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_other_rejections_and_a_status_on_entry(H, montgomery):
    vk, proofs, inst = setup(H, montgomery)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    good = run(H, vk, proofs, inst)
    sec = sections(CP.model9()[0].cfg)
    no_point = next(x for x in range(2, 100) if C.decompress(x.to_bytes(32, "little")) is None)
    for off, val, want in ((sec["evals"][0] + 32 * 7, R, E_SHAPE), (sec["perm_z"][0] + 32, Q, E_SHAPE), (sec["h"][0], no_point | 1 << 255, E_ASSERTION),
                           (sec["w"][0] + 96, no_point, E_ASSERTION)):
        raw = val.to_bytes(32, "little")
        got = run(H, vk, with_bytes(proofs, 1, off, raw), inst)
        assert got[2] == [0, want, 0]
        assert not same_as_model(got, 1, host[1][:off] + raw + host[1][off + 32:], montgomery)
        assert (got[0][0], got[0][2], got[1][0], got[1][2]) == (good[0][0], good[0][2], good[1][0], good[1][2])
    # both in one proof: H2R_E_SHAPE wins
    both = with_bytes(with_bytes(proofs, 1, sec["advice"][0], no_point.to_bytes(32, "little")), 1, sec["w"][0], Q.to_bytes(32, "little"))
    assert run(H, vk, both, inst)[2] == [0, E_SHAPE, 0]
    # a status that is set on entry: the circuit is skipped, its outputs keep their sentinel bytes, the byte is not cleared
    got = run(H, vk, proofs, inst, status_in=[0, 0, 5])
    assert got[2] == [0, 0, 5] and got[0][2] == got[1][2] == bytes([SENTINEL]) * 64
    assert (got[0][:2], got[1][:2]) == (good[0][:2], good[1][:2])


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_combine(H, montgomery):
    vk, proofs, inst = setup(H, montgomery)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    off = sections(CP.model9()[0].cfg)["evals"][0] + 5
    bad = bytearray(host[1])
    bad[off] ^= 1
    mixed = with_bytes(proofs, 1, 0, bytes(bad))

    def fold(p, flag=None):
        left, right, status = H.prover.verify_proof(vk, p, inst)
        if flag is not None:
            status[flag] = E_ASSERTION
        Ls, Rs = H.prover.combine(left, right, status, COMBINE_SEED, vk.chip)
        torch.cuda.synchronize()
        st = status.cpu().tolist()
        lefts = [M.IDENT if s else M.points_from_bytes(bytes(r), montgomery)[0] for r, s in zip(left.cpu().numpy(), st)]
        rights = [M.IDENT if s else M.points_from_bytes(bytes(r), montgomery)[0] for r, s in zip(right.cpu().numpy(), st)]
        want = V.combine(lefts, rights, st, COMBINE_SEED)
        got = M.points_from_bytes(bytes(Ls.cpu().numpy()), montgomery)[0], M.points_from_bytes(bytes(Rs.cpu().numpy()), montgomery)[0]
        assert got == want and bytes(Ls.cpu().numpy()) == M.point_bytes([want[0]], montgomery)
        return V.accepts(*got, TAU)

    assert fold(proofs)                                          # three good circuits: accepted together
    assert not fold(mixed)                                       # the bad circuit unflagged: the one pair rejects
    assert fold(mixed, flag=1)                                   # flagged and dropped: the rest is accepted
    # two chunks, 4,096 circuits and 1, and the sum of the two sums; then the second chunk's only circuit unflagged, so that its rho and its
    # points count
    fold_of_structured_points(H, vk.chip, montgomery, CHUNK + 1, (1234, CHUNK))
    fold_of_structured_points(H, vk.chip, montgomery, CHUNK + 1, (CHUNK - 1,))


def fold_of_structured_points(H, chip, montgomery, batch, flagged):
    """combine on synthetic accumulators with known logarithms, left[e] = P_e and right[e] = P_(batch + e): the fold is ONE scalar
    multiplication, L* = [sum rho_e log_e]G.  A flagged circuit's rows hold sentinel bytes, which are no point: they must not count."""
    if "structured" not in CACHE:
        CACHE["structured"] = M.structured_bases(2 * (CHUNK + 1), A0, D)
    pts = CACHE["structured"]
    assert 2 * batch <= len(pts) and batch > CHUNK and all(e < batch for e in flagged)
    assert {e // CHUNK for e in flagged} == set(range((batch + CHUNK - 1) // CHUNK)) or len(flagged) == 1
    sides = []
    for first in (0, batch):
        raw = bytearray(M.point_bytes(pts[first:first + batch], montgomery))
        for e in flagged:
            raw[64 * e:64 * e + 64] = bytes([SENTINEL]) * 64
        sides.append(torch.frombuffer(raw, dtype=torch.uint8).reshape(batch, 64).cuda())
    st = [E_ASSERTION if e in flagged else 0 for e in range(batch)]
    status = torch.tensor(st, dtype=torch.uint8, device="cuda")
    before = [t.clone() for t in sides]
    Ls, Rs = H.prover.combine(sides[0], sides[1], status, COMBINE_SEED, chip)
    torch.cuda.synchronize()
    rhos = [0 if s else V.rho(COMBINE_SEED, e) for e, s in enumerate(st)]
    assert len(set(rhos)) == batch - len(flagged) + 1
    for got, first, name in ((Ls, 0, "L*"), (Rs, batch, "R*")):
        want = M.mul_g(sum(rho * (A0 + (first + e) * D) for e, rho in enumerate(rhos)) % R)
        assert bytes(got.cpu().numpy()) == M.point_bytes([want], montgomery), "%s of %d circuits, flagged %r" % (name, batch, flagged)
    assert all(torch.equal(a, b) for a, b in zip(sides, before)) and status.cpu().tolist() == st, "combine writes none of its operands"


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_a_batch_across_a_workgroup_boundary(H, montgomery):
    """The three proofs tiled to 65 circuits -- circuit e holds proof e mod 3 under the instances of e mod 3 --, one evaluation bit flipped in
    circuits 63 (the first workgroup's last lane) and 64 (the second workgroup's only one)."""
    vk, proofs, inst = setup(H, montgomery)
    host = [bytes(p) for p in proofs.cpu().numpy()]
    batch = 65
    off = sections(CP.model9()[0].cfg)["evals"][0] + 5
    tiled, tiled_inst = proofs.repeat(22, 1)[:batch].contiguous(), inst.repeat(22, 1, 1)[:batch].contiguous()
    want = [host[e % B] for e in range(batch)]
    for e in (63, 64):
        bad = bytearray(want[e])
        bad[off] ^= 1
        want[e] = bytes(bad)
        tiled = with_bytes(tiled, e, 0, want[e])
    got = run(H, vk, tiled, tiled_inst)
    assert [bytes(p) for p in tiled.cpu().numpy()] == want
    for e in range(batch):
        accepted = same_as_model(got, e, want[e], montgomery, instances_of=e % B)
        assert accepted == (e not in (63, 64)), "circuit %d is %s" % (e, "accepted" if accepted else "rejected")
    assert got[2] == [0] * batch, "a flipped evaluation bit is a rejection without a status"


def test_no_host_access(H):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("the installed torch has no torch.cuda.set_sync_debug_mode")
    vk, proofs, inst = setup(H, True)
    want = run(H, vk, proofs, inst)                              # untimed first call: code objects, allocator
    torch.cuda.set_sync_debug_mode("error")
    try:
        left, right, status = H.prover.verify_proof(vk, proofs, inst)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * B and [bytes(r) for r in left.cpu().numpy()] == want[0] and [bytes(r) for r in right.cpu().numpy()] == want[1]


def test_recorded_circuits_with_one_changed_cell(H):
    from halo2_rsa_amd import _lib
    c = G.Chain(H, "bn254_fr")
    assert G.B == B
    key = CP.device_key(H, c.chip, c.la, c.cfg, c.fixed, c.sigma, c.kinds)
    vk = key.verifying_key()
    inst = CP.instances_tensor(False)
    row, col = next((r, q) for (r, q, _, _) in c.inside if c.kinds[r] == AR.ROW_MUL_ADD)
    image = c.emit()
    c.cell(image, 1, row, col)[0] ^= 1
    proofs, status = H.prover.create_proof(key, image, B, seed=SEED, instances=inst)
    left, right, vstatus = H.prover.verify_proof(vk, proofs, inst)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, _lib.H2R_E_ASSERTION, 0]
    vst = vstatus.cpu().tolist()
    accepted = []
    for e in range(B):
        Lp, Rp = M.points_from_bytes(bytes(left[e].cpu().numpy()), False)[0], M.points_from_bytes(bytes(right[e].cpu().numpy()), False)[0]
        accepted.append(vst[e] == 0 and Lp != M.IDENT and V.accepts(Lp, Rp, TAU))
    assert accepted == [True, False, True]
