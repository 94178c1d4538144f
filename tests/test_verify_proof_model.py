"""CPU: the model of the verifier's accumulators (tests/verify_proof_ref.py) against the model verifier of
tests/create_proof_ref.py, on the k = 9 `mul_mod-64x4-bn254` proof of tests/test_create_proof_model.py: [tau] L = R holds exactly when
`verify` accepts, over every case that file builds, and a rejection by status falls where the model returns early."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
import verify_proof_ref as V
from test_create_proof_model import INSTANCES, SEED, TAU, VK, case, flips, sections   # noqa: F401  (case: the module's fixture, one proof here too)
from transcript_ref import E_ASSERTION, E_SHAPE


def agree(key, proof, instances=INSTANCES, tau=TAU):
    """Whether the accumulators accept; asserted equal to the model verifier's answer."""
    status, left, right = V.accumulate(V.VerifyingKey(key, tau), proof, instances)
    ok = status == 0 and V.accepts(left, right, tau)
    assert ok == C.verify(key, proof, tau, instances)
    return ok, status


def test_the_accumulators_accept_the_provers_proof(case):
    _, key, proof = case
    assert agree(key, proof) == (True, 0)
    vk = V.VerifyingKey(key, TAU)
    status, left, right = V.accumulate(vk, proof, INSTANCES)
    assert left != V.M.IDENT and right != V.M.IDENT and V.M.on_curve(left) and V.M.on_curve(right)
    assert not V.accepts(left, right, TAU + 1)
    # the base order and the scalars: as many scalars as bases, G last, W's scalars u^p z_p
    _, sec = V.decode(key.cfg, proof)
    ch = V.challenges(vk, sec, INSTANCES)
    _, scal, lsc = V.scalars_of(key.cfg, sec["evals"], ch)
    assert len(scal) == len(V.bases_of(vk, sec)) == len(V.base_index(key.cfg)) == 32 + key.cfg.num_fixed + key.cfg.m + 1
    assert lsc == [pow(ch[6], p, C.R) for p in range(4)]
    w0 = V.base_index(key.cfg)[("w", 0)]
    assert scal[w0:w0 + 4] == [l * z % C.R for l, z in zip(lsc, C.points_of(key.cfg, ch[4]))]


def test_one_flipped_bit_in_any_section_agrees_with_the_model_verifier(case):
    _, key, proof = case
    for name, byte, bit in flips(key.cfg):
        bad = bytearray(proof)
        bad[byte + bit // 8] ^= 1 << (bit % 8)
        ok, status = agree(key, bytes(bad))
        assert not ok, name
        if status:                                                   # a flipped abscissa may be no point's: the model's early return
            assert status == E_ASSERTION and C.decompress(bytes(bad[byte - byte % 32:byte - byte % 32 + 32])) is None, name
    bad = bytearray(proof)
    bad[31] ^= 0x80                                                  # the sign bit of a point: decodes, then [tau] L != R
    assert agree(key, bytes(bad)) == (False, 0)
    bad = bytearray(proof)
    bad[sections(key.cfg)["evals"][0] + 31] ^= 0x80                   # a scalar >= r
    assert agree(key, bytes(bad)) == (False, E_SHAPE)


def test_statuses_of_the_decoder(case):
    _, key, proof = case
    sec = sections(key.cfg)

    def with_item(off, val):
        return proof[:off] + val.to_bytes(32, "little") + proof[off + 32:]

    no_point = next(x for x in range(2, 100) if C.decompress(x.to_bytes(32, "little")) is None)
    assert agree(key, with_item(sec["evals"][0] + 64, C.R)) == (False, E_SHAPE)
    assert agree(key, with_item(sec["perm_z"][0], C.Q)) == (False, E_SHAPE)
    assert agree(key, with_item(sec["perm_z"][0], C.Q | 1 << 255)) == (False, E_SHAPE)
    assert agree(key, with_item(sec["h"][0], no_point)) == (False, E_ASSERTION)
    both = with_item(sec["advice"][0], no_point)                     # E_SHAPE wins wherever the two occur
    assert agree(key, both[:sec["w"][0]] + C.Q.to_bytes(32, "little") + both[sec["w"][0] + 32:]) == (False, E_SHAPE)
    assert V.decode_item("point", (1).to_bytes(32, "little")) == (0, (1, 2)) and V.decode_item("point", (1 | 1 << 255).to_bytes(32, "little")) == (0, (1, C.Q - 2))


def test_another_vk_repr_or_instance_agrees(case):
    _, key, proof = case
    other = C.Key(key.cfg, key.fixed, key.sigma, key.fixed_rows, key.lcfg, 0, VK + 1)
    assert agree(other, proof) == (False, 0)
    for inst in ([8, C.R - 1], INSTANCES[:1], []):
        assert agree(key, proof, inst) == (False, 0)
    assert agree(key, proof, tau=TAU + 1) == (False, 0)


def test_the_proof_of_an_image_with_one_changed_cell_agrees(case):
    rows, key, _ = case
    row = next(i for i in range(key.cfg.u) if key.fixed[0][i])
    bad = [list(r) for r in rows]
    bad[row][0] = (bad[row][0] + 1) % C.R
    assert agree(key, C.prove(bad, key, SEED, 0, TAU, INSTANCES, strict=False)) == (False, 0)


def test_x_a_root_of_unity_is_an_assertion(case):
    _, key, proof = case
    _, sec = V.decode(key.cfg, proof)
    ch = list(V.challenges(V.VerifyingKey(key, TAU), sec, INSTANCES))
    ch[4] = pow(key.cfg.omega(C.R), 5, C.R)
    assert V.scalars_of(key.cfg, sec["evals"], ch) == (E_ASSERTION, None, None)


def test_combine_folds_a_batch_into_one_pair(case):
    _, key, proof = case
    vk = V.VerifyingKey(key, TAU)
    bad = bytearray(proof)
    bad[sections(key.cfg)["evals"][0] + 5] ^= 1
    acc = [V.accumulate(vk, p, INSTANCES) for p in (proof, bytes(bad), proof)]
    lefts, rights = [a[1] for a in acc], [a[2] for a in acc]
    seed = bytes(range(7, 39))
    assert V.rho(seed, 0) != V.rho(seed, 2)
    good = V.combine([lefts[0], lefts[2]], [rights[0], rights[2]], [0, 0], seed)
    assert V.accepts(*good, TAU)
    assert not V.accepts(*V.combine(lefts, rights, [0, 0, 0], seed), TAU)           # the bad circuit unflagged: the pair rejects
    dropped = V.combine(lefts, rights, [0, E_ASSERTION, 0], seed)                    # flagged and dropped: the rest is accepted
    assert V.accepts(*dropped, TAU) and dropped != good
    assert V.combine(lefts, rights, [1, 1, 1], seed) == (V.M.IDENT, V.M.IDENT)
