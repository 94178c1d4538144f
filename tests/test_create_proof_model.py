"""CPU: the model prover and the model verifier of tests/create_proof_ref.py fit each other on the k = 9 `mul_mod-64x4-bn254` image of
tests/test_prover_chain_model.py: the verifier accepts the prover's proof, and rejects it after one flipped bit in
every section, under another vk_repr, another instance value, and for an image with one changed cell.  One proof per module."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
from test_prover_chain_model import BASE, Chain

SEED, VK, INSTANCES = bytes(range(100, 132)), 0x1234567, [7, C.R - 1]
TAU = random.Random("create_proof/model/tau").randrange(2, C.R)


@pytest.fixture(scope="module")
def case():
    chain = Chain()
    circ = chain.circuit(BASE)
    rows, _, _, lcfg = chain.image(BASE)
    key = C.Key(circ.cfg, circ.lag["fixed"], circ.lag["sigma"], circ.fixed_rows, lcfg, 0, VK)
    return rows, key, C.prove(rows, key, SEED, 0, TAU, INSTANCES)


def sections(cfg):
    """name -> (first byte, count) of every section of the proof."""
    out, off = {}, 0
    for name, _, count in C.proof_layout(cfg):
        out[name] = (off, count)
        off += 32 * count
    return out


def test_the_verifier_accepts_the_provers_proof(case):
    rows, key, proof = case
    assert len(proof) == 32 * (5 + 10 + 3 + 5 + 1 + 4 + 60 + 4)
    assert C.verify(key, proof, TAU, INSTANCES)
    assert C.prove(rows, key, SEED, 0, TAU, INSTANCES) == proof                       # reproducible from the seed
    assert not C.verify(key, proof, TAU + 1, INSTANCES) and not C.verify(key, proof[:-32], TAU, INSTANCES)


def flips(cfg):
    sec = sections(cfg)
    q = C.queries(C.eval_plan(cfg))
    out = [("advice", sec["advice"][0] + 32 * 2, 3), ("A'", sec["lookup_perm"][0] + 32 * 4, 0), ("permutation Z", sec["perm_z"][0] + 32, 5),
           ("lookup Z", sec["lookup_z"][0] + 32 * 3, 1), ("random polynomial", sec["random"][0], 2), ("h piece", sec["h"][0] + 32 * 3, 4)]
    for probe in (("advice", 0, 0), ("advice", 4, 1), ("fixed", 5, 0), ("random", 0, 0), ("sigma", 2, 0), ("perm_z", 0, 2), ("perm_z", 2, 1), ("lookup_z", 1, 1),
                  ("lookup_a_perm", 3, 3), ("lookup_s_perm", 4, 0)):
        out.append(("evaluation %s %d at point %d" % probe, sec["evals"][0] + 32 * q.index(probe), 9))
    return out + [("W %d" % p, sec["w"][0] + 32 * p, 6) for p in range(4)]


def test_one_flipped_bit_in_any_section_is_rejected(case):
    _, key, proof = case
    for name, byte, bit in flips(key.cfg):
        bad = bytearray(proof)
        bad[byte + bit // 8] ^= 1 << (bit % 8)
        assert not C.verify(key, bytes(bad), TAU, INSTANCES), name
    for byte in (31, sections(key.cfg)["evals"][0] + 31):                              # the sign bit of a point; a scalar >= r
        bad = bytearray(proof)
        bad[byte] ^= 0x80
        assert not C.verify(key, bytes(bad), TAU, INSTANCES), byte


def test_another_vk_repr_or_instance_is_rejected(case):
    _, key, proof = case
    other = C.Key(key.cfg, key.fixed, key.sigma, key.fixed_rows, key.lcfg, 0, VK + 1)
    assert not C.verify(other, proof, TAU, INSTANCES)
    assert not C.verify(key, proof, TAU, [8, C.R - 1]) and not C.verify(key, proof, TAU, INSTANCES[:1]) and not C.verify(key, proof, TAU, [])


def test_the_proof_of_an_image_with_one_changed_cell_is_rejected(case):
    rows, key, _ = case
    row = next(i for i in range(key.cfg.u) if key.fixed[0][i])                          # a row whose sa is nonzero: cell a counts
    bad = [list(r) for r in rows]
    bad[row][0] = (bad[row][0] + 1) % C.R
    proof = C.prove(bad, key, SEED, 0, TAU, INSTANCES, strict=False)
    assert not C.verify(key, proof, TAU, INSTANCES)
