"""halo2 commits its columns in Lagrange form (commit_lagrange over g_lagrange): the key EvaluationDomain.lagrange_key makes on the device
(h2r_curve_ntt) under the columns of a recorded circuit.  The advice columns and the Z columns of the permutation and
lookup arguments of a recorded mul_mod image at k = 10, as tests/prover_chain_ref.py provides them (Lagrange form, random tails behind row
u), satisfy on the device alone, byte for byte,
    lagrange_key(key).commit([f])  ==  key.commit([lagrange_to_coeff(f)])
for a key whose bases are no powers of a tau (the identity is linear algebra).  One changed point of the Lagrange key breaks it."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import curve_ntt_ref as C
import msm_ref as M
import prover_chain_ref as CR
from pyref import FIELD_MODULI
from test_prover_chain_model import BASE, IMAGES, Chain

K = 10
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
        w, L, field, _, _, _, _ = IMAGES[BASE]
        assert field == "bn254_fr"
        rows, kinds, pairs, lcfg = Chain().image(BASE)
        rng = random.Random("commit/lagrange/chain")
        ch = tuple(rng.randrange(1, P) for _ in range(4))
        circ = CR.circuit_from_image(rows, kinds, pairs, w, L, P, lcfg, K, ch, random.Random("commit/lagrange/tails"))
        assert circ.cfg.n == 1 << K
        CACHE["columns"] = circ.lag["advice"] + circ.lag["perm_z"] + [z for z in circ.lag["lookup_z"] if z is not None]
        CACHE["bases"] = M.mul_g_batch([rng.randrange(1, P) for _ in range(1 << K)])
    return CACHE


@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
def test_lagrange_commitments_of_a_recorded_circuit(H, montgomery):
    cs = setup_once()
    cols = cs["columns"]
    assert len(cols) == 5 + 3 + 5 and all(len(c) == 1 << K for c in cols)
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    rep = (lambda v: v * (1 << 256) % P) if montgomery else (lambda v: v)
    dom = H.EvaluationDomain(chip, K, K, rep(C.omega_of(K)), rep(1))
    key = H.CommitKey(chip, torch.frombuffer(bytearray(M.point_bytes(cs["bases"], montgomery)), dtype=torch.uint8).reshape(1 << K, 64).cuda())
    lag = torch.frombuffer(bytearray(b"".join(M.scalar_bytes(c, montgomery) for c in cols)), dtype=torch.uint8).reshape(len(cols), 1 << K, 32).cuda()
    lkey = dom.lagrange_key(key)
    coeff = dom.lagrange_to_coeff(lag)
    a = lkey.commit([lag[c] for c in range(len(cols))])
    b = key.commit([coeff[c] for c in range(len(cols))])
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    host = a.cpu().numpy()
    assert all(host[0, c].any() for c in range(len(cols))) and len({host[0, c].tobytes() for c in range(len(cols))}) == len(cols)
    # the first advice column against the model: [sum_i f_i log(L_i)]G is out of reach (the bases have no known relation), the naive sum is not
    assert host[0, 0].tobytes() == M.point_bytes([M.naive_msm(cs.setdefault("coeff0", C.NR.inverse(cols[0], K, C.omega_of(K), 1, P)), cs["bases"])], montgomery)
    # one changed point of the Lagrange key (its neighbour's copy): every column whose cell there is nonzero commits to something else
    bad = H.CommitKey(chip, lkey.bases.clone())
    row = next(i for i in range(1 << K) if all(c[i] and c[i + 1] for c in cols))
    bad.bases[row] = bad.bases[row + 1]
    c_bad = bad.commit([lag[c] for c in range(len(cols))])
    torch.cuda.synchronize()
    assert all(not torch.equal(c_bad[0, c], b[0, c]) for c in range(len(cols)))
