"""Key generation on the device against the plain models, byte for byte, on bn254_fr and pasta_fq in both
representations, every output in a sentinel-guarded buffer.
sigma: h2r_keygen_sigma_columns against permutation_ref.sigma_from_pairs on the smallest shapes at which it can go wrong (k = 4 .. 11, m in
1, 2, 5, 8; stars, reverse stars, paths across wavefront / workgroup / sort-tile boundaries, whole columns, one class of every cell), the
status cases, and one pair list in two orders.  Fixed columns: h2r_keygen_fixed_columns against prover_chain_ref.fixed_columns on the
recorded k = 10 circuit, on every kind that has a fixed row, and on the RSA table.  End to end: prover.keygen's key is the host-built key
(columns, proof bytes), its derived vk_repr is the model's (tests/keygen_ref.py), its proofs verify, and a key with one copy pair less is
another key.  One case at the reference's size (k = 17, one RSA-2048 modpow_public_key element): the permutation product closes under the
device-built sigma, and sigma differs from the labels exactly on the cells the pairs name."""
import ctypes
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
import keygen_ref as KR
import mockprover_ref as MP
import permutation_ref as PR
import prover_chain_ref as CR
import test_create_proof_gpu as CP
import test_prover_chain_gpu as G
import test_prover_chain_model as PM
import test_verify_gpu as VG
from pyref import FIELD_MODULI
from test_create_proof_gpu import H   # noqa: F401  (the fixture)
from test_lookup_product import bytes_of
from transcript_ref import Q

FIELDS, REPRS = G.FIELDS, [False, True]
COMBOS = [(f, m) for f in FIELDS for m in REPRS]
COMBO_IDS = ["%s-%s" % (f, "montgomery" if m else "canonical") for f, m in COMBOS]
BF, SENTINEL, GUARD = 5, 0xAB, 3
SRC_A, SRC_B, SRC_N = PR.H2R_COPY_SRC
E_SHAPE, E_ASSERTION = 1, 9
W, L = 64, 4
CACHE = {}


def chip_of(H, field, montgomery):
    key = ("chip", field, montgomery)
    if key not in CACHE:
        CACHE[key] = H.BigIntChip(W, W * L, field=field, montgomery=montgomery)
    return CACHE[key]


def rep(v, P, montgomery):
    return v * (1 << 256) % P if montgomery else v


def guarded(columns, rows):
    """(full, view): a sentinel-filled [columns, rows + GUARD, 32] and the view of its first `rows` rows that a kernel is given."""
    full = torch.full((columns, rows + GUARD, 32), SENTINEL, dtype=torch.uint8, device="cuda")
    return full, full[:, :rows]


def intact(full, rows):
    return bool((full[:, rows:] == SENTINEL).all())


def columns_bytes(cols, P, montgomery):
    return np.stack([bytes_of(c, P, montgomery) for c in cols])


def usable(k):
    return (1 << k) - BF - 1


def device_sigma(H, field, montgomery, k, column_src, pairs, first_row=0):
    """(sigma bytes [m, n, 32], status, info) of the device, its guard rows checked."""
    P, chip = FIELD_MODULI[field], chip_of(H, field, montgomery)
    omega, delta = PR.domain(P, k)
    full, view = guarded(len(column_src), 1 << k)
    status = torch.zeros(1, dtype=torch.uint8, device="cuda")
    host = np.array(pairs, dtype=np.uint32).reshape(-1, 4)
    sigma, st, info = H.prover.keygen_sigma_columns(chip, host, k, BF, rep(delta, P, montgomery), rep(omega, P, montgomery), column_src, first_row=first_row,
                                                    out=(view, status))
    torch.cuda.synchronize()
    assert sigma is view and st is status and intact(full, 1 << k), "guard rows behind sigma were written"
    return view.cpu().numpy(), int(status.cpu()[0]), info


def model_sigma(field, montgomery, k, column_src, pairs):
    P = FIELD_MODULI[field]
    omega, delta = PR.domain(P, k)
    sigma = PR.sigma_from_pairs(pairs, len(column_src), 1 << k, delta, omega, P, column_of={src: c for c, src in enumerate(column_src) if src < 5})
    return columns_bytes(sigma, P, montgomery)


def check_sigma(H, field, montgomery, k, column_src, pairs, name):
    got, status, info = device_sigma(H, field, montgomery, k, column_src, pairs)
    assert status == 0, name
    want = model_sigma(field, montgomery, k, column_src, pairs)
    assert got.shape == want.shape and np.array_equal(got, want), "%s: sigma differs in %d cells" % (name, int((got != want).any(axis=-1).sum()))
    return info


# ---- pair lists: (row, physical column, src_row, physical src_col) --------------------------------------------------------------------------
def chain_pairs(cells):
    """One pair per step of a walk over cells (permutation column = physical column here): cell i copies cell i - 1."""
    return [(r, c, pr, pc) for (pc, pr), (c, r) in zip(cells, cells[1:])]


def sample_cells(rng, k, columns, count):
    """`count` distinct usable cells (column, row) in ascending id order."""
    u = usable(k)
    ids = sorted(rng.sample(range(len(columns) * u), count))
    return [(columns[i // u], i % u) for i in ids]


def named_cases(rng):
    """(name, k, column_src, pairs)."""
    ident, k, u = (0, 1, 2, 3, 4), 9, usable(9)
    cases = [("no pairs", k, ident, []), ("one pair", k, ident, [(3, 1, 7, 2)]), ("a self-pair", k, ident, [(5, 2, 5, 2)]),
             ("duplicated pairs", k, ident, [(3, 1, 7, 2)] * 3 + [(7, 2, 3, 1), (8, 0, 3, 1), (8, 0, 3, 1)]),
             ("sources outside the image mixed in", k, ident, [(3, 1, SRC_A, 0), (4, 0, 9, 3), (5, 1, SRC_N, 2), (9, 3, SRC_B, 1), (2, 2, 4, 0), (600, 9, SRC_A, 77)])]
    cases.append(("a star", k, ident, [(1 + i, i % 5, 0, 0) for i in range(300)]))
    cases.append(("a reverse star", k, ident, [(i, i % 5, u - 1, 4) for i in range(300)]))
    tops = [(4, u - 3), (4, u - 2), (4, u - 1)]
    deep = [(top[1], top[0], nxt[1], nxt[0]) for top, nxt in zip(tops, tops[1:])]
    for j, top in enumerate(tops):
        deep += [(100 * j + i, (i + j) % 4, top[1], top[0]) for i in range(100)]
    cases.append(("reverse stars chained three deep", k, ident, deep))
    path = chain_pairs(sample_cells(rng, k, ident, 1500))
    shuffled = list(path)
    rng.shuffle(shuffled)
    cases += [("a path of 1,500 cells, ascending", k, ident, path), ("a path, descending", k, ident, [(sr, sc, r, c) for (r, c, sr, sc) in reversed(path)]),
              ("a path, shuffled", k, ident, shuffled)]
    cells = sample_cells(rng, k, ident, 1400)
    rng.shuffle(cells)
    a, b = cells[:700], cells[700:]
    cases.append(("two paths joined by the final pair", k, ident, chain_pairs(a) + chain_pairs(b) + [(b[0][1], b[0][0], a[-1][1], a[-1][0])]))
    column = [(2, r) for r in range(u)]
    rng.shuffle(column)
    cases.append(("one class that fills a column", k, ident, chain_pairs(column)))
    every = [(c, r) for c in range(5) for r in range(usable(6))]
    rng.shuffle(every)
    cases.append(("one class that is every cell", 6, ident, chain_pairs(every)))
    u11 = usable(11)
    cases.append(("4,000 random pairs", 11, ident, [(rng.randrange(u11), rng.randrange(5), rng.randrange(u11), rng.randrange(5)) for _ in range(4000)]))
    src = (4, 2, 0)
    cases.append(("column_src (4, 2, 0)", k, src, [(rng.randrange(u), rng.choice(src), rng.randrange(u), rng.choice(src)) for _ in range(400)]))
    return cases


@pytest.mark.parametrize("field,montgomery", COMBOS, ids=COMBO_IDS)
def test_sigma_is_the_models_on_named_shapes(H, field, montgomery):
    rounds = {}
    for name, k, src, pairs in named_cases(random.Random("keygen/gpu/named")):
        info = check_sigma(H, field, montgomery, k, src, pairs, name)
        rounds[name] = info.hook_rounds
        if not pairs:
            assert (info.hook_rounds, info.touched_cells, info.sort_passes) == (0, 0, 0)
    assert rounds["a reverse star"] > 2 and rounds["reverse stars chained three deep"] > 2      # more than one changing round


@pytest.mark.parametrize("field,montgomery", COMBOS, ids=COMBO_IDS)
def test_sigma_is_the_models_on_swept_shapes(H, field, montgomery):
    rng = random.Random("keygen/gpu/sweep")
    for k in range(4, 12):
        for m in (1, 2, 5, 8):
            src, u = tuple(range(m)), usable(k)                            # (m = 8: three extra columns, which no pair names)
            phys = [s for s in src if s < 5]
            pairs = [(rng.randrange(u), rng.choice(phys), rng.randrange(u), rng.choice(phys)) for _ in range(min(3 * u, 150))]
            pairs += [(rng.randrange(u), rng.choice(phys), rng.choice(PR.H2R_COPY_SRC), 0), pairs[0], (1, phys[-1], 1, phys[-1])]
            info = check_sigma(H, field, montgomery, k, src, pairs, "k = %d, m = %d" % (k, m))
            assert info.sort_passes == ((m << k) - 1).bit_length() // 8 + (1 if ((m << k) - 1).bit_length() % 8 else 0)


@pytest.mark.parametrize("field,montgomery", COMBOS, ids=COMBO_IDS)
def test_the_order_of_the_pairs_does_not_matter(H, field, montgomery):
    rng = random.Random("keygen/gpu/order")
    u = usable(10)
    pairs = [(rng.randrange(u), rng.randrange(5), rng.randrange(u), rng.randrange(5)) for _ in range(2500)]
    other = [(sr, sc, r, c) if i % 3 == 0 else (r, c, sr, sc) for i, (r, c, sr, sc) in enumerate(pairs)]
    rng.shuffle(other)
    a, st_a, _ = device_sigma(H, field, montgomery, 10, (0, 1, 2, 3, 4), pairs)
    b, st_b, _ = device_sigma(H, field, montgomery, 10, (0, 1, 2, 3, 4), other)
    assert st_a == st_b == 0 and np.array_equal(a, b)
    assert np.array_equal(a, model_sigma(field, montgomery, 10, (0, 1, 2, 3, 4), pairs))


@pytest.mark.parametrize("field,montgomery", COMBOS, ids=COMBO_IDS)
def test_sigma_status_cases(H, field, montgomery):
    k, u = 8, usable(8)
    good = [(3, 1, 7, 2), (9, 0, 3, 1)]
    for name, src, bad in (("row >= u", (0, 1, 2, 3, 4), (u, 0, 1, 1)), ("src_row >= u", (0, 1, 2, 3, 4), (1, 1, u, 0)), ("row far out", (0, 1, 2, 3, 4), (2 ** 32 - 300, 0, 1, 1)),
                           ("a column that column_src does not hold", (4, 2, 0), (1, 1, 2, 2)), ("a source column likewise", (4, 2, 0), (1, 4, 2, 3)),
                           ("a column >= 5", (0, 1, 2, 3, 4), (1, 5, 2, 2)), ("an unknown source marker", (0, 1, 2, 3, 4), (1, 1, 0xFFFFFF04, 2))):
        _, status, _ = device_sigma(H, field, montgomery, k, src, [p for p in good if p[1] in src and p[3] in src] + [bad])
        assert status == E_SHAPE, name
    _, status, _ = device_sigma(H, field, montgomery, k, (0, 1, 2, 3, 4), [(u - 8, 0, 1, 1)], first_row=7)       # first_row is added to both rows
    assert status == 0
    _, status, _ = device_sigma(H, field, montgomery, k, (0, 1, 2, 3, 4), [(u - 7, 0, 1, 1)], first_row=7)
    assert status == E_SHAPE
    got, status, _ = device_sigma(H, field, montgomery, k, (0, 1, 2, 3, 4), [(3, 1, 7, 2)], first_row=7)
    assert status == 0 and np.array_equal(got, model_sigma(field, montgomery, k, (0, 1, 2, 3, 4), CR.shifted_pairs([(3, 1, 7, 2)], 7)))


# ---- the fixed columns -----------------------------------------------------------------------------------------------------------------------
def device_fixed(H, chip, la, kinds, k, first_row=0):
    full, view = guarded(15, 1 << k)
    status = torch.zeros(1, dtype=torch.uint8, device="cuda")
    fixed, st = H.prover.keygen_fixed_columns(chip, la, np.asarray(kinds, dtype=np.uint8), k, BF, first_row=first_row, out=(view, status))
    torch.cuda.synchronize()
    assert fixed is view and st is status and intact(full, 1 << k), "guard rows behind the fixed columns were written"
    return view.cpu().numpy(), int(status.cpu()[0])


def model_rows(kinds, lcfg):
    """AR.fixed_row per kind (CR.fixed_rows_of), AR.fixed_row_bits_compose for to_bits' compose kinds, which fixed_rows_of does not know."""
    g = MP.Geometry(W, L)
    return [AR.fixed_row_bits_compose(int(kd)) if kd >= 64 else AR.fixed_row(int(kd), W, L, g.carry_bits, g.carry_sub_bits, g.carry_nsub, lcfg) for kd in kinds]


def recorded_kinds(H, chip):
    from halo2_rsa_amd import _lib
    from halo2_rsa_amd._lib import lib
    x, n = chip.assign_integer([5]), chip.assign_integer([(1 << 255) | 12345])
    pl = chip.pow_mod_fixed_exp(x, G.E, n, check_in_field=True).trace.pow_layout
    k_if = chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True)
    k_pow = np.zeros(int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl))), dtype=np.uint8)
    assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k_pow.ctypes.data) == 0
    kinds = np.concatenate([k_if, k_pow])
    assert len(kinds) == G.ROWS
    return kinds


@pytest.mark.parametrize("field,montgomery", COMBOS, ids=COMBO_IDS)
def test_fixed_columns_are_the_models(H, field, montgomery):
    from halo2_rsa_amd import _lib
    from halo2_rsa_amd._lib import lib
    P, chip = FIELD_MODULI[field], chip_of(H, field, montgomery)
    la, lcfg = H.LookupArgument(chip, rsa_chip=False), AR.LookupConfig(AR.range_lens(W, L))
    kinds = recorded_kinds(H, chip)
    for first_row in (0, 7):                                               # the recorded k = 10 circuit: 746 rows
        got, status = device_fixed(H, chip, la, kinds, 10, first_row)
        want = columns_bytes(CR.fixed_columns(CR.fixed_rows_of(kinds, W, L, lcfg), lcfg.table(), 1 << 10, first_row, P), P, montgomery)
        assert status == 0 and np.array_equal(got, want), "first_row %d: %s" % (first_row, sorted(set(np.nonzero((got != want).any(axis=-1))[0].tolist())))
    for rsa in (False, True):                                              # every kind that has a fixed row, k = 9; the RSA table
        la_r, lcfg_r = H.LookupArgument(chip, rsa_chip=rsa), AR.LookupConfig(AR.range_lens(W, L, rsa=rsa))
        every = [kd for kd in range(256) if lib().h2r_advice_fixed_row(chip._ctx, ctypes.byref(la_r.cfg), kd, ctypes.byref(_lib.H2RFixedRow())) == 0]
        assert len(every) > 100 and (48 in every) == rsa
        synthetic = np.array(every + every[::-1] + [every[len(every) // 2]] * 40, dtype=np.uint8)
        got, status = device_fixed(H, chip, la_r, synthetic, 9, 3)
        want = columns_bytes(CR.fixed_columns(model_rows(synthetic, lcfg_r), lcfg_r.table(), 1 << 9, 3, P), P, montgomery)
        assert status == 0 and np.array_equal(got, want), "rsa %s: columns %s" % (rsa, sorted(set(np.nonzero((got != want).any(axis=-1))[0].tolist())))
        assert got[CR.QR.F_TABLE_TAG].any() and got[CR.QR.F_OVER_TAG].any() and got[8].any()
    # a kind without a fixed row: the status byte, zeros in its row, the guards intact (device_fixed)
    bad = next(kd for kd in range(256) if kd not in every)
    got, status = device_fixed(H, chip, la, np.array([every[1], bad, every[2]], dtype=np.uint8), 9)
    assert status == E_SHAPE and not got[:9, 1].any() and not got[11:, 1].any()


def test_fixed_columns_refusals(H):
    from halo2_rsa_amd import _lib
    chip = chip_of(H, "bn254_fr", False)
    la = H.LookupArgument(chip, rsa_chip=False)
    u = usable(9)
    for kw, rows in ((dict(first_row=u - 9), 10), (dict(first_row=0), u + 1)):       # first_row + rows > u
        with pytest.raises(H.H2RError) as err:
            H.prover.keygen_fixed_columns(chip, la, np.zeros(rows, dtype=np.uint8), 9, BF, **kw)
        assert err.value.code == _lib.H2R_E_SHAPE
    with pytest.raises(H.H2RError) as err:                                            # the table's rows > u
        H.prover.keygen_fixed_columns(chip, la, np.zeros(4, dtype=np.uint8), 8, BF)
    assert err.value.code == _lib.H2R_E_SHAPE and la.n_rows > usable(8)
    fixed, status = H.prover.keygen_fixed_columns(chip, la, np.zeros(10, dtype=np.uint8), 9, BF, first_row=u - 10)     # the last usable row
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def key_points(key):
    """The F + m + 1 key points of a key that keygen() made, canonical (x, y) integers."""
    q, mont = Q, key.chip.montgomery
    raw = torch.cat([key.commitments[0].reshape(-1), key.commitments[1].reshape(-1), key.ck.bases[0].contiguous().view(torch.int64).reshape(-1)]).cpu().numpy()
    words = raw.view(np.uint64).reshape(-1, 4).tolist()
    vals = [sum(int(w[i]) << (64 * i) for i in range(4)) for w in words]
    if mont:
        rinv = pow(1 << 256, -1, q)
        vals = [v * rinv % q for v in vals]
    return list(zip(vals[0::2], vals[1::2]))


def proofs_of(H, key, image, montgomery):
    proof, status = H.prover.create_proof(key, image, CP.B, seed=CP.SEED, instances=CP.instances_tensor(montgomery))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * CP.B
    return proof


def accepts(H, key, proofs, montgomery):
    vk = key.verifying_key()
    accept, status = VG.verdicts(H, vk, VG.pairing_key(H, vk, montgomery), proofs, CP.instances_tensor(montgomery))
    assert status == [0] * CP.B
    return accept


def vk_integer(key):
    from halo2_rsa_amd._marshal import from_words
    return from_words(key.vk[0].tolist())


def end_to_end(H, montgomery, chip, dom, la, cfg, fixed, sigma, kinds, pairs, image):
    """The checks of one circuit: `fixed`, `sigma` the host-built columns (integers), `pairs` counted inside the image."""
    P = CP.P
    ck = CP.commit_key(H, chip, cfg.n)
    host_key = CP.device_key(H, chip, la, cfg, fixed, sigma, kinds)
    host_pairs = np.array(pairs, dtype=np.uint32).reshape(-1, 4)
    key = H.prover.keygen(chip, dom, ck, la, kinds, host_pairs, cfg.blinding_factors, column_src=cfg.column_src, chunk_len=cfg.chunk_len, vk_repr=rep(CP.VK, P, montgomery))
    torch.cuda.synchronize()
    assert torch.equal(key.fixed_lag, host_key.fixed_lag) and torch.equal(key.sigma_lag, host_key.sigma_lag)
    assert (key.delta, key.gate_fixed, key.lookup) == (host_key.delta, host_key.gate_fixed, host_key.lookup) and key.proof_bytes == host_key.proof_bytes
    want = proofs_of(H, host_key, image, montgomery)
    assert torch.equal(proofs_of(H, key, image, montgomery), want)
    # the derived vk_repr is the model's over the key's own points; the key verifies what it proves
    own = H.prover.keygen(chip, dom, ck, la, kinds, host_pairs, cfg.blinding_factors, column_src=cfg.column_src, chunk_len=cfg.chunk_len, lagrange_key=key.lk)
    assert vk_integer(own) == rep(KR.vk_repr(P, *KR.config_args("bn254_fr", cfg, P, key_points(own))), P, montgomery) != vk_integer(key)
    assert torch.equal(own.commitments[0], key.commitments[0]) and torch.equal(own.commitments[1], key.commitments[1])
    vk = own.verifying_key()
    assert torch.equal(vk.key_bases[:15].view(torch.int64).reshape(1, 15, 2, 4), own.commitments[0])       # the commitments keygen formed, not new ones
    mine = proofs_of(H, own, image, montgomery)
    assert accepts(H, own, mine, montgomery) == [1] * CP.B
    # one copy pair less: another sigma, other commitments, another vk_repr; neither key accepts the other's proofs
    omega, delta = cfg.omega(P), cfg.delta
    full = PR.sigma_from_pairs(pairs, 5, cfg.n, delta, omega, P)
    drop = next(i for i, p in enumerate(pairs) if p[2] not in PR.H2R_COPY_SRC and PR.sigma_from_pairs(pairs[:i] + pairs[i + 1:], 5, cfg.n, delta, omega, P) != full)
    less = H.prover.keygen(chip, dom, ck, la, kinds, np.delete(host_pairs, drop, axis=0), cfg.blinding_factors, column_src=cfg.column_src, chunk_len=cfg.chunk_len,
                           lagrange_key=key.lk)
    assert not torch.equal(less.commitments[1], own.commitments[1]) and torch.equal(less.commitments[0], own.commitments[0])
    assert vk_integer(less) != vk_integer(own)
    theirs = proofs_of(H, less, image, montgomery)
    assert accepts(H, less, theirs, montgomery) == [1] * CP.B
    assert accepts(H, less, mine, montgomery) == [0] * CP.B and accepts(H, own, theirs, montgomery) == [0] * CP.B


@pytest.mark.parametrize("montgomery", REPRS, ids=["canonical", "montgomery"])
def test_keygen_end_to_end_on_the_k9_model_circuit(H, montgomery):
    circ, rows, kinds, _, _ = CP.model9()
    _, _, pairs, _ = PM.Chain().image(PM.BASE)
    host_key, image = CP.setup9(H, montgomery)
    end_to_end(H, montgomery, host_key.chip, host_key.dom, host_key.la, circ.cfg, circ.lag["fixed"], circ.lag["sigma"], np.asarray(kinds, dtype=np.uint8), list(pairs), image)


@pytest.mark.parametrize("montgomery", REPRS, ids=["canonical", "montgomery"])
def test_keygen_end_to_end_on_the_recorded_k10_circuits(H, montgomery):
    c = G.Chain(H, "bn254_fr", montgomery=montgomery)
    end_to_end(H, montgomery, c.chip, c.dom, c.la, c.cfg, c.fixed, c.sigma, c.kinds, list(c.pairs), c.emit())


def test_keygen_refuses_what_its_kernels_flag(H):
    from halo2_rsa_amd import _lib
    circ, rows, kinds, _, _ = CP.model9()
    host_key, _ = CP.setup9(H, False)
    args = (host_key.chip, host_key.dom, CP.commit_key(H, host_key.chip, circ.cfg.n), host_key.la)
    for kd, pairs in ((np.asarray(kinds, dtype=np.uint8), [(circ.cfg.u, 0, 1, 1)]), (np.array([1, 27, 1], dtype=np.uint8), [(1, 0, 2, 0)])):
        with pytest.raises(H.H2RError) as err:
            H.prover.keygen(*args, kd, np.array(pairs, dtype=np.uint32), circ.cfg.blinding_factors, lagrange_key=host_key.lk)
        assert err.value.code == _lib.H2R_E_SHAPE


# ---- the reference's size -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,montgomery", COMBOS, ids=COMBO_IDS)
def test_one_rsa2048_element_at_k17(H, field, montgomery):
    from halo2_rsa_amd import _lib
    from halo2_rsa_amd._lib import lib
    P, k, e = FIELD_MODULI[field], 17, 65537
    n, u = 1 << k, usable(k)
    chip = H.BigIntChip(64, 2048, field=field, montgomery=montgomery)
    rng = random.Random("keygen/gpu/k17/" + field)
    mod = rng.getrandbits(2048) | (1 << 2047) | 1
    res = chip.pow_mod_fixed_exp(chip.assign_integer([rng.randrange(mod)]), e, chip.assign_integer([mod]), check_in_field=True)
    assert not res.status.cpu().numpy().any()
    pl = res.trace.pow_layout
    rows_if = len(chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True))
    rows = rows_if + int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl)))
    assert rows == 77040 <= u
    copies = chip.pow_copy_map(pl, e, row_offset=rows_if)
    pairs = np.frombuffer(copies, dtype=np.uint32).reshape(-1, 4)
    omega, delta = PR.domain(P, k)
    wr, dr = rep(omega, P, montgomery), rep(delta, P, montgomery)
    src = (0, 1, 2, 3, 4)
    full, view = guarded(5, n)
    status = torch.zeros(1, dtype=torch.uint8, device="cuda")
    sigma, _, info = H.prover.keygen_sigma_columns(chip, copies, k, BF, dr, wr, src, out=(view, status))
    ident, st_ident, _ = H.prover.keygen_sigma_columns(chip, np.zeros((0, 4), dtype=np.uint32), k, BF, dr, wr, src)
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0 and int(st_ident.cpu()[0]) == 0 and intact(full, n) and info.sort_passes == 3 and info.hook_rounds >= 2
    # sigma differs from the labels exactly on the two cells of every pair that lies inside the image and is no self-pair
    inside = pairs[(pairs[:, 2] < 0xFFFFFF00) & ((pairs[:, 0] != pairs[:, 2]) | (pairs[:, 1] != pairs[:, 3]))]
    named = np.zeros((5, n), dtype=bool)
    named[inside[:, 1], inside[:, 0]] = True
    named[inside[:, 3], inside[:, 2]] = True
    differs = (sigma != ident).any(dim=-1).cpu().numpy()
    kept = pairs[pairs[:, 2] < 0xFFFFFF00]
    touched = named.copy()
    touched[kept[:, 1], kept[:, 0]] = True
    touched[kept[:, 3], kept[:, 2]] = True
    assert np.array_equal(differs, named) and int(touched.sum()) == info.touched_cells and int(named.sum()) > 100000
    # the permutation product of the recorded image closes under it; with one destination cell changed it does not
    image = res.emit_modpow_advice()
    pa = H.PermutationArgument(chip, src, 2, dr, wr)
    beta, gamma = rep(rng.randrange(1, P), P, montgomery), rep(rng.randrange(1, P), P, montgomery)
    _, st = pa.product_columns(image, 1, rows, sigma, [beta], [gamma], u)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0]
    row, col = int(inside[len(inside) // 2][0]), int(inside[len(inside) // 2][1])
    if chip.columns:
        pytest.fail("a row-major image is expected")
    image.view(1, rows, 5, 32)[0, row, col, 0] ^= 1
    _, st = pa.product_columns(image, 1, rows, sigma, [beta], [gamma], u)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [E_ASSERTION]
