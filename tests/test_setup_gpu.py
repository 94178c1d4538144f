"""The KZG setup on the device (h2r_fixed_base_table, h2r_fixed_base_mul, h2r_kzg_setup_scalars, prover.setup) byte
for byte against the plain models (tests/setup_ref.py, tests/msm_ref.py), bn254_fr (bn256 G1) in both representations; what the models made
is shared by the two.  Every output is written into a sentinel-filled buffer whose rows before and after it must stay untouched.

THE BOUNDS OF THE IMPLEMENTATION (h2r_setup.hpp) and the sizes on each side of them: one lane per element, workgroups of 256, so the sizes
are 1, 2 (a partial wavefront), 63 / 64 / 65 (a wavefront), 255 / 256 / 257 (a workgroup), 1,000 (no power of two) and 2,048 (eight
workgroups).  A launch is cut into slices of 65,535 workgroups: 2^24 elements are 65,536 of them, the slicer is the curve transform's and
tests/test_curve_ntt_gpu.py runs that size through it; here the k = 17 test is the large one.
A tau inside the domain is refused by contract (tau^n = 1: the formula divides by zero), and r - 1 = -1 = omega^(n/2) lies in EVERY domain:
the Lagrange case tau = r - 1 is therefore pinned as that refusal, at every size."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import msm_ref as M
import permutation_ref as PR
import setup_ref as S

REPRS, IDS = [False, True], ["canonical", "montgomery"]
SENTINEL, GUARD = 0xAB, 2
R, R256 = M.R_ORDER, 1 << 256
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 2048]
A = 0x1F2E3D4C5B6A79881726354453627180
TAU = random.Random("setup/gpu/tau").randrange(2, R)
CACHE = {}                      # what the models made, shared by the two representations


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def chip_of(H, montgomery):
    return H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)


def rep(v, montgomery):
    return v * R256 % R if montgomery else v


def cached(key, make):
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def omega_of(k):
    return PR.domain(R, k)[0]


def guarded(n, row):
    """(the sentinel-filled buffer, its n rows in the middle)"""
    full = torch.full((n + 2 * GUARD, row), SENTINEL, dtype=torch.uint8, device="cuda")
    return full, full[GUARD:GUARD + n]


def rows_of(full, n):
    """the n rows as bytes, after checking the guards"""
    host = full.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "bytes outside the output were written"
    return host[GUARD:GUARD + n].tobytes()


def scalars_tensor(vals, montgomery):
    return torch.frombuffer(bytearray(M.scalar_bytes(vals, montgomery)), dtype=torch.uint8).reshape(len(vals), 32).cuda()


# ---- the scalars ----------------------------------------------------------------------------------------------------------------------------
POWER_TAUS = [("0", 0), ("1", 1), ("2", 2), ("r-1", R - 1), ("root16", omega_of(4)), ("random", TAU)]


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("name,tau", POWER_TAUS, ids=[n for n, _ in POWER_TAUS])
def test_powers(H, montgomery, name, tau):
    from halo2_rsa_amd import _lib
    chip = chip_of(H, montgomery)
    want = cached(("powers", tau), lambda: S.powers(tau, max(SIZES)))
    if tau == 0:
        assert want[:3] == [1, 0, 0]
    for n in SIZES:
        full, out = guarded(n, 32)
        got = H.prover.setup_scalars(chip, _lib.H2R_SETUP_POWERS, n, rep(tau, montgomery), out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        assert rows_of(full, n) == M.scalar_bytes(want[:n], montgomery), (name, n)


LAGRANGE_TAUS = [("0", 0), ("2", 2), ("random", TAU)]


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("k", [1, 2, 6, 8, 11])
def test_lagrange(H, montgomery, k):
    from halo2_rsa_amd import _lib
    chip = chip_of(H, montgomery)
    n, omega = 1 << k, omega_of(k)
    for name, tau in LAGRANGE_TAUS:
        want = cached(("lagrange", tau, k), lambda: S.lagrange(tau, omega, k))
        assert sum(want) % R == 1
        full, out = guarded(n, 32)
        H.prover.setup_scalars(chip, _lib.H2R_SETUP_LAGRANGE, k, rep(tau, montgomery), rep(omega, montgomery), out=out)
        torch.cuda.synchronize()
        assert rows_of(full, n) == M.scalar_bytes(want, montgomery), (name, k)
    # tau = r - 1 lies in the domain (omega^(n/2) = -1): refused, nothing written
    full, out = guarded(n, 32)
    with pytest.raises(_lib.H2RError) as e:
        H.prover.setup_scalars(chip, _lib.H2R_SETUP_LAGRANGE, k, rep(R - 1, montgomery), rep(omega, montgomery), out=out)
    torch.cuda.synchronize()
    assert e.value.code == _lib.H2R_E_SHAPE and rows_of(full, n) == bytes([SENTINEL]) * (32 * n)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
def model_table(base):
    """T[w][d] = [d 256^w]B as 8,192 affine points: one addition per entry, one inversion in all"""
    if base == M.G:
        return [p for row in M.g_table() for p in row]
    rows, cur = [], M.jac(base)
    for _ in range(32):
        row = [M.JIDENT, cur]
        for _d in range(2, 256):
            row.append(M.jadd(row[-1], cur))
        rows.append(row)
        cur = M.jadd(row[-1], cur)
    return M.to_affine_batch([p for row in rows for p in row])


TABLE_BASES = [("G", lambda: M.G), ("[a]G", lambda: M.mul_g(A)), ("identity", lambda: M.IDENT)]


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("name,base", TABLE_BASES, ids=[n for n, _ in TABLE_BASES])
def test_table(H, montgomery, name, base):
    from halo2_rsa_amd import _lib
    chip = chip_of(H, montgomery)
    base = base()
    want = cached(("table", name), lambda: M.point_bytes(model_table(base), True))     # entries are in Montgomery form in either ctx
    n = _lib.H2R_FIXED_BASE_TABLE_BYTES // 64
    assert n == 8192 and len(want) == 64 * n
    full, out = guarded(n, 64)
    got = H.prover.fixed_base_table(chip, None if name == "G" else M.point_bytes([base], montgomery), out=out.reshape(-1))
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    host = rows_of(full, n)
    for w in range(32):
        assert host[w * 16384:(w + 1) * 16384] == want[w * 16384:(w + 1) * 16384], "window %d" % w
    if name == "identity":
        assert host == bytes(64 * n)
    assert host[:64] == bytes(64)                                # d = 0


# ---- the multiplication ---------------------------------------------------------------------------------------------------------------------
def mul_case():
    rng = random.Random("setup/gpu/mul")
    ks = S.edge_scalars(rng)
    ks += [rng.getrandbits(256) for _ in range(max(SIZES) - len(ks))]
    rng.shuffle(ks)
    return ks, M.mul_g_batch(ks)


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_mul(H, montgomery):
    chip = chip_of(H, montgomery)
    ks, pts = cached("mul", mul_case)
    table = H.prover.fixed_base_table(chip)
    for n in SIZES:
        sub = ks[-n:]                                            # (the edge scalars are spread over the list: every size meets some)
        scal = scalars_tensor(sub, montgomery)
        before = scal.clone()
        full, out = guarded(n, 64)
        got = H.prover.fixed_base_mul(chip, table, scal, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and torch.equal(scal, before)
        assert rows_of(full, n) == M.point_bytes(pts[-n:], montgomery), n
    # every edge scalar in one call, a column of zeros, a column of one repeated value
    edge = S.edge_scalars(random.Random(1), random_count=0)
    for vals, want in ((edge, M.mul_g_batch(edge)), ([0] * 300, [M.IDENT] * 300), ([ks[0]] * 300, [M.mul_g(ks[0])] * 300), ([R] * 65, [M.IDENT] * 65)):
        full, out = guarded(len(vals), 64)
        H.prover.fixed_base_mul(chip, table, scalars_tensor(vals, montgomery), out=out)
        torch.cuda.synchronize()
        assert rows_of(full, len(vals)) == M.point_bytes(want, montgomery)
    # another base, and the identity's table
    other = H.prover.fixed_base_table(chip, M.point_bytes([M.mul_g(A)], montgomery))
    got = H.prover.fixed_base_mul(chip, other, scalars_tensor(ks[:64], montgomery))
    ident = H.prover.fixed_base_mul(chip, H.prover.fixed_base_table(chip, bytes(64)), scalars_tensor(ks[:64], montgomery))
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == M.point_bytes(M.mul_g_batch([k * A % R for k in ks[:64]]), montgomery)
    assert ident.cpu().numpy().tobytes() == bytes(64 * 64)


# ---- two device routes against each other -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("k", [1, 6, 11, 13])
def test_the_direct_lagrange_key_is_the_curve_transforms(H, montgomery, k):
    chip = chip_of(H, montgomery)
    params = H.prover.setup(chip, k, tau=rep(TAU, montgomery))
    dom = H.EvaluationDomain(chip, k, k, rep(omega_of(k), montgomery), rep(1, montgomery))
    assert params.omega == dom.omega and (params.k, params.n, params.g.n, params.g_lagrange.n) == (k, 1 << k, 1 << k, 1 << k)
    other = dom.lagrange_key(params.g)
    torch.cuda.synchronize()
    assert torch.equal(params.g_lagrange.bases.reshape(-1), other.bases.reshape(-1))
    if k <= 11:
        pts = cached("tau powers", lambda: M.mul_g_batch(S.powers(TAU, 1 << 11)))
        assert params.g.bases.cpu().numpy().tobytes() == M.point_bytes(pts[:1 << k], montgomery)
    import pairing_ref as P
    if k == 1:
        assert params.g2 == P.g2_bytes(P.G2, montgomery) and params.s_g2 == P.g2_bytes(cached("tau g2", lambda: P.g2_mul(TAU, P.G2)), montgomery)


def test_setup_draws_tau_from_the_seed(H):
    """tau = None: the generator's element (seed, circuit 0, tag 7 * 256, row 0); one seed gives one key, another seed another"""
    import create_proof_ref as C
    chip = chip_of(H, False)
    seed = bytes(range(32))
    a, b, c = H.prover.setup(chip, 3, seed=seed), H.prover.setup(chip, 3, seed=seed), H.prover.setup(chip, 3)
    torch.cuda.synchronize()
    assert torch.equal(a.g.bases, b.g.bases) and a.s_g2 == b.s_g2 and not torch.equal(a.g.bases, c.g.bases)
    tau = C.random_element(seed, 0, 7 * 256, 0)
    assert H.prover.TAG_SETUP == 7 * 256 and a.g.bases.cpu().numpy().tobytes() == M.point_bytes(M.mul_g_batch(S.powers(tau, 8)), False)


# ---- scale ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_k17(H, montgomery):
    """No per-point model at this size: the two keys are held to what their commitments must be -- g.commit(f) = [f(tau)]G,
    g_lagrange.commit(v) = [sum v_i l_i(tau)]G, g_lagrange.commit(1, 1, ...) = G -- and to the model at 64 sampled indices each."""
    k, n = 17, 1 << 17
    chip = chip_of(H, montgomery)

    def model():
        rng = random.Random("setup/gpu/k17")
        f = [rng.randrange(R) for _ in range(n)]
        v = [rng.randrange(R) for _ in range(n)]
        lag = S.lagrange(TAU, omega_of(k), k)
        acc = 0
        for c in reversed(f):
            acc = (acc * TAU + c) % R
        idx = sorted(rng.sample(range(n), 62) + [0, n - 1])
        return f, v, M.mul_g(acc), M.mul_g(sum(a * b for a, b in zip(v, lag)) % R), idx, [M.mul_g(pow(TAU, i, R)) for i in idx], [M.mul_g(lag[i]) for i in idx]

    f, v, want_f, want_v, idx, want_g, want_l = cached("k17", model)
    params = H.prover.setup(chip, k, tau=rep(TAU, montgomery))
    cols = [scalars_tensor(c, montgomery) for c in (f, v, [1] * n)]
    cf = params.g.commit(cols[:1])
    cl = params.g_lagrange.commit(cols[1:])
    sel = torch.tensor(idx, device="cuda")
    g_s, l_s = params.g.bases[sel], params.g_lagrange.bases[sel]
    torch.cuda.synchronize()
    assert cf.cpu().numpy().tobytes() == M.point_bytes([want_f], montgomery)
    assert cl.cpu().numpy().tobytes() == M.point_bytes([want_v, M.G], montgomery)
    assert g_s.cpu().numpy().tobytes() == M.point_bytes(want_g, montgomery)
    assert l_s.cpu().numpy().tobytes() == M.point_bytes(want_l, montgomery)
