"""The Lagrange-basis key on the device (CommitKey.transform, EvaluationDomain.lagrange_key: h2r_curve_ntt) byte for
byte against the plain model (tests/curve_ntt_ref.py), bn254_fr (bn256 G1) in both representations; what the model made is shared by the two.
The output and the workspace lie between sentinel-filled guards.

THE BOUNDS OF THE IMPLEMENTATION (h2r_curve_ntt.hpp), and the sizes on each side of them -- all inside log_n = 1 .. 11:
  * a stage is numbered twiddle-major, and multiplies by the wave-uniform double-and-add, where it has >= 64 butterflies per twiddle
    (n / 2^s >= 64); otherwise group-major with the lane's 2-bit windows.  log_n <= 6: every stage windowed; log_n = 7: the first
    twiddle-major stage (stage 1, twiddle 1: no multiplication); log_n = 8: the first wave-uniform multiplication (stage 2); from there
    on the last six stages are windowed and the others uniform.
  * a workgroup is 256 lanes: the load / store launches cross it between log_n = 8 and 9, the stages (n / 2 butterflies) between 9 and 10.
  * one stage per launch at every size; log_n = 1 is the single butterfly with twiddle 1, log_n = 2 brings the first real twiddle.
  * a launch is cut into slices of at most 65,535 workgroups: only the load and the store of log_n = 24 (65,536 workgroups) reach that, and
    their last workgroup is then a launch of its own with a non-zero first-workgroup index.  A bound above 2^11: covered by the 2^17 case
    plus test_two_to_the_twenty_four, the one case here that takes tens of seconds (a fault in that index shows at no smaller size)."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import curve_ntt_ref as C
import msm_ref as M

REPRS = [False, True]
IDS = ["canonical", "montgomery"]
SENTINEL, GUARD = 0xAB, 2
A0, D = 0x1234567890abcdef1122334455667788, 0x0fedcba987654321ffeeddccbbaa9988   # the structured bases: P_j = [A0 + j D]G
R, R256 = M.R_ORDER, 1 << 256
CACHE = {}                      # what the model made, shared by the two representations


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def chip_of(H, montgomery, field="bn254_fr"):
    return H.BigIntChip(64, 256, field=field, montgomery=montgomery)


def rep(v, montgomery, P=R):
    return v * R256 % P if montgomery else v


def cached(key, make):
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def structured(n):
    """(points, logs) of the first n structured bases; the 2^12 every small test shares are made once."""
    big = cached("bases", lambda: M.structured_bases(1 << 12, A0, D))
    return big[:n], [(A0 + j * D) % R for j in range(n)]


def key_of(H, chip, points, montgomery):
    raw = M.point_bytes(points, montgomery)
    return H.CommitKey(chip, torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(len(points), 64).cuda())


def transform(H, montgomery, points, k, inverse, chip=None):
    """The device's transform of the first 2^k of `points` as bytes, between guards."""
    import ctypes
    from halo2_rsa_amd import _lib
    chip = chip or chip_of(H, montgomery)
    n = 1 << k
    key = key_of(H, chip, points, montgomery)
    cfg = _lib.H2RCurveNttConfig()
    cfg.struct_size, cfg.log_n = ctypes.sizeof(cfg), k
    need = int(_lib.lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(cfg)))
    assert need > 0
    out_full = torch.full((n + GUARD, 64), SENTINEL, dtype=torch.uint8, device="cuda")
    ws_full = torch.full((256 + need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
    before = key.bases.clone()
    got = key.transform(rep(C.omega_of(k), montgomery), k=k, inverse=inverse, out=out_full[:n], workspace=ws_full[256:256 + need])
    torch.cuda.synchronize()
    assert got.n == n and got.bases.data_ptr() == out_full.data_ptr() and got.chip is chip
    assert torch.equal(before, key.bases), "the input was written"
    host = out_full.cpu().numpy()
    assert (host[n:] == SENTINEL).all(), "guard rows behind the output were written"
    wsh = ws_full.cpu().numpy()
    assert (wsh[:256] == SENTINEL).all() and (wsh[256 + need:] == SENTINEL).all(), "the workspace's neighbours were written"
    return host[:n].tobytes()


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("inverse", [True, False], ids=["inverse", "forward"])
@pytest.mark.parametrize("k", list(range(1, 12)))
def test_sizes_against_the_logarithm_route(H, montgomery, inverse, k):
    """log_n = 1 .. 11: every bound the module's docstring lists has a size on each side.  From n = 4 on one base is (0, 0)."""
    n = 1 << k
    points, logs = structured(n)
    points, logs = list(points), list(logs)
    if n >= 4:
        points[n // 2 + 1], logs[n // 2 + 1] = M.IDENT, 0
    want = cached(("sizes", k, inverse), lambda: C.by_logs(logs, C.omega_of(k), inverse))
    assert transform(H, montgomery, points, k, inverse) == M.point_bytes(want, montgomery)


def unstructured_case(name, n):
    rng = random.Random("curve_ntt/unstructured/%s/%d" % (name, n))
    pts = M.mul_g_batch([rng.randrange(1, R) for _ in range(n)])
    if name == "identities":                      # (0, 0) at the first, a middle and the last index (what of them n leaves apart)
        for i in {2: (0,), 4: (0, 2)}.get(n, (0, n // 2, n - 1)):
            pts[i] = M.IDENT
    elif name == "repeats":                       # P and -P as the pair of a first-stage butterfly (n / 2 apart); a point repeated
        pts[n // 2] = M.neg(pts[0])
        if n >= 4:
            pts[3] = pts[1]
        if n >= 8:
            pts[6] = pts[5] = pts[1]
    return pts


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("name", ["random", "identities", "repeats"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_unstructured_input_against_the_definition(H, montgomery, name, k):
    n = 1 << k
    pts = cached(("unstructured", name, n), lambda: unstructured_case(name, n))
    for inverse in (True, False):
        want = cached(("unstructured/want", name, n, inverse), lambda: C.naive(pts, C.omega_of(k), inverse))
        assert transform(H, montgomery, pts, k, inverse) == M.point_bytes(want, montgomery), (name, n, inverse)
    if name == "repeats" and n == 2:
        assert transform(H, montgomery, pts, k, False)[:64] == bytes(64), "P + (-P) is written as (0, 0)"


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_all_identities_stay_identities(H, montgomery, k):
    for inverse in (True, False):
        assert transform(H, montgomery, [M.IDENT] * (1 << k), k, inverse) == bytes(64 << k)


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_forward_undoes_inverse_at_two_to_the_twelve(H, montgomery):
    k = 12
    points, _ = structured(1 << k)
    raw = M.point_bytes(points, montgomery)
    lagrange = transform(H, montgomery, points, k, True)
    assert lagrange != raw
    chip = chip_of(H, montgomery)
    key = H.CommitKey(chip, torch.frombuffer(bytearray(lagrange), dtype=torch.uint8).reshape(1 << k, 64).cuda())
    back = key.transform(rep(C.omega_of(k), montgomery), inverse=False)
    torch.cuda.synchronize()
    assert back.bases.cpu().numpy().tobytes() == raw


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_downsize_the_transform_at_k_of_a_longer_key(H, montgomery):
    k = 5
    points, _ = structured(2 << k)
    chip = chip_of(H, montgomery)
    long_key, short_key = key_of(H, chip, points, montgomery), key_of(H, chip, points[:1 << k], montgomery)
    w = rep(C.omega_of(k), montgomery)
    a, b = long_key.transform(w, k=k), short_key.transform(w)
    torch.cuda.synchronize()
    assert a.n == b.n == 1 << k and torch.equal(a.bases, b.bases) and a.bases.any()
    odd = key_of(H, chip, points[:48], montgomery)                    # n is no power of two: k must be given, and fit
    for kw in ({}, {"k": 6}, {"k": 0}):
        with pytest.raises(H.H2RError):
            odd.transform(w, **kw)
    c = odd.transform(w, k=k)
    torch.cuda.synchronize()
    assert torch.equal(c.bases, b.bases)


def big_case():
    k = 17
    return cached("2^17", lambda: M.structured_bases(1 << k, A0, D))


@pytest.mark.parametrize("montgomery", REPRS, ids=IDS)
def test_two_to_the_seventeen(H, montgomery):
    """64 indices of g_lagrange against the closed form; then, on the device alone, a random Lagrange-form column commits under the Lagrange
    key to what its coefficients commit to under the monomial key."""
    k = 17
    n = 1 << k
    points = big_case()
    omega = C.omega_of(k)
    rng = random.Random("curve_ntt/2^17")
    idx = cached("2^17/idx", lambda: [0, 1, n // 2, n - 1, 63, 64, 65, n // 2 - 1, n // 2 + 1] + [rng.randrange(n) for _ in range(55)])
    assert len(idx) == 64
    want = cached("2^17/want", lambda: M.mul_g_batch(C.closed_form_logs(n, A0, D, omega, idx)))
    chip = chip_of(H, montgomery)
    key = key_of(H, chip, points, montgomery)
    dom = H.EvaluationDomain(chip, k, k, rep(omega, montgomery), rep(1, montgomery))
    lag = dom.lagrange_key(key)
    torch.cuda.synchronize()
    assert lag.n == n
    host = lag.bases.cpu().numpy()
    for i, p in zip(idx, want):
        assert host[i].tobytes() == M.point_bytes([p], montgomery), i
    f = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda")
    f[:, 31] &= 0x0F                                                    # below 2^252 < r: field elements in either representation
    a = lag.commit([f])
    b = key.commit([dom.lagrange_to_coeff(f)])
    torch.cuda.synchronize()
    assert torch.equal(a, b) and a.any()


def test_two_to_the_twenty_four(H):
    """The largest size, the only one whose load and store are cut into two launches (65,535 workgroups and one).  The input is the 2^17
    structured bases repeated 128 times, so the model knows the whole inverse transform: index 128 t holds index t of the 2^17 transform
    (the closed form), every other index (0, 0).  The last workgroup of the store -- the second launch -- holds indices n - 256 and
    n - 128 of them; the last workgroup of the load feeds every output.  Then forward(inverse(g)) == g byte for byte.  One representation."""
    k, m_log, montgomery = 24, 17, True
    n, m = 1 << k, 1 << m_log
    block = big_case()
    omega = C.omega_of(k)
    assert pow(omega, n // m, R) == C.omega_of(m_log)
    ts = [0, 1, m // 2, m - 2, m - 1]
    want = cached("2^24/want", lambda: M.mul_g_batch(C.closed_form_logs(m, A0, D, C.omega_of(m_log), ts)))
    chip = chip_of(H, montgomery)
    g = key_of(H, chip, block, montgomery).bases.repeat(n // m, 1)
    key = H.CommitKey(chip, g)
    lag = key.transform(rep(omega, montgomery))
    torch.cuda.synchronize()
    rows = lag.bases.view(m, n // m, 64)
    assert not bool(rows[:, 1:].any()), "an index that is no multiple of 128 is not (0, 0)"
    assert bool(rows[:, 0].any(dim=1).all())
    for t, p in zip(ts, want):
        assert rows[t, 0].cpu().numpy().tobytes() == M.point_bytes([p], montgomery), t
    back = lag.transform(rep(omega, montgomery), inverse=False)
    torch.cuda.synchronize()
    assert torch.equal(back.bases, g)
    del back, lag, key, g, rows
    torch.cuda.empty_cache()


def test_a_field_without_a_curve_is_refused(H):
    from halo2_rsa_amd import _lib
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    from pyref import FIELD_MODULI
    for montgomery in REPRS:
        for field, k in (("bn254_fq", 1), ("pasta_fp", 5), ("pasta_fq", 5)):
            P = FIELD_MODULI[field]
            chip = chip_of(H, montgomery, field=field)
            key = H.CommitKey(chip, torch.zeros((1 << k, 2, 4), dtype=torch.int64, device="cuda"))
            with pytest.raises(H.H2RError) as err:
                key.transform(rep(C.NR.omega_of(P, k), montgomery, P), k=k)
            assert err.value.code == _lib.H2R_E_UNSUPPORTED, field
            with pytest.raises(H.H2RError) as err:                       # ... after the shape checks: omega = 1 is no primitive root
                key.transform(rep(1, montgomery, P), k=k)
            assert err.value.code == _lib.H2R_E_SHAPE, field
