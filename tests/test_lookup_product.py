"""h2r_lookup_input_columns / h2r_lookup_product_columns: the lookup argument's compressed input column A (original row order) and the
grand-product column Z of halo2's plonk::lookup::prover::commit_product [3P, restated in DESIGN.md section 2d], against Python big integers.

The plain model: A = AR.compress(AR.lookup_inputs(cells decoded from the GPU image itself, AR.fixed_row of every row's kind)), S =
AR.table_column, A' / S' = AR.permute_expression_pair, Z by the recurrence Z[i+1] = Z[i] * (A+beta)(S+gamma) * ((A'+beta)(S'+gamma))^-1 with
pow(den, -1, P).  The kernels work in tiles of GRAND_PRODUCT_TILE rows (read from csrc/h2r_grand_product.hpp: 1,024); the usable rows are
chosen against it: a column shorter than one tile (1,018), columns of 8 and 32 tiles with a ragged last tile (8,186, 32,762), and -- since
2^k - 6 is never a multiple of a power-of-two tile -- one circuit with usable_rows = 2 * tile exactly, where Z[usable_rows] is the first row
of a tile that no column row starts (the "length + 1 crosses a tile boundary" case)."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import advice_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R256 = 1 << 256
M64 = (1 << 64) - 1
SENTINEL = 0xAB
with open(os.path.join(ROOT, "halo2_rsa_amd", "csrc", "h2r_grand_product.hpp")) as _f:
    TILE = int(re.search(r"GRAND_PRODUCT_TILE = (\d+);", _f.read()).group(1))


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


def _P(field):
    return __import__("pyref").FIELD_MODULI[field]


def rand_modulus(rng, bits):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def usable_for(rows):
    k = 1
    while (1 << k) - 6 < rows:
        k += 1
    return (1 << k) - 6


def ints_of(t):
    """uint8 [..., n, 32] device tensor -> nested lists of Python integers (little-endian elements)."""
    a = np.ascontiguousarray(t.cpu().numpy())
    w = a.view("<u8").reshape(-1, 4)
    flat = [x0 | x1 << 64 | x2 << 128 | x3 << 192 for x0, x1, x2, x3 in w.tolist()]
    return np.array(flat, dtype=object).reshape(a.shape[:-1])


def bytes_of(vals, P, montgomery):
    """list of canonical integers -> uint8 [n, 32] in the ctx's representation."""
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        if montgomery:
            v = v * R256 % P
        out[i] = (v & M64, (v >> 64) & M64, (v >> 128) & M64, v >> 192)
    return out.view(np.uint8).reshape(len(vals), 32)


def in_repr(vals, P, montgomery):
    return [v * R256 % P for v in vals] if montgomery else list(vals)


def decode(chip, elem_host, rows, P):
    """One element's image bytes -> [[5 canonical integers]] (a Montgomery ctx: divided by R)."""
    a = np.ascontiguousarray(elem_host, dtype=np.uint8)
    a = a.reshape(5, rows, 32).transpose(1, 0, 2) if chip.columns else a.reshape(rows, 5, 32)
    w = np.ascontiguousarray(a).view("<u8").reshape(rows * 5, 4).tolist()
    rinv = pow(R256, -1, P)
    cells = [x0 | x1 << 64 | x2 << 128 | x3 << 192 for x0, x1, x2, x3 in w]
    assert all(v < P for v in cells)
    if chip.montgomery:
        cells = [v * rinv % P if v else 0 for v in cells]
    return [cells[5 * r:5 * r + 5] for r in range(rows)]


class Case:
    """A batch of modpow_public_key elements ([assert_in_field rows][pow rows]) on the GPU and everything the model needs of it."""

    def __init__(self, H, w, L, e, field, rsa_chip, B=3, seed=1, **repr_kw):
        from halo2_rsa_amd import _lib
        from halo2_rsa_amd._lib import lib
        self.P, self.B = _P(field), B
        self.chip = chip = H.BigIntChip(w, w * L, field=field, **repr_kw)
        self.la = H.LookupArgument(chip, rsa_chip=rsa_chip)
        rng = random.Random(seed)
        N = [rand_modulus(rng, w * L) for _ in range(B)]
        X = [rng.randrange(n) for n in N]
        res = chip.pow_mod_fixed_exp(chip.assign_integer(X), e, chip.assign_integer(N), check_in_field=True)
        assert not res.status.cpu().numpy().any()
        pl = res.trace.pow_layout
        k_if = chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True)
        k_pow = np.zeros(int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl))), dtype=np.uint8)
        assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k_pow.ctypes.data) == 0
        self.kinds = np.concatenate([k_if, k_pow])
        self.rows = len(self.kinds)
        self.image = res.emit_modpow_advice()
        torch.cuda.synchronize()
        self.cfg = AR.LookupConfig(AR.range_lens(w, L, rsa=rsa_chip))
        lo = chip.layout
        self.fixed = [AR.fixed_row(int(k), w, L, lo.carry_bits, lo.carry_sub_bits, lo.carry_nsub, self.cfg) for k in self.kinds]
        host = self.image.cpu().numpy().reshape(B, -1)
        self.cells = [decode(chip, host[b], self.rows, self.P) for b in range(B)]
        self.hist = self.la.hist_advice(self.kinds, self.image, B, self.la.new_hist(B))

    def model(self, b, theta, beta, gamma, usable, first_row=0, cells=None):
        """(A[5], A'[5], S'[5], Z[5]) of circuit b as lists of canonical integers (cells: another image's PHYSICAL cells of that circuit)."""
        P = self.P
        inputs = AR.lookup_inputs(self.cells[b] if cells is None else cells, self.fixed, usable)
        S = AR.table_column(self.cfg, theta, usable, P)
        out = ([], [], [], [])
        for name in AR.ARGS:
            A = AR.compress([(0, 0)] * first_row + inputs[name][:usable - first_row], theta, P)
            Ap, Sp = AR.permute_expression_pair(A, S)
            Z, inv = [1], {}
            for i in range(usable):
                den = (Ap[i] + beta) * (Sp[i] + gamma) % P
                if den not in inv:                      # (a few hundred distinct denominators per column: each inverted once)
                    inv[den] = pow(den, -1, P)
                Z.append(Z[-1] * (A[i] + beta) % P * (S[i] + gamma) % P * inv[den] % P)
            for lst, v in zip(out, (A, Ap, Sp, Z)):
                lst.append(v)
        return out

    def run(self, thetas, betas, gammas, usable, first_row=0, image=None, kinds=None, layout=None):
        """The device's A, A', S', Z, status for per-circuit challenges given as canonical integers."""
        m, P = self.chip.montgomery, self.P
        th, be, ga = in_repr(thetas, P, m), in_repr(betas, P, m), in_repr(gammas, P, m)
        image = self.image if image is None else image
        kinds = self.kinds if kinds is None else kinds
        a_in = self.la.input_columns(kinds, image, self.B, th, usable, first_row=first_row, layout=layout)
        a_perm, s_perm, st = self.la.permuted_columns(self.hist, th, usable)
        z, zst = self.la.product_columns(a_in, a_perm, s_perm, th, be, ga, usable)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any()
        return a_in, a_perm, s_perm, z, zst

    def assert_equal(self, got, want, b):
        """got: device tensors (A, A', S', Z); want: the model's lists of circuit b."""
        for name, g, w in zip(("A", "A'", "S'", "Z"), got, want):
            gh = g[b].cpu().numpy()
            for k in range(5):
                assert np.array_equal(gh[k], bytes_of(w[k], self.P, self.chip.montgomery)), (name, b, AR.ARGS[k])


def challenges(P, seed):
    """theta in {random, 1, P - 1} (colliding and wrapping compressions), beta / gamma random, one circuit with gamma = P - 1 -- the one
    with the random theta: under theta = 1 or P - 1 the table holds the value 1 (tag 1 + 0, -1 + 2), and S + gamma = 0 there is a zero
    denominator, which is the red case below and not parity."""
    rng = random.Random(seed)
    return [rng.randrange(P), 1, P - 1], [rng.randrange(1, P) for _ in range(3)], [P - 1, rng.randrange(P), rng.randrange(P)]


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
PARITY = [  # (w, L, e, field, rsa_chip, usable_rows (None: 2^k - 6 for the smallest k that fits), first_row)
    (64, 4, 65537, "bn254_fq", False, None, 0),     # 4,996 rows in 8,186: eight tiles, the last one ragged
    (32, 8, 0b1011, "pasta_fp", False, None, 7),    # 4,560 rows from row 7 of 8,186
    (64, 32, 5, "bn254_fr", True, None, 0),         # 21,404 rows in 32,762: 32 tiles, RangeChip's 4-bit table
    (64, 4, 1, "bn254_fq", False, None, 0),         # 746 rows in 1,018: shorter than one tile
    (64, 4, 1, "bn254_fq", False, 2 * TILE, 7),     # Z[usable_rows] lies behind the last tile
]


@pytest.mark.parametrize("w,L,e,field,rsa_chip,usable,first_row", PARITY)
def test_parity_with_the_plain_model(H, w, L, e, field, rsa_chip, usable, first_row):
    c = Case(H, w, L, e, field, rsa_chip, seed=w + L + e)
    usable = usable or usable_for(c.rows + first_row)
    tiles = (usable + TILE - 1) // TILE
    print("rows %d usable %d tiles %d" % (c.rows, usable, tiles))
    if e == 65537 or L == 32:
        assert tiles >= 3 and usable % TILE
    if e == 1:
        assert usable < TILE or usable % TILE == 0
    thetas, betas, gammas = challenges(c.P, usable)
    a_in, a_perm, s_perm, z, zst = c.run(thetas, betas, gammas, usable, first_row)
    assert zst.cpu().tolist() == [0, 0, 0]
    assert z.shape == (3, 5, usable + 1, 32)
    for b in range(3):
        c.assert_equal((a_in, a_perm, s_perm, z), c.model(b, thetas[b], betas[b], gammas[b], usable, first_row), b)


# ---- 2. representations ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(H):
    """The (64, 4, 65537) case in the default representation with its model, shared by the tests below (never modified)."""
    c = Case(H, 64, 4, 65537, "bn254_fq", False, seed=11)
    usable = usable_for(c.rows)
    thetas, betas, gammas = challenges(c.P, 77)
    want = [c.model(b, thetas[b], betas[b], gammas[b], usable) for b in range(3)]
    return c, usable, (thetas, betas, gammas), want


def test_representations_and_layout(H, small):
    from halo2_rsa_amd import _lib
    from halo2_rsa_amd._lib import lib
    c0, usable, (thetas, betas, gammas), want = small
    P = c0.P
    got = {}
    for key, kw in (("default", dict()), ("columns", dict(columns=True)), ("montgomery", dict(montgomery=True)),
                    ("both", dict(columns=True, montgomery=True))):
        c = Case(H, 64, 4, 65537, "bn254_fq", False, seed=11, **kw)
        a_in, a_perm, s_perm, z, zst = c.run(thetas, betas, gammas, usable)
        assert zst.cpu().tolist() == [0, 0, 0], key
        for b in range(3):
            c.assert_equal((a_in, a_perm, s_perm, z), want[b], b)       # Montgomery: the canonical value * 2^256 mod p
        got[key] = (a_in, z)
    for i in range(2):   # row-major or planar image: the same A and Z
        assert torch.equal(got["default"][i], got["columns"][i]) and torch.equal(got["montgomery"][i], got["both"][i])
    zc, zm = ints_of(got["default"][1]), ints_of(got["montgomery"][1])
    assert all(int(m) == int(v) * R256 % P for v, m in zip(zc.reshape(-1)[::97], zm.reshape(-1)[::97]))
    # Under a custom layout: test_lookup_hist_advice.py's (kinds 6 and 7 with a and b swapped) plus the first row of a limb's range assign (kind 32, a
    # composition-lookup row) with b, c, d rotated -- column a and e must stay (layout_lookup_valid).  The lookups read PHYSICAL columns, as
    # h2r_lookup_hist_advice does: the model is fed the permuted image's physical cells, A' / S' come from hist_advice on that image under the layout.
    chip, la = c0.chip, c0.la
    lay = _lib.H2RAdviceLayout()
    ks = (ctypes.c_uint8 * 3)(6, 7, AR.ROW_RANGE_LIMB)
    cols = ((ctypes.c_uint8 * 5) * 3)((1, 0, 2, 3, 4), (1, 0, 2, 3, 4), (0, 2, 3, 1, 4))
    assert lib().h2r_advice_layout_custom(chip._ctx, ks, cols, 3, ctypes.byref(lay)) == 0
    perm = c0.image.clone()
    kd = torch.tensor(c0.kinds, device="cuda")
    assert lib().h2r_advice_apply_layout(chip._ctx, ctypes.byref(lay), kd.data_ptr(), len(c0.kinds), perm.data_ptr(), perm.shape[1], 3, None, chip._stream()) == 0
    hist_l = la.hist_advice(kd, perm, 3, la.new_hist(3), layout=lay)
    a_l = la.input_columns(kd, perm, 3, thetas, usable, layout=lay)
    ap_l, sp_l, st_l = la.permuted_columns(hist_l, thetas, usable)
    z_l, zst = la.product_columns(a_l, ap_l, sp_l, thetas, betas, gammas, usable)
    torch.cuda.synchronize()
    assert st_l.cpu().tolist() == [0, 0, 0] and zst.cpu().tolist() == [0, 0, 0]
    host = perm.cpu().numpy().reshape(3, -1)
    for b in range(3):
        c0.assert_equal((a_l, ap_l, sp_l, z_l), c0.model(b, thetas[b], betas[b], gammas[b], usable, cells=decode(chip, host[b], c0.rows, P)), b)
    a_d = got["default"][0]
    assert torch.equal(a_l[:, 0], a_d[:, 0]) and torch.equal(a_l[:, 4], a_d[:, 4])          # column a stays
    assert all(not torch.equal(a_l[:, k], a_d[:, k]) for k in (1, 2, 3))                    # b, c, d of the limb rows moved


# ---- 3. full size: the recurrence on a whole RSA-2048 verify circuit, k = 17 ----------------------------------------------------------
def _hashed_tensor(vals):
    limbs = [[(h >> (64 * j)) & M64 for j in range(4)] for h in vals]
    return torch.tensor(np.array(limbs, dtype=np.uint64).view(np.int64), device="cuda")


def test_full_size_recurrence(H, golden):
    rsa = H.RSAChip(2048, 5)
    chip = rsa.bigint_chip()
    la = H.LookupArgument(chip, rsa_chip=True)
    P = _P("bn254_fr")
    kat = golden["rsa_kats"][0]
    n, sig, hashed = int(kat["n"]), int(kat["sig"]), int(kat["hashed"])
    pk = rsa.assign_public_key(H.RSAPublicKey(H.UnassignedInteger.from_ints([n], 32, 64), H.Fix(65537)))
    sg = rsa.assign_signature(H.RSASignature(H.UnassignedInteger.from_ints([sig], 32, 64)))
    kinds = rsa.verify_pkcs1v15_signature(pk, _hashed_tensor([hashed]), sg).row_kinds()
    pipe = H.Pipeline(chip, 2, 2)
    vl = pipe.verify_compact_layout(65537)
    rows = len(kinds)
    img = torch.empty((1, chip.image_bytes(rows)), dtype=torch.uint8, device="cuda")
    wit = torch.zeros((1, vl.elem_stride), dtype=torch.uint8, device="cuda")
    ws = torch.empty(chip.workspace_bytes(1, vl.pow.num_mul_mods), dtype=torch.uint8, device="cuda")
    powed = torch.zeros((1, chip.num_limbs), dtype=torch.int64, device="cuda")
    valid, st = torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.uint8, device="cuda")
    pipe.verify_pkcs1v15_advice(chip.assign_integer([sig]), 65537, chip.assign_integer([n]), _hashed_tensor([hashed]), wit, ws, powed, valid, st, img)
    pipe.join()
    pipe.close()
    assert st.cpu().tolist() == [0] and valid.cpu().tolist() == [1]
    usable = (1 << 17) - 6
    assert rows <= usable
    rng = random.Random(17)
    theta, beta, gamma = rng.randrange(P), rng.randrange(P), rng.randrange(P)
    hist = la.hist_advice(kinds, img, 1, la.new_hist(1), status=st)
    a_in = la.input_columns(kinds, img, 1, [theta], usable, status=st)
    a_perm, s_perm, e1 = la.permuted_columns(hist, [theta], usable)
    z, zst = la.product_columns(a_in, a_perm, s_perm, [theta], [beta], [gamma], usable)
    torch.cuda.synchronize()
    assert e1.cpu().tolist() == [0] and zst.cpu().tolist() == [0]
    A, Ap, Sp, Z = ints_of(a_in[0]), ints_of(a_perm[0]), ints_of(s_perm[0]), ints_of(z[0])
    cfg = AR.LookupConfig(AR.range_lens(64, 32, rsa=True))
    S = AR.table_column(cfg, theta, usable, P)
    counts = hist[0].sum(dim=1).cpu().tolist()
    assert counts[0] > 5000 and counts[4] > 500             # composition and overflow inputs are both there
    for k in range(5):
        a, ap, sp, zz = A[k].tolist(), Ap[k].tolist(), Sp[k].tolist(), Z[k].tolist()
        assert zz[0] == 1 and zz[usable] == 1, AR.ARGS[k]
        assert sum(1 for v in a if v) == counts[k]          # every counted lookup is a nonzero input (tag * theta + value), every other row is 0
        bad = [i for i in range(usable) if (zz[i + 1] * (ap[i] + beta) % P * (sp[i] + gamma) - zz[i] * (a[i] + beta) % P * (S[i] + gamma)) % P]
        assert not bad, (AR.ARGS[k], bad[:4])


# ---- 4. red cases: only circuit 1 of three is damaged ---------------------------------------------------------------------------------
def _product(c, a_in, a_perm, s_perm, ch, usable, arg_mask=31, status=None):
    """product_columns into a sentinel-filled Z; ch = (thetas, betas, gammas) as they are handed to the device."""
    z = torch.full((3, 5, usable + 1, 32), SENTINEL, dtype=torch.uint8, device="cuda")
    st = torch.zeros(3, dtype=torch.uint8, device="cuda") if status is None else status
    c.la.product_columns(a_in, a_perm, s_perm, ch[0], ch[1], ch[2], usable, arg_mask=arg_mask, out=(z, st))
    torch.cuda.synchronize()
    return z, st.cpu().tolist()


def test_red_cases(H, small):
    from halo2_rsa_amd import _lib
    c, usable, ch, want = small
    P = c.P
    thetas, betas, gammas = ch
    a_in = c.la.input_columns(c.kinds, c.image, 3, thetas, usable)
    a_perm, s_perm, st0 = c.la.permuted_columns(c.hist, thetas, usable)
    torch.cuda.synchronize()
    sentinel = torch.full((5, usable + 1, 32), SENTINEL, dtype=torch.uint8, device="cuda")

    def others_green(z, st):
        assert st[0] == 0 and st[2] == 0
        for b in (0, 2):
            zh = z[b].cpu().numpy()
            for k in range(5):
                assert np.array_equal(zh[k], bytes_of(want[b][3][k], P, False)), (b, k)

    z, st = _product(c, a_in, a_perm, s_perm, ch, usable)               # the undamaged batch
    assert st == [0, 0, 0]
    others_green(z, st)
    good1 = z[1].clone()
    # one row of A' replaced by another table value
    bad = a_perm.clone()
    assert not torch.equal(bad[1, 0, usable - 1], bad[1, 0, 0])
    bad[1, 0, usable - 1] = bad[1, 0, 0]
    z, st = _product(c, a_in, bad, s_perm, ch, usable)
    assert st[1] == _lib.H2R_E_ASSERTION
    others_green(z, st)
    assert torch.equal(z[1, 1:], good1[1:]) and not torch.equal(z[1, 0], good1[0])                    # written as computed
    assert torch.equal(z[1, 0, :usable - 1], good1[0, :usable - 1])                                    # (Z[i] D is the same product up to the damaged row)
    # A' / S' built from a histogram with one count moved
    h2 = c.hist.clone()
    r1 = int(torch.nonzero(h2[1, 0] > 0).flatten()[-1])
    r2 = r1 - 1 if r1 > 1 else r1 + 1
    h2[1, 0, r1] -= 1
    h2[1, 0, r2] += 1
    ap2, sp2, e2 = c.la.permuted_columns(h2, thetas, usable)
    z, st = _product(c, a_in, ap2, sp2, ch, usable)
    assert e2.cpu().tolist() == [0, 0, 0] and st[1] == _lib.H2R_E_ASSERTION
    others_green(z, st)
    # beta = 0: the sorted A' starts with the (0, 0) rows, so a denominator is zero -- nothing of that circuit is written
    z, st = _product(c, a_in, a_perm, s_perm, (thetas, [betas[0], 0, betas[2]], gammas), usable)
    assert st[1] == _lib.H2R_E_ASSERTION and torch.equal(z[1], sentinel)
    others_green(z, st)
    # beta = p: not a canonical element
    z, st = _product(c, a_in, a_perm, s_perm, (thetas, [betas[0], P, betas[2]], gammas), usable)
    assert st[1] == _lib.H2R_E_SHAPE and torch.equal(z[1], sentinel)
    others_green(z, st)
    # arg_mask: the other arguments' Z stay at the sentinel
    z, st = _product(c, a_in, a_perm, s_perm, ch, usable, arg_mask=0b00101)
    assert st == [0, 0, 0]
    for b in range(3):
        for k in range(5):
            if k in (0, 2):
                assert np.array_equal(z[b, k].cpu().numpy(), bytes_of(want[b][3][k], P, False))
            else:
                assert torch.equal(z[b, k], sentinel[0])
    # a circuit whose status byte is nonzero on entry is skipped, and the byte is not cleared
    z, st = _product(c, a_in, a_perm, s_perm, ch, usable, status=torch.tensor([0, 7, 0], dtype=torch.uint8, device="cuda"))
    assert st == [0, 7, 0] and torch.equal(z[1], sentinel)
    others_green(z, st)
    # the input columns skip such a circuit too
    a2 = torch.full_like(a_in, SENTINEL)
    c.la.input_columns(c.kinds, c.image, 3, thetas, usable, status=torch.tensor([0, 7, 0], dtype=torch.uint8, device="cuda"), out=a2)
    torch.cuda.synchronize()
    assert torch.equal(a2[0], a_in[0]) and torch.equal(a2[2], a_in[2]) and bool((a2[1] == SENTINEL).all())


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------------------
def test_capacity_is_refused(H, small):
    from halo2_rsa_amd import _lib
    from halo2_rsa_amd._lib import lib
    c, usable, (thetas, betas, gammas), want = small
    la, chip = c.la, c.chip
    th, be, ga = (H._marshal.challenges(v, "cuda", 3) for v in (thetas, betas, gammas))
    kd = torch.from_numpy(c.kinds).cuda()
    a = torch.zeros((3, 5, usable, 32), dtype=torch.uint8, device="cuda")

    def inputs(first_row, u):
        return lib().h2r_lookup_input_columns(chip._ctx, ctypes.byref(la.cfg), None, kd.data_ptr(), c.rows, c.image.data_ptr(), c.image.shape[1], 3, None,
                                              th.data_ptr(), u, first_row, 31, a.data_ptr(), 5 * usable * 32, chip._stream())
    assert inputs(usable - c.rows, usable) == _lib.H2R_OK
    assert inputs(usable - c.rows + 1, usable) == _lib.H2R_E_SHAPE
    assert inputs(0, c.rows - 1) == _lib.H2R_E_SHAPE
    assert inputs(0, 0) == _lib.H2R_E_SHAPE and inputs(0, (1 << 28) + 1) == _lib.H2R_E_SHAPE      # usable_rows out of range
    bad_cfg = type(la.cfg).from_buffer_copy(la.cfg)                                                  # a hand-filled table that does not start at row 1
    bad_cfg.row_off[0] = 2
    assert lib().h2r_lookup_input_columns(chip._ctx, ctypes.byref(bad_cfg), None, kd.data_ptr(), c.rows, c.image.data_ptr(), c.image.shape[1], 3, None,
                                          th.data_ptr(), usable, 0, 31, a.data_ptr(), 5 * usable * 32, chip._stream()) == _lib.H2R_E_SHAPE
    z = torch.zeros((3, 5, usable + 1, 32), dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(lib().h2r_lookup_product_workspace_bytes(usable, 3)), dtype=torch.uint8, device="cuda")
    st = torch.zeros(3, dtype=torch.uint8, device="cuda")

    def product(col_stride, elem_stride):
        return lib().h2r_lookup_product_columns(chip._ctx, ctypes.byref(la.cfg), a.data_ptr(), a.data_ptr(), a.data_ptr(), 5 * usable * 32, th.data_ptr(),
                                                be.data_ptr(), ga.data_ptr(), 3, usable, 0, z.data_ptr(), elem_stride, col_stride, st.data_ptr(),
                                                ws.data_ptr(), chip._stream())
    col = (usable + 1) * 32
    assert product(col, 5 * col) == _lib.H2R_OK                      # (arg_mask 0: the arguments are checked, nothing runs)
    assert product(col - 32, 5 * col) == _lib.H2R_E_SHAPE            # too small
    assert product(col + 16, 5 * (col + 16)) == _lib.H2R_E_SHAPE     # not a multiple of 32
    assert product(col, 4 * col) == _lib.H2R_E_SHAPE                 # the element stride does not cover five columns
    torch.cuda.synchronize()
