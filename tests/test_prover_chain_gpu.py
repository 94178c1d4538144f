"""The per-proof half of the prover as one chain on the device, on a circuit this library records: the advice image of
three modpow_public_key elements (emit_modpow_advice: w = 64, L = 4, e = 1; 746 rows, so k = 10, u = 1,018, the extended domain 2^13), A, A',
S' and Z of LookupArgument, Z of PermutationArgument under pow_copy_map's pairs, vanishing_columns, then lagrange_to_coeff, coeff_to_extended,
quotient and extended_to_coeff.  Only the key's columns -- fixed and sigma -- are built on the host (tests/prover_chain_ref.py), and what
lies between the kernels is torch: every column is placed in a 2^k-row buffer whose rows behind u (behind u + 1 for a Z) hold random
field elements.

What is asserted needs no model of the quotient: the constraints of a recorded image hold, so h is a polynomial of degree < 4n and every
byte of its coefficients of index >= 4n is zero -- if the kernels agree on the order of the fixed columns, the rotations, the lookup
expressions, labels against sigma, Z_s[0] = Z_{s-1}[u], the place of u and first_row.  For circuit 0 the model's quotient of the same
Lagrange data, read back from the device, is compared byte for byte as well.  Every output buffer has sentinel rows behind it."""
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
import ntt_ref as NR
import permutation_ref as PR
import prover_chain_ref as CR
import quotient_ref as QR
from pyref import FIELD_MODULI
from test_lookup_product import bytes_of, in_repr, rand_modulus
from test_ntt_gpu import to_ints

W, L, E, B = 64, 4, 1, 3
ROWS, K, BF = 746, 10, 5
N_ROWS, U, N_EXT = 1 << K, (1 << K) - BF - 1, 1 << (K + 3)
COLUMN_SRC, CHUNK = (0, 1, 2, 3, 4), 2
SENTINEL, GUARD = 0xAB, 3
FIELDS = ("bn254_fr", "pasta_fq")
assert all(f in NR.FIELDS_WITH_DOMAINS for f in FIELDS) and ROWS <= U < ROWS * 2

MODEL = {}          # what the plain model made of a circuit's Lagrange data: the extensions (CR.extended's cache) and h, kept between the cases


@pytest.fixture(scope="module")
def H():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import halo2_rsa_amd as H_
    return H_


class Chain:
    """One batch of three circuits on a chip over `field` and every step from the image to the coefficients of h."""

    def __init__(self, H, field, montgomery=False, planar=False, first_row=0):
        from halo2_rsa_amd import _lib
        from halo2_rsa_amd._lib import lib
        self.H, self.field, self.P, self.mont, self.planar, self.first_row = H, field, FIELD_MODULI[field], montgomery, planar, first_row
        P = self.P
        kw = dict(columns=True, col_stride=N_ROWS * 32) if planar else {}
        self.chip = chip = H.BigIntChip(W, W * L, field=field, montgomery=montgomery, **kw)
        rng = random.Random("chain/gpu/" + field)
        mods = [rand_modulus(rng, W * L) for _ in range(B)]
        x, n = chip.assign_integer([rng.randrange(m) for m in mods]), chip.assign_integer(mods)
        self.res = res = chip.pow_mod_fixed_exp(x, E, n, check_in_field=True)
        assert not res.status.cpu().numpy().any()
        pl = res.trace.pow_layout
        k_if = chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True)
        k_pow = np.zeros(int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl))), dtype=np.uint8)
        assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k_pow.ctypes.data) == 0
        self.kinds = np.concatenate([k_if, k_pow])
        assert len(self.kinds) == ROWS and first_row + ROWS <= U
        self.pairs = [(c.row, c.col, c.src_row, c.src_col) for c in chip.pow_copy_map(pl, E, row_offset=len(k_if))]
        self.inside = [p for p in self.pairs if p[2] not in PR.H2R_COPY_SRC]
        assert len(self.inside) > 500
        self.tail_rng = random.Random("chain/gpu/tails/" + field)
        self.ch = [[rng.randrange(1, P) for _ in range(B)] for _ in range(4)]                # theta, beta, gamma, y per circuit
        self.la = H.LookupArgument(chip, rsa_chip=False)
        self.lcfg = AR.LookupConfig(AR.range_lens(W, L))
        assert self.la.n_rows == self.lcfg.n_rows <= U
        # the key, on the host: the fixed columns and sigma
        self.cfg = cfg = CR.config(P, K, BF, COLUMN_SRC, CHUNK)
        self.omega = cfg.omega(P)
        self.fixed = CR.fixed_columns(CR.fixed_rows_of(self.kinds, W, L, self.lcfg), self.lcfg.table(), N_ROWS, first_row, P)
        self.sigma = PR.sigma_from_pairs(CR.shifted_pairs(self.pairs, first_row), 5, N_ROWS, cfg.delta, self.omega, P)
        self.fixed_dev, self.sigma_dev = self.columns_tensor(self.fixed), self.columns_tensor(self.sigma)
        self.dom = H.EvaluationDomain(chip, K, K + 3, self.rep(cfg.omega_ext), self.rep(cfg.zeta))
        assert self.dom.omega == self.rep(self.omega)
        self.guards = []

    # ---- buffers ----
    def rep(self, v):
        return v * (1 << 256) % self.P if self.mont else v

    def columns_tensor(self, cols):
        return torch.from_numpy(np.stack([bytes_of(c, self.P, self.mont) for c in cols])).cuda()

    def tails(self, *shape):
        """uint8 [*shape, 32]: random field elements in the chip's representation; the same values whatever the representation."""
        count = int(np.prod(shape))
        return torch.from_numpy(bytes_of([self.tail_rng.randrange(self.P) for _ in range(count)], self.P, self.mont).reshape(*shape, 32).copy()).cuda()

    def guarded(self, lead, rows):
        """A sentinel-filled [*lead, rows + GUARD, 32]; the view of its first `rows` rows is what a kernel is given."""
        full = torch.full(tuple(lead) + (rows + GUARD, 32), SENTINEL, dtype=torch.uint8, device="cuda")
        self.guards.append((full, rows))
        return full[..., :rows, :]

    def packed(self, *shape):
        """A contiguous [*shape] for the calls whose output strides are fixed, with GUARD sentinel rows behind the whole of it."""
        numel = int(np.prod(shape))
        full = torch.full((numel // 32 + GUARD, 32), SENTINEL, dtype=torch.uint8, device="cuda")
        self.guards.append((full, numel // 32))
        return full[:numel // 32].view(*shape)

    def check_guards(self):
        torch.cuda.synchronize()
        for full, rows in self.guards:
            assert bool((full[..., rows:, :] == SENTINEL).all()), "guard rows behind an output of shape %s were written" % (tuple(full.shape),)
        self.guards = []

    def lagrange(self, cols, used):
        """[B, C, rows, 32] of a kernel -> [B, C, 2^k, 32]: the first `used` rows, random elements behind them."""
        Bc, C = cols.shape[:2]
        buf = torch.zeros((Bc, C, N_ROWS, 32), dtype=torch.uint8, device="cuda")
        buf[:, :, :used] = cols[:, :, :used]
        buf[:, :, used:] = self.tails(Bc, C, N_ROWS - used)
        return buf

    def extend(self, lag):
        lead = lag.shape[:-2]
        coeff = self.dom.lagrange_to_coeff(lag, out=self.guarded(lead, N_ROWS))
        return self.dom.coeff_to_extended(coeff, out=self.guarded(lead, N_EXT))

    # ---- the steps ----
    def emit(self):
        """The image as the kernels take it.  Planar: written into the [B, 5, 2^k, 32] buffer that is the Lagrange form of the advice columns."""
        if not self.planar:
            return self.res.emit_modpow_advice()
        buf = torch.zeros((B, 5, N_ROWS, 32), dtype=torch.uint8, device="cuda")
        buf[:, :, U:] = self.tails(B, 5, N_ROWS - U)
        before = buf.clone()
        image = self.res.emit_modpow_advice(out=buf)
        torch.cuda.synchronize()
        assert image.data_ptr() == buf.data_ptr() and tuple(image.shape) == (B, 5 * N_ROWS * 32)
        assert torch.equal(buf[:, :, ROWS:], before[:, :, ROWS:]) and bool(buf[:, :, :ROWS].any())       # the image's rows and nothing behind them
        return image

    def cell(self, image, b, row, col):
        """The 32 bytes of PHYSICAL cell (row, col) of circuit b's image."""
        return image.view(B, 5, N_ROWS, 32)[b, col, row] if self.planar else image.view(B, ROWS, 5, 32)[b, row, col]

    def advice(self, image):
        if self.planar:
            adv = image.view(B, 5, N_ROWS, 32)
            assert adv.data_ptr() == image.data_ptr()                                                # no copy: the image is the column vectors
            return adv
        assert tuple(image.shape) == (B, ROWS * 160)
        adv = torch.zeros((B, 5, N_ROWS, 32), dtype=torch.uint8, device="cuda")
        adv[:, :, self.first_row:self.first_row + ROWS] = image.view(B, ROWS, 5, 32).permute(0, 2, 1, 3)
        adv[:, :, U:] = self.tails(B, 5, N_ROWS - U)
        return adv

    def run(self, image_fault=None, s_perm_fault=None, chunk_product=CHUNK):
        """Everything from the image to the coefficients of h.  image_fault = (circuit, row, col): one image cell changed on the device before
        anything reads it; s_perm_fault = (circuit, argument, row): one entry of S' changed after the products; chunk_product: the
        permutation argument's set size as the product is told it (the quotient is always told CHUNK).  Returns a dict of what the
        assertions need, everything still on the device."""
        P, fr = self.P, self.first_row
        th, be, ga, ys = (in_repr(v, P, self.mont) for v in self.ch)
        image = self.emit()
        if image_fault:
            self.cell(image, *image_fault)[0] ^= 1
        adv = self.advice(image)
        la = self.la
        hist = la.hist_advice(self.kinds, image, B, la.new_hist(B))
        a_in = la.input_columns(self.kinds, image, B, th, U, first_row=fr, out=self.packed(B, 5, U, 32))
        a_perm, s_perm, st_perm = la.permuted_columns(hist, th, U, out=(self.packed(B, 5, U, 32), self.packed(B, 5, U, 32)))
        lz, st_lz = la.product_columns(a_in, a_perm, s_perm, th, be, ga, U, out=(self.packed(B, 5, U + 1, 32), torch.zeros(B, dtype=torch.uint8, device="cuda")))
        # the permutation's Z go straight into their 2^k-row columns: the rows behind Z[u] are the tails, and must stay what they are.  Three
        # columns whatever chunk_product is, every row a field element: the quotient reads three
        pa = self.H.PermutationArgument(self.chip, COLUMN_SRC, chunk_product, self.rep(self.cfg.delta), self.rep(self.omega))
        assert pa.sets <= len(self.cfg.sets) == 3
        pz = self.tails(B, 3, N_ROWS)
        pz_before = pz.clone()
        _, st_pz = pa.product_columns(image, B, ROWS, self.sigma_dev, be, ga, U, first_row=fr, out=(pz[:, :pa.sets], torch.zeros(B, dtype=torch.uint8, device="cuda")))
        torch.cuda.synchronize()
        assert torch.equal(pz[:, :, U + 1:], pz_before[:, :, U + 1:]) and torch.equal(pz[:, pa.sets:], pz_before[:, pa.sets:])
        assert not torch.equal(pz[:, :pa.sets, :U + 1], pz_before[:, :pa.sets, :U + 1])
        assert st_perm.cpu().tolist() == [0] * B
        if s_perm_fault:
            b, a, row = s_perm_fault
            s_perm[b, a, row, 0] ^= 1
        lag = dict(advice=adv, perm_z=pz, lookup_a_perm=self.lagrange(a_perm, U), lookup_s_perm=self.lagrange(s_perm, U), lookup_z=self.lagrange(lz, U + 1))
        ext = {name: self.extend(t) for name, t in lag.items()}
        ext["fixed"], ext["sigma"] = self.extend(self.fixed_dev), self.extend(self.sigma_dev)
        ext["l"] = self.dom.vanishing_columns(BF)
        for name, cols in (("advice", 5), ("perm_z", 3), ("lookup_a_perm", 5), ("lookup_s_perm", 5), ("lookup_z", 5)):
            assert tuple(ext[name].shape) == (B, cols, N_EXT, 32)
        assert tuple(ext["fixed"].shape) == (QR.NUM_FIXED, N_EXT, 32) and tuple(ext["sigma"].shape) == (5, N_EXT, 32) and tuple(ext["l"].shape) == (3, N_EXT, 32)
        cfg = self.cfg
        status = torch.zeros(B, dtype=torch.uint8, device="cuda")
        h, _ = self.dom.quotient(BF, self.rep(cfg.delta), cfg.gate_fixed, COLUMN_SRC, CHUNK, ext["advice"], ext["perm_z"], ext["fixed"], ext["sigma"], ext["l"],
                                 th, be, ga, ys, lookup_mask=31, lookup_advice=cfg.lookup_advice, lookup_tag=cfg.lookup_tag, lookup_enable=cfg.lookup_enable,
                                 table_tag=cfg.table_tag, table_value=cfg.table_value, lookup_a_perm=ext["lookup_a_perm"], lookup_s_perm=ext["lookup_s_perm"],
                                 lookup_z=ext["lookup_z"], out=(self.guarded((B,), N_EXT), status))
        coeffs = self.dom.extended_to_coeff(h, out=self.guarded((B,), N_EXT))
        self.check_guards()
        return dict(lag=lag, ext=ext, h=h, coeffs=coeffs.cpu().numpy(), status=status.cpu().tolist(), st_pz=st_pz.cpu().tolist(), st_lz=st_lz.cpu().tolist(),
                    image=image)


def assert_polynomial(out, circuits=range(B)):
    """Status 0 everywhere; the circuits named have zero bytes in every coefficient of index >= 4n and not only zeros below."""
    assert out["status"] == [0] * B
    for b in circuits:
        high, low = out["coeffs"][b, 4 * N_ROWS:], out["coeffs"][b, :4 * N_ROWS]
        assert not high.any(), "circuit %d: %d nonzero bytes in the coefficients of index >= 4n" % (b, int(np.count_nonzero(high)))
        assert low.any() and out["coeffs"][b, 3 * N_ROWS:4 * N_ROWS].any()


def assert_no_polynomial(out, circuits):
    assert out["status"] == [0] * B
    for b in circuits:
        assert out["coeffs"][b, 4 * N_ROWS:].any(), "circuit %d" % b


def model_of(c, out):
    """The plain model on circuit 0's Lagrange data as the device holds it: ({group: extended columns}, h).  Made once per distinct data:
    the two representations of a field hold the same values."""
    P = c.P

    def ints(t):
        return [to_ints(col, P, c.mont) for col in t.cpu().numpy()]

    lag = {name: ints(t[0]) for name, t in out["lag"].items()}
    lag.update(extra=[], fixed=ints(c.fixed_dev), sigma=ints(c.sigma_dev), l=QR.vanishing_lagrange(c.cfg))
    assert lag["fixed"] == c.fixed and lag["sigma"] == c.sigma
    ch = tuple(v[0] for v in c.ch)
    key = (P, ch, tuple(hash(tuple(col)) for name in sorted(lag) for col in lag[name]))
    if key not in MODEL:
        cols = CR.extended(QR.Circuit(cfg=c.cfg, P=P, ch=ch, lag=lag), MODEL.setdefault("extensions", {}))
        MODEL[key] = (cols, QR.quotient(c.cfg, cols, ch, P))
    return lag, MODEL[key]


# ---- 1, 2, 6: the chain in every representation, and circuit 0 byte for byte ------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("field", FIELDS)
def test_the_chain_of_a_recorded_circuit(H, field, montgomery):
    c = Chain(H, field, montgomery)
    out = c.run()
    assert out["st_pz"] == [0] * B and out["st_lz"] == [0] * B
    assert_polynomial(out)
    lag, (cols, h) = model_of(c, out)
    # what the device products are: Z_0[0] = 1, Z_s[0] = Z_{s-1}[u], the last Z[u] = 1; a lookup Z starts and ends at 1
    pz, lz = lag["perm_z"], lag["lookup_z"]
    assert pz[0][0] == 1 and pz[1][0] == pz[0][U] and pz[2][0] == pz[1][U] and pz[2][U] == 1 and len({pz[0][U], pz[1][U], 1}) == 3
    assert all(z[0] == 1 and z[U] == 1 and len(set(z[:U + 1])) > 2 for z in lz)
    assert np.array_equal(out["h"][0].cpu().numpy(), bytes_of(h, c.P, montgomery)), "h of circuit 0 is not the model's"
    # two of the extended columns against NR.forward at 2^13
    for name, i in (("advice", 0), ("perm_z", 1)):
        want = NR.forward(NR.inverse(lag[name][i], K, c.omega, 1, c.P), K + 3, c.cfg.omega_ext, c.cfg.zeta, c.P)
        assert want == cols[name][i]
        assert np.array_equal(out["ext"][name][0, i].cpu().numpy(), bytes_of(want, c.P, montgomery)), name


# ---- 3: a planar image with col_stride = 2^k * 32 is the Lagrange form of the advice columns -------------------------------------------------------
def test_a_planar_image_is_transformed_in_place(H):
    c = Chain(H, "bn254_fr", montgomery=True, planar=True)
    assert c.chip.col_stride == N_ROWS * 32 and c.chip.image_bytes(ROWS) == 5 * N_ROWS * 32
    out = c.run()
    assert out["lag"]["advice"].data_ptr() == out["image"].data_ptr()
    assert out["st_pz"] == [0] * B and out["st_lz"] == [0] * B
    assert_polynomial(out)


# ---- 4: the image at row 7 -----------------------------------------------------------------------------------------------------------------------------
def test_the_image_at_first_row_7(H):
    c = Chain(H, "pasta_fq", first_row=7)
    assert not any(any(col[:7]) for col in c.fixed[:9]) and any(col[7] for col in c.fixed[:9]) and c.fixed[QR.F_TABLE_TAG][1] == 1
    out = c.run()
    assert out["st_pz"] == [0] * B and out["st_lz"] == [0] * B
    assert_polynomial(out)
    adv = out["lag"]["advice"]
    assert not bool(adv[:, :, :7].any()) and not bool(adv[:, :, 7 + ROWS:U].any()) and bool(adv[:, :, 7].any())
    # ... and not with the key of an image at row 0: the fixed columns moved with the image
    c0 = Chain(H, "pasta_fq")
    c.fixed_dev, c.sigma_dev = c0.fixed_dev, c0.sigma_dev
    assert_no_polynomial(c.run(), range(B))


# ---- 5: faults on the device -----------------------------------------------------------------------------------------------------------------------------
def test_device_side_faults(H):
    from halo2_rsa_amd import _lib
    c = Chain(H, "bn254_fr")
    others = [0, 2]
    # one image cell that a copy pair names (the destination, on a row without a lookup), changed before the products
    row, col = next((r, q) for (r, q, _, _) in c.inside if c.kinds[r] == AR.ROW_MUL_ADD)
    out = c.run(image_fault=(1, row, col))
    assert out["st_pz"] == [0, _lib.H2R_E_ASSERTION, 0] and out["st_lz"] == [0] * B           # the product tells; its Z are written as computed
    assert_polynomial(out, others)
    assert_no_polynomial(out, [1])
    # one entry of the device's S'
    out = c.run(s_perm_fault=(1, 2, 300))
    assert out["st_pz"] == [0] * B and out["st_lz"] == [0] * B
    assert_polynomial(out, others)
    assert_no_polynomial(out, [1])
    # sets of 3 for the product, of 2 for the quotient: the configuration is the call's, so no circuit has a polynomial
    out = c.run(chunk_product=3)
    assert out["st_pz"] == [0] * B and out["st_lz"] == [0] * B
    assert_no_polynomial(out, range(B))
