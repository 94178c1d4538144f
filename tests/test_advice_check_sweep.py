"""h2r_advice_check against a plain model, cell by cell (the differential sweep).

For an image the library's own emitters wrote, EVERY cell is replaced in turn by every value of tests/mockprover_ref.mutation_set
(v + 1, v - 1, p - 1; the lookup boundaries 2^bits - 1, 2^bits, 2^64 on lookup rows; the raw patterns p and 2^256 - 1), one mutant per
batch element, and the device's verdict -- the COUNT of violated checks and the (row, code) it names -- is compared with the
plain-Python MockProver of tests/mockprover_ref.py for every mutant: equal counts for canonical mutants, bad >= 1 for raw patterns.
In every chunk element 0 is the untouched image (stays green) and the last element is a mutant with a nonzero status byte (skipped).

Images: A fixed-exponent pow (copy map, operands, both limb widths, both representations, no table, a custom layout, a kind without a
fixed row), B variable-exponent pow (to_bits, BITS_COMPOSE*, SELECT), C the Fresh family, D the rows of a verify element outside its
pow section (CONST_EM, RANGE_U32 under RangeChip's 4-bit table), E the hashed-message rows (CONST_COEFF8)."""
import ctypes
import os
import random
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import advice_ref as AR
import mockprover_ref as MP

R256 = 1 << 256
CHUNK_BYTES = 448 << 20            # a chunk of mutants stays below about 512 MB
MUL_ADD, SUB = 6, 8


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


def _pow_kinds(chip, pl):
    from halo2_rsa_amd._lib import lib
    n = int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl)))
    k = np.zeros(n, dtype=np.uint8)
    assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k.ctypes.data) == 0
    return k


def _cell_off(chip, rows, r, c):
    return c * rows * 32 + r * 32 if chip.columns else r * 160 + c * 32


def decode(chip, elem_host, rows, P):
    """One element's image bytes -> [[5 canonical integers]] (a Montgomery ctx: divided by R)."""
    a = np.ascontiguousarray(elem_host, dtype=np.uint8)
    a = a.reshape(5, rows, 32).transpose(1, 0, 2) if chip.columns else a.reshape(rows, 5, 32)
    rinv = pow(R256, -1, P)
    out = []
    for r in range(rows):
        cells = [int.from_bytes(a[r, c].tobytes(), "little") for c in range(5)]
        assert all(v < P for v in cells), ("the emitter wrote a non-canonical cell", r)
        out.append([v * rinv % P for v in cells] if chip.montgomery else cells)
    return out


def _cfg(chip, rsa_chip):
    return AR.LookupConfig(AR.range_lens(chip.limb_width, chip.num_limbs, rsa=rsa_chip))


def _copies_host(copies):
    return np.frombuffer(copies, dtype=np.uint32).reshape(-1, 4).copy()


def sweep(H, label, chip, kinds, good, prover, lookup=None, copies=None, src_a=None, src_n=None, layout=None, only_rows=None):
    """good: uint8 device tensor, ONE element's image; prover: the model of that image (same table, layout, copies, operands).
    copies: uint32 host array [n, 4]; src_a / src_n: [1, L] device limbs.  Returns {(kind, logical column): [(row, good value)]} of the
    cells with a canonical mutant nobody flags (for the completeness check)."""
    t0 = time.perf_counter()
    P, rows, ib = prover.P, len(prover.rows), good.numel()
    assert ib == chip.image_bytes(rows)
    base = prover.violations()
    muts = [m for m in MP.mutation_set(prover) if only_rows is None or m[0] in only_rows]
    verdicts = [prover.with_cell(r, c, v) if canonical else None for (r, c, v, canonical) in muts]
    t_model = time.perf_counter() - t0
    t_dev = 0.0
    kd = torch.from_numpy(np.ascontiguousarray(kinds, dtype=np.uint8)).cuda()
    cd = torch.from_numpy(copies.view(np.int32)).cuda() if copies is not None else None
    per = max(1, CHUNK_BYTES // ib - 2)
    lane = np.arange(32, dtype=np.int64)
    mism, n_chunks = [], 0
    for lo in range(0, len(muts), per):
        chunk, cv = muts[lo:lo + per], verdicts[lo:lo + per]
        n = len(chunk)
        skip = next(i for i in range(n) if cv[i] is None or cv[i])      # the skipped element carries a mutation somebody would flag
        vals = np.zeros((n + 1, 32), dtype=np.uint8)
        offs = np.zeros(n + 1, dtype=np.int64)
        for i, (r, c, v, canonical) in enumerate(chunk + [chunk[skip]]):
            stored = v * R256 % P if (canonical and chip.montgomery) else v
            vals[i] = np.frombuffer(stored.to_bytes(32, "little"), dtype=np.uint8)
            offs[i] = (i + 1) * ib + _cell_off(chip, rows, r, c)
        t1 = time.perf_counter()
        buf = good.reshape(1, ib).repeat(n + 2, 1)
        idx = torch.from_numpy((offs[:, None] + lane[None, :]).reshape(-1)).cuda()
        buf.view(-1)[idx] = torch.from_numpy(vals.reshape(-1)).cuda()                       # one indexed store
        status = torch.zeros(n + 2, dtype=torch.uint8, device="cuda")
        status[n + 1] = 7
        sa = H.AssignedInteger(src_a.repeat(n + 2, 1).contiguous(), chip.limb_width) if src_a is not None else None
        sn = H.AssignedInteger(src_n, chip.limb_width) if src_n is not None else None
        bad, first = chip.advice_check(kd, buf, n + 2, status=status, copies=cd, src_a=sa, src_n=sn, lookup=lookup, layout=layout)
        bad, first = bad.cpu().tolist(), first.cpu().tolist()
        t_dev += time.perf_counter() - t1
        n_chunks += 1
        exp0 = (len(base), {(r << 8) | code for r, code in base} or {0})
        assert bad[0] == exp0[0] and first[0] in exp0[1], (label, "the untouched image", bad[0], hex(first[0]), base[:4])
        assert bad[n + 1] == 0 and first[n + 1] == 0, (label, "a skipped element was checked", bad[n + 1], hex(first[n + 1]))
        for i, ((r, c, v, canonical), want) in enumerate(zip(chunk, cv)):
            b, f = bad[i + 1], first[i + 1]
            if canonical:
                ok = b == len(want) and (f in {(q << 8) | code for q, code in want} if want else f == 0)
            else:
                ok = b >= 1 and ((f & 0xff) != MP.RANGE or (f >> 8) == r)
            if not ok:
                mism.append(dict(row=r, col=c, kind=prover.kinds[r], good=prover.rows[r][c], value=hex(v), canonical=canonical, bad=b,
                                 first=(f >> 8, f & 0xff), model=want))
        del buf, idx
    dt = time.perf_counter() - t0
    print("SWEEP %-44s rows %5d  mutants %6d  chunks %3d  %.3f s (model %.3f s, device: clone + scatter + check + read back %.3f s)" %
          (label, rows, len(muts), n_chunks, dt, t_model, t_dev))
    assert not mism, (label, len(mism), mism[:8])
    return MP.unseen_cells(prover, muts, verdicts)


# ------------------------------------------------------------------------------------------------------------------------------
# A. fixed-exponent pow, e = 3 (four records), with h2r_pow_copy_map and the operands
_A = {}


def _pow_image(H, w, field, repr_kw):
    """(chip, kinds, image [1, ib], rows of the model, copies, x limbs, n limbs, X, N) -- one element, built once per (w, field, repr)."""
    key = (w, field, tuple(sorted(repr_kw.items())))
    if key not in _A:
        chip = H.BigIntChip(w, 256, field, **repr_kw)
        rng = random.Random(100 + w)
        N = rand_modulus(rng, 256)
        X = rng.randrange(N)
        x, n = chip.assign_integer([X]), chip.assign_integer([N])
        res = chip.pow_mod_fixed_exp(x, 3, n)
        pl = res.trace.pow_layout
        assert pl.num_mul_mods == 4
        kinds = _pow_kinds(chip, pl)
        img = res.emit_advice(direct=True)
        torch.cuda.synchronize()
        assert int(res.status.max().item()) == 0
        L = chip.num_limbs
        assert len(kinds) == 2 + 4 * MP.rows_per_mul_mod(L, MP.Geometry(w, L).carry_nrows)
        m = (1 << w) - 1
        _A[key] = dict(chip=chip, kinds=kinds, img=img, copies=_copies_host(chip.pow_copy_map(pl, 3)), x=x, n=n,
                       xl=[(X >> (w * i)) & m for i in range(L)], nl=[(N >> (w * i)) & m for i in range(L)])
    return _A[key]


# The cells of a fixed-exponent pow element that a prover could change without any check noticing, by (kind, logical column): every
# other cell whose mutant goes unnoticed must hold 0 in the good image (the padding of a row shape: an unused column is unconstrained).
FREE_CELLS = {
    (AR.ROW_ISZERO_INV, 1): "is_zero's inverse witness a' when a = 0: a * a' + r - 1 = 0 holds for every a' (maingate leaves it free too)",
}


@pytest.mark.parametrize("w,field,repr_kw,variant", [
    (64, "bn254_fr", dict(), "plain"), (64, "bn254_fr", dict(columns=True, montgomery=True), "plain"),
    (32, "pasta_fq", dict(), "plain"), (32, "pasta_fq", dict(columns=True, montgomery=True), "plain"),
    (64, "bn254_fr", dict(), "no_table"), (64, "bn254_fr", dict(), "layout"), (64, "bn254_fr", dict(), "kind200")],
    ids=["64x4", "64x4-columns-montgomery", "32x8", "32x8-columns-montgomery", "64x4-no-table", "64x4-custom-layout", "64x4-kind-200"])
def test_pow_fixed_every_cell(H, w, field, repr_kw, variant):
    """Every cell of a pow_mod_fixed_exp element (e = 3): 1,002 rows at 64 x 4, 2,362 rows at 32 x 8 (4-bit sub-limbs, another overflow
    length); with lookup = None the model has no lookups; under a custom layout (MUL_ADD -> [2, 3, 0, 1, 4], SUB -> [1, 0, 2, 3, 4]) the
    image is permuted by h2r_advice_apply_layout and the model gets the same table; with one kind byte 200 every element reports one code 4
    on that row.  The plain runs also pin the copy map's completeness: a cell nobody watches holds 0 or is listed in FREE_CELLS."""
    from halo2_rsa_amd import _lib
    from halo2_rsa_amd._lib import lib
    A = _pow_image(H, w, field, repr_kw)
    chip, kinds, P = A["chip"], A["kinds"], _P(field)
    g = MP.Geometry(w, chip.num_limbs)
    assert (g.carry_bits, g.carry_sub_bits, g.carry_nsub) == (chip.layout.carry_bits, chip.layout.carry_sub_bits, chip.layout.carry_nsub)
    look = None if variant == "no_table" else H.LookupArgument(chip, rsa_chip=False)
    cfg = None if variant == "no_table" else _cfg(chip, False)
    img, lay, layout = A["img"], None, None
    if variant == "layout":
        layout = {MUL_ADD: [2, 3, 0, 1, 4], SUB: [1, 0, 2, 3, 4]}
        lay = _lib.H2RAdviceLayout()
        ks = (ctypes.c_uint8 * 2)(MUL_ADD, SUB)
        cols = ((ctypes.c_uint8 * 5) * 2)(tuple(layout[MUL_ADD]), tuple(layout[SUB]))
        assert lib().h2r_advice_layout_custom(chip._ctx, ks, cols, 2, ctypes.byref(lay)) == 0
        img = img.clone()
        kd = torch.from_numpy(kinds).cuda()
        assert lib().h2r_advice_apply_layout(chip._ctx, ctypes.byref(lay), kd.data_ptr(), len(kinds), img.data_ptr(), img.shape[1], 1, None,
                                             chip._stream()) == 0
    if variant == "kind200":
        kinds = kinds.copy()
        kinds[int(np.flatnonzero(kinds == MUL_ADD)[3])] = 200
    torch.cuda.synchronize()
    rows = decode(chip, img[0].cpu().numpy(), len(kinds), P)
    prover = MP.MockProver(rows, kinds, g, P, cfg=cfg, layout=layout, copies=A["copies"].tolist(),
                           operands={MP.COPY_SRC_A: A["xl"], MP.COPY_SRC_N: A["nl"]})
    base = prover.violations()
    assert base == ([(int(np.flatnonzero(kinds == 200)[0]), MP.KIND)] if variant == "kind200" else []), base[:5]
    unseen = sweep(H, "A pow e=3 %dx%d %s %s" % (w, chip.num_limbs, "col+mont" if repr_kw else "default", variant), chip, kinds, img[0],
                   prover, lookup=look, copies=A["copies"], src_a=A["x"].limbs_dev, src_n=A["n"].limbs_dev, layout=lay)
    if variant == "plain":
        holes = {cls: sorted(cells)[:3] for cls, cells in unseen.items() if cls not in FREE_CELLS and any(v for _, v in cells)}
        assert not holes, ("cells no gate, lookup or copy pair watches", holes)
        assert all(cls in unseen for cls in FREE_CELLS)


@pytest.mark.parametrize("which", ["src_a", "src_n"])
def test_pow_fixed_operand_limb_changed(H, which):
    """The operand side of the copy pairs: one limb of src_a (then of src_n) changed for one element -- the count is the number of pairs
    that name that limb, the neighbour stays green."""
    A = _pow_image(H, 64, "bn254_fr", dict())
    chip, kinds = A["chip"], A["kinds"]
    look = H.LookupArgument(chip, rsa_chip=False)
    src_code = MP.COPY_SRC_A if which == "src_a" else MP.COPY_SRC_N
    limb = 2
    named = sorted(int(c[0]) for c in A["copies"] if c[2] == src_code and c[3] == limb)
    assert len(named) >= 4
    img = A["img"].repeat(3, 1)
    ops = {"src_a": A["x"].limbs_dev.repeat(3, 1).contiguous(), "src_n": A["n"].limbs_dev.repeat(3, 1).contiguous()}
    ops[which][1, limb] ^= 1
    cd = torch.from_numpy(A["copies"].view(np.int32)).cuda()
    bad, first = chip.advice_check(kinds, img, 3, copies=cd, src_a=H.AssignedInteger(ops["src_a"], 64), src_n=H.AssignedInteger(ops["src_n"], 64),
                                   lookup=look)
    bad, first = bad.cpu().tolist(), first.cpu().tolist()
    # the model with the same changed operand
    P = _P("bn254_fr")
    rows = decode(chip, A["img"][0].cpu().numpy(), len(kinds), P)
    xl, nl = list(A["xl"]), list(A["nl"])
    (xl if which == "src_a" else nl)[limb] ^= 1
    want = MP.MockProver(rows, kinds, MP.Geometry(64, 4), P, cfg=_cfg(chip, False), copies=A["copies"].tolist(),
                         operands={MP.COPY_SRC_A: xl, MP.COPY_SRC_N: nl}).violations()
    assert want == [(r, MP.COPY) for r in named]
    assert bad == [0, len(named), 0] and first[0] == 0 and first[2] == 0, (bad, named)
    assert (first[1] >> 8, first[1] & 0xff) in want


# ------------------------------------------------------------------------------------------------------------------------------
# B. variable-exponent pow: to_bits, BITS_COMPOSE*, SELECT (no copy map for this arm)
@pytest.mark.parametrize("e", [3, 0])
def test_pow_var_every_cell(H, e):
    chip = H.BigIntChip(64, 256)
    P = _P("bn254_fr")
    rng = random.Random(40 + e)
    N = rand_modulus(rng, 256)
    X = rng.randrange(N)
    x, n = chip.assign_integer([X]), chip.assign_integer([N])
    ev = H.AssignedInteger(torch.tensor([[e]], dtype=torch.int64, device="cuda"), 64)
    res = chip.pow_mod(x, ev, n, 2)
    kinds = _pow_kinds(chip, res.trace.pow_layout)
    img = res.emit_advice(direct=True)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) == 0 and res.value.to_big_uint() == [pow(X, e, N)]
    assert len(kinds) == (2 + 1 + 1) + 2 + 2 * (2 * 250 + 4)
    assert {AR.ROW_SELECT, AR.ROW_BITS_COMPOSE_LAST + 1} <= set(kinds.tolist())
    prover = MP.MockProver(decode(chip, img[0].cpu().numpy(), len(kinds), P), kinds, MP.Geometry(64, 4), P, cfg=_cfg(chip, False))
    assert prover.violations() == []
    sweep(H, "B pow_mod var e=%d 64x4" % e, chip, kinds, img[0], prover, lookup=H.LookupArgument(chip, rsa_chip=False))


# ------------------------------------------------------------------------------------------------------------------------------
# C. the Fresh family at 64 x 4 (no copies)
_FLAG_OPS = ["is_zero", "is_equal_fresh", "is_less_than", "is_less_than_or_equal", "is_greater_than", "is_greater_than_or_equal", "is_in_field"]
_FRESH_CASES = [(name, False) for name in ["add", "sub", "add_mod", "sub_mod"] + _FLAG_OPS] + [(name, True) for name in _FLAG_OPS]


@pytest.mark.parametrize("name,assert_one", _FRESH_CASES, ids=["%s%s" % (nm, "-assert_one" if ao else "") for nm, ao in _FRESH_CASES])
def test_fresh_family_every_cell(H, name, assert_one):
    """Every op h2r_fresh_op_emit_advice supports; the flag ops once more with H2R_ADVICE_ASSERT_ONE (operands that make the flag 1)."""
    chip = H.BigIntChip(64, 256)
    P = _P("bn254_fr")
    rng = random.Random(len(name))
    N = rand_modulus(rng, 256)
    lo, hi = sorted([rng.randrange(N), rng.randrange(N)])
    a, b = {"is_zero": (0, 0), "is_equal_fresh": (lo, lo), "is_greater_than": (hi, lo), "is_greater_than_or_equal": (hi, lo)}.get(name, (lo, hi)) \
        if assert_one else ((hi, lo) if name in ("sub", "sub_mod", "is_less_than") else (lo, hi))
    A, B, Nn = chip.assign_integer([a]), chip.assign_integer([b]), chip.assign_integer([N])
    res = chip._fresh_op(name, A, None if name == "is_zero" else B, Nn if name in ("add_mod", "sub_mod") else None)
    img = res.emit_advice(assert_one=assert_one)
    kinds = chip.fresh_op_row_kinds(res.op, assert_one)
    torch.cuda.synchronize()
    assert int(res.status.max().item()) == 0 and (not assert_one or int(res.flag[0].item()) == 1)
    prover = MP.MockProver(decode(chip, img[0].cpu().numpy(), len(kinds), P), kinds, MP.Geometry(64, 4), P, cfg=_cfg(chip, False))
    assert prover.violations() == []
    sweep(H, "C fresh %s%s 64x4" % (name, " assert_one" if assert_one else ""), chip, kinds, img[0], prover,
          lookup=H.LookupArgument(chip, rsa_chip=False))


# ------------------------------------------------------------------------------------------------------------------------------
# D. a verify element at the smallest RSAChip shape: RSAChip(768, 5), L = 12 (verify_layout needs 64-bit limbs, L >= 9, L % 4 == 0)
def _is_prime(n, rng):
    if n % 2 == 0 or any(n % q == 0 for q in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
        return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(24):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def _rsa768_e3(rng):
    """(n, d) of an RSA-768 key with public exponent 3 (both primes = 2 mod 3)."""
    ps = []
    while len(ps) < 2:
        c = rng.getrandbits(384) | (3 << 382) | 1
        if c % 3 == 2 and _is_prime(c, rng):
            ps.append(c)
    p, q = ps
    return p * q, pow(3, -1, (p - 1) * (q - 1))


def _encoded_message(hashed, L):
    """The PKCS#1 v1.5 encoded message the chip compares with, as the integer of its 64-bit limbs (src/chip.rs:138-198, advice_ref.em_image)."""
    limbs = [(hashed >> (64 * i)) & (2 ** 64 - 1) for i in range(4)] + [AR.EM_CONSTS[0], AR.EM_CONSTS[1], (AR.EM_CONSTS[4] << 32) | AR.EM_CONSTS[3]]
    limbs += [2 ** 64 - 1] * (L - 1 - 7) + [AR.EM_CONSTS[5]]
    return sum(v << (64 * i) for i, v in enumerate(limbs))


@pytest.mark.parametrize("elem", [0, 1], ids=["valid", "message-differs"])
def test_verify_element_rows_outside_the_pow_section(H, elem):
    """is_eq's seed, assert_in_field, the encoded-message check (CONST_EM + j, both RANGE_U32 decompositions under RangeChip's 4-bit table)
    and the two boundary rows of the pow section; e = 3; one valid element, one whose encoded message differs (is_valid = 0, every gate
    still satisfied).  The pow rows in between are image A's business -- the model still holds them (and their copy pairs)."""
    rsa = H.RSAChip(768, 5)
    chip = rsa.bigint_chip()
    L, P = 12, _P("bn254_fr")
    rng = random.Random(768)
    n, d = _rsa768_e3(rng)
    hashed = [rng.getrandbits(256), rng.getrandbits(256)]
    sig = pow(_encoded_message(hashed[0], L), d, n)
    pk = rsa.assign_public_key(H.RSAPublicKey(H.UnassignedInteger.from_ints([n, n], L, 64), H.Fix(3)))
    sg = rsa.assign_signature(H.RSASignature(H.UnassignedInteger.from_ints([sig, sig], L, 64)))
    res = rsa.verify_pkcs1v15_signature(pk, hashed, sg)
    kinds = res.row_kinds()
    total, sec = res.advice_sections()
    img = res.emit_advice(direct=True)
    torch.cuda.synchronize()
    assert res.is_valid.cpu().tolist() == [1, 0] and res.status.cpu().tolist() == [0, 0]
    assert total == len(kinds) == sum(sec) and sec[0] == 1
    assert {AR.ROW_CONST_EM + j for j in range(6)} | {AR.ROW_RANGE_U32, AR.ROW_RANGE_U32 + 1} <= set(kinds[sec[0] + sec[1] + sec[2]:].tolist())
    copies = _copies_host(chip.pow_copy_map(res.layout.pow, 3, row_offset=sec[0] + sec[1]))
    m = 2 ** 64 - 1
    prover = MP.MockProver(decode(chip, img[elem].cpu().numpy(), total, P), kinds, MP.Geometry(64, L), P, cfg=_cfg(chip, True), copies=copies.tolist(),
                           operands={MP.COPY_SRC_A: [(sig >> (64 * i)) & m for i in range(L)], MP.COPY_SRC_N: [(n >> (64 * i)) & m for i in range(L)]})
    assert prover.violations() == []
    pow_lo, pow_hi = sec[0] + sec[1], sec[0] + sec[1] + sec[2]
    only = set(range(0, pow_lo + 1)) | set(range(pow_hi - 1, total))
    sweep(H, "D verify 768 e=3 %s" % ("valid" if elem == 0 else "message differs"), chip, kinds, img[elem], prover,
          lookup=H.LookupArgument(chip, rsa_chip=True), copies=copies, src_a=sg.c.limbs_dev[elem:elem + 1], src_n=pk.n.limbs_dev[elem:elem + 1], only_rows=only)


# ------------------------------------------------------------------------------------------------------------------------------
# E. the hashed-message rows (CONST_COEFF8 + j)
def test_hashed_msg_rows_every_cell(H):
    from halo2_rsa_amd._lib import lib
    chip = H.BigIntChip(64, 256)
    P = _P("bn254_fr")
    _, _, hm = H.sha256_hashed_msg(chip, [b"hello world"])
    rows = int(lib().h2r_hashed_msg_advice_rows(chip._ctx))
    kinds = np.zeros(rows, dtype=np.uint8)
    assert rows == 68 and lib().h2r_hashed_msg_row_kinds(chip._ctx, kinds.ctypes.data) == 0
    assert {AR.ROW_CONST_COEFF8 + j for j in range(8)} <= set(kinds.tolist())
    img = torch.empty((1, chip.image_bytes(rows)), dtype=torch.uint8, device="cuda")
    assert lib().h2r_hashed_msg_emit_advice(chip._ctx, hm.data_ptr(), hm.shape[1], 1, None, img.data_ptr(), img.shape[1], chip._stream()) == 0
    torch.cuda.synchronize()
    prover = MP.MockProver(decode(chip, img[0].cpu().numpy(), rows, P), kinds, MP.Geometry(64, 4), P, cfg=_cfg(chip, False))
    assert prover.violations() == []
    sweep(H, "E hashed-message rows", chip, kinds, img[0], prover, lookup=H.LookupArgument(chip, rsa_chip=False))


# ------------------------------------------------------------------------------------------------------------------------------
def test_image_that_ends_on_a_row_with_se_next(H):
    """An image cut after the FIRST row of a decomposition: its last row refers to a next row the image does not have -- one gate
    violation on the good cells already -- and still has its lookup: a sub-limb pushed out of the table counts 2 on that row."""
    chip = H.BigIntChip(64, 256)
    P = _P("bn254_fr")
    A, B = chip.assign_integer([12345 << 70]), chip.assign_integer([987 << 130])
    res = chip._fresh_op("add", A, B, None)
    img = res.emit_advice()
    kinds = chip.fresh_op_row_kinds(res.op)
    torch.cuda.synchronize()
    r = int(np.flatnonzero(kinds == AR.ROW_RANGE_LIMB)[0])
    kinds = kinds[:r + 1]
    cut = img[0, :(r + 1) * 160].contiguous()
    prover = MP.MockProver(decode(chip, cut.cpu().numpy(), r + 1, P), kinds, MP.Geometry(64, 4), P, cfg=_cfg(chip, False))
    assert prover.violations() == [(r, MP.GATE)]
    assert prover.with_cell(r, 0, 1 << 8) == [(r, MP.GATE), (r, MP.LOOKUP)]
    sweep(H, "an image cut after a decomposition's first row", chip, kinds, cut, prover, lookup=H.LookupArgument(chip, rsa_chip=False))
