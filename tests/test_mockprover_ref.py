"""CPU: the plain-Python MockProver of tests/mockprover_ref.py -- the model h2r_advice_check is compared with on the GPU -- on the images
tests/advice_ref.py restates from the oracle's streams: green on every satisfying assignment, exactly the one assert_one violation when
x >= n, the closed-form row counts, an incremental form that agrees with a full evaluation, and verdicts that depend on the seed alone."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import advice_ref as AR
import mockprover_ref as MP
from oracle_lib import FRESH_OPS, Oracle, fresh_op
from test_maingate_image_ref import FIELDS


def _mul_mod(w, L, field, seed):
    o = Oracle(w, L)
    rng = random.Random(seed)
    bits = w * L
    n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    a, b = rng.randrange(n), rng.randrange(n)
    rc, _, st = o.mul_mod(o.limbs(a), o.limbs(b), o.limbs(n))
    assert rc == 0
    la, lb, ln = ([int(x) for x in o.limbs(v)] for v in (a, b, n))
    return o, la, lb, ln, AR.mul_mod_image(o.p, la, lb, ln, st, FIELDS[field])


def _prover(im, w, L, field, rsa=False, **kw):
    g = MP.Geometry(w, L)
    return MP.MockProver(im.rows, im.kinds, g, FIELDS[field], cfg=AR.LookupConfig(AR.range_lens(w, L, rsa=rsa)), **kw)


@pytest.mark.parametrize("w,L,rows", [(64, 4, 250), (32, 8, 590), (64, 8, 590)])
def test_geometry_and_row_counts_are_the_closed_form(w, L, rows):
    """Geometry restates the oracle's carry geometry, and a mul_mod has the rows the closed form gives: 250 at (64, 4), 590 at L = 8."""
    o = Oracle(w, L)
    g = MP.Geometry(w, L)
    assert (g.carry_bits, g.carry_sub_bits, g.carry_nsub) == (o.p.carry_bits, o.p.carry_sub_bits, o.p.carry_nsub)
    assert MP.rows_per_mul_mod(L, g.carry_nrows) == rows
    _, _, _, _, im = _mul_mod(w, L, "bn254_fr", 5)
    assert len(im.rows) == rows


@pytest.mark.parametrize("w,L,field", [(64, 4, "bn254_fr"), (32, 8, "pasta_fq")])
def test_mul_mod_images_are_green(w, L, field):
    _, _, _, _, im = _mul_mod(w, L, field, 1000 * w + L)
    for rsa in (False, True):
        assert _prover(im, w, L, field, rsa=rsa).violations() == []
    assert MP.MockProver(im.rows, im.kinds, MP.Geometry(w, L), FIELDS[field], cfg=None).violations() == []      # no table: gates only


@pytest.mark.parametrize("w,L,field,case", [(64, 4, "bn254_fq", "lt"), (64, 4, "bn254_fq", "ge"), (64, 8, "pasta_fq", "eq"), (32, 16, "pasta_fp", "lt")])
def test_in_field_image_green_or_exactly_the_assert_one(w, L, field, case):
    """assert_in_field(x, n): green for x < n; with x >= n exactly one violation, the gate of the closing assert_one row."""
    o = Oracle(w, L)
    rng = random.Random(7 * w + L)
    bits = w * L
    n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    x = {"lt": rng.randrange(n), "ge": min(n + 3, (1 << bits) - 1), "eq": n}[case]
    _, _, st = o.assert_in_field(o.limbs(x), o.limbs(n))
    im = AR.in_field_image(o.p, [int(v) for v in o.limbs(x)], [int(v) for v in o.limbs(n)], st, FIELDS[field])
    assert _prover(im, w, L, field).violations() == ([] if x < n else [(len(im.rows) - 1, MP.GATE)])


@pytest.mark.parametrize("w,L,field", [(64, 4, "bn254_fr"), (32, 8, "pasta_fp")])
def test_fresh_family_images_are_green(w, L, field):
    o = Oracle(w, L)
    rng = random.Random(w + L)
    bits = w * L
    n = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    seen = set()
    for a, b in [(rng.randrange(n), rng.randrange(n)), (5, 5), (0, n - 1), (n - 1, 0)]:
        for name in FRESH_OPS:
            rc, _, _, st = fresh_op(o, name, o.limbs(a), o.limbs(b), o.limbs(n))
            if rc != 0:
                continue
            im = AR.fresh_image(o.p, name, o.limbs(a), None if name == "is_zero" else o.limbs(b),
                                o.limbs(n) if name in ("add_mod", "sub_mod") else None, st, FIELDS[field])
            assert _prover(im, w, L, field).violations() == [], name
            seen.add(name)
    assert seen == set(FRESH_OPS)


def test_row_order_of_the_codes():
    """Code 4 hides everything else of its row, code 5 hides lookup and gate, lookup and gate are each counted once per row, and a row
    that refers to a next row the image does not have is a gate violation."""
    w, L, field = 64, 4, "bn254_fr"
    P = FIELDS[field]
    _, _, _, _, im = _mul_mod(w, L, field, 3)
    g, cfg = MP.Geometry(w, L), AR.LookupConfig(AR.range_lens(w, L))
    r = im.kinds.index(AR.ROW_RANGE_LIMB)
    rows = [list(c) for c in im.rows]
    rows[r][0], rows[r][1] = 1 << 8, 1 << 70                  # two cells out of the 8-bit table, the composition broken too
    assert MP.MockProver(rows, im.kinds, g, P, cfg=cfg).violations() == [(r, MP.GATE), (r, MP.LOOKUP)]
    rows[r][3] = P                                            # ... and a non-canonical cell: only that is reported
    assert MP.MockProver(rows, im.kinds, g, P, cfg=cfg).violations() == [(r, MP.RANGE)]
    kinds = list(im.kinds)
    kinds[r] = 200                                            # ... on a kind without a fixed row: only that
    assert MP.MockProver(rows, kinds, g, P, cfg=cfg).violations() == [(r, MP.KIND)]
    assert MP.MockProver(im.rows[:r + 1], im.kinds[:r + 1], g, P, cfg=cfg).violations() == [(r, MP.GATE)]     # se_next on the last row
    # a table without the 8-bit range: the rows that look their cells up there have no fixed row
    v = MP.MockProver(im.rows, im.kinds, g, P, cfg=AR.LookupConfig([1])).violations()
    assert [row for row, _ in v] == [q for q, k in enumerate(im.kinds) if k >= AR.ROW_RANGE_LIMB] and {code for _, code in v} == {MP.KIND}


def _record_copies(w, L):
    from test_copymap_layout import _host_ctx
    from halo2_rsa_amd import _lib
    lib, ctx = _host_ctx(w, w * L)
    n = int(lib.h2r_advice_copy_map(ctx, None, 0))
    buf = (_lib.H2RCopy * n)()
    assert int(lib.h2r_advice_copy_map(ctx, buf, n)) == n
    lib.h2r_ctx_destroy(ctx)
    return [(c.row, c.col, c.src_row, c.src_col) for c in buf]


def test_copy_pairs_and_operands():
    """With the record's copy map and its operands the image stays green; a changed operand limb violates exactly the pairs that name
    it, a pair outside the image or a missing operand is a violation of its own."""
    w, L, field = 64, 4, "bn254_fr"
    _, a, b, n, im = _mul_mod(w, L, field, 11)
    copies = _record_copies(w, L)
    ops = {MP.COPY_SRC_A: a, MP.COPY_SRC_B: b, MP.COPY_SRC_N: n}
    assert _prover(im, w, L, field, copies=copies, operands=ops).violations() == []
    a2 = list(a)
    a2[2] ^= 1
    v = _prover(im, w, L, field, copies=copies, operands={**ops, MP.COPY_SRC_A: a2}).violations()
    named = sorted((c[0], MP.COPY) for c in copies if c[2] == MP.COPY_SRC_A and c[3] == 2)
    assert v == named and len(v) == L
    v = _prover(im, w, L, field, copies=copies, operands={MP.COPY_SRC_A: a, MP.COPY_SRC_B: b}).violations()
    assert len(v) == L * L and all(code == MP.COPY for _, code in v)
    assert _prover(im, w, L, field, copies=[(3, 0, len(im.rows), 0), (3, 5, 2, 0), (3, 0, 3, 0)]).violations() == [(3, MP.COPY)] * 2


def test_a_layout_moves_the_selectors_with_the_cells():
    w, L, field = 64, 4, "bn254_fr"
    _, a, b, n, im = _mul_mod(w, L, field, 12)
    layout = {AR.ROW_MUL_ADD: [2, 3, 0, 1, 4], AR.ROW_SUB: [1, 0, 2, 3, 4]}
    rows = [list(c) for c in im.rows]
    for r, k in enumerate(im.kinds):
        if k in layout:
            for q in range(5):
                rows[r][layout[k][q]] = im.rows[r][q]
    copies = _record_copies(w, L)
    ops = {MP.COPY_SRC_A: a, MP.COPY_SRC_B: b, MP.COPY_SRC_N: n}
    g, cfg, P = MP.Geometry(w, L), AR.LookupConfig(AR.range_lens(w, L)), FIELDS[field]
    assert MP.MockProver(rows, im.kinds, g, P, cfg=cfg, layout=layout, copies=copies, operands=ops).violations() == []
    assert MP.MockProver(rows, im.kinds, g, P, cfg=cfg, copies=copies, operands=ops).violations() != []       # ... and not without it


def _verdicts(seed):
    w, L, field = 64, 4, "bn254_fr"
    _, a, b, n, im = _mul_mod(w, L, field, seed)
    pr = _prover(im, w, L, field, copies=_record_copies(w, L), operands={MP.COPY_SRC_A: a, MP.COPY_SRC_B: b, MP.COPY_SRC_N: n})
    muts = MP.mutation_set(pr)
    return pr, muts, [pr.with_cell(r, c, v) if canonical else None for (r, c, v, canonical) in muts]


def test_mutation_verdicts_are_deterministic_and_incremental_equals_full():
    """The sweep's mutation set on the (64, 4) mul_mod image: the same seed gives the same mutants and the same verdicts, no mutant
    equals the value it replaces, and the incremental evaluation of a mutant is the full evaluation of the mutated image."""
    pr, muts, v1 = _verdicts(21)
    _, muts2, v2 = _verdicts(21)
    assert muts == muts2 and v1 == v2
    assert all(pr.rows[r][c] != v for (r, c, v, _) in muts)
    # the count, class by class: per cell v + 1, v - 1 and the two raw patterns; p - 1 unless v = 0 (then it is v - 1); on the a..d cells of
    # a lookup row 2^bits - 1, 2^bits and 2^64 unless already listed; on column a of an overflow row its two boundaries likewise
    want = 0
    for cells, kind in zip(pr.rows, pr.kinds):
        _, comp, ov = pr._kind_row(kind)
        for c, v in enumerate(cells):
            vals = {(v + 1) % pr.P, (v - 1) % pr.P, pr.P - 1}
            if comp and c < 4:
                vals |= {(1 << comp) - 1, 1 << comp, 1 << 64}
            if ov and c == 0:
                vals |= {(1 << ov) - 1, 1 << ov}
            want += len(vals - {v}) + 2
    assert len(muts) == want == 6049
    assert sum(1 for m in muts if not m[3]) == 2 * 5 * len(pr.rows)
    rng = random.Random(1)
    for i in rng.sample(range(len(muts)), 300):
        r, c, v, canonical = muts[i]
        if not canonical:
            continue
        rows = [list(x) for x in pr.rows]
        rows[r][c] = v
        full = MP.MockProver(rows, pr.kinds, pr.g, pr.P, cfg=pr.cfg, copies=pr.copies, operands=pr.operands).violations()
        assert full == v1[i], (r, c, v)
    assert pr.violations() == []                              # with_cell leaves the image as it was
    # ... also on an image that is not green to begin with (a kind without a fixed row, an operand that is not given)
    kinds = list(pr.kinds)
    kinds[40] = 200
    ops = {k: v for k, v in pr.operands.items() if k != MP.COPY_SRC_B}
    red = MP.MockProver(pr.rows, kinds, pr.g, pr.P, cfg=pr.cfg, copies=pr.copies, operands=ops)
    assert len(red.violations()) == 1 + 4 * 4
    for i in rng.sample(range(len(muts)), 200):
        r, c, v, canonical = muts[i]
        rows = [list(x) for x in pr.rows]
        rows[r][c] = v
        assert red.with_cell(r, c, v) == MP.MockProver(rows, kinds, pr.g, pr.P, cfg=pr.cfg, copies=pr.copies, operands=ops).violations(), (r, c, v)


def test_cells_the_record_copy_map_leaves_free():
    """Gate, lookup and the record's copy pairs together: the only cells of a mul_mod record a prover could change unnoticed hold 0 in
    the good image (padding), or are the inverse witness of an is_zero whose input is 0."""
    w, L, field = 64, 4, "bn254_fr"
    _, a, b, n, im = _mul_mod(w, L, field, 21)
    pr = _prover(im, w, L, field, copies=_record_copies(w, L), operands={MP.COPY_SRC_A: a, MP.COPY_SRC_B: b, MP.COPY_SRC_N: n})
    nonzero = {cls for cls, cells in MP.unseen_cells(pr).items() if any(v for _, v in cells)}
    assert nonzero <= {(AR.ROW_ISZERO_INV, 1)}, nonzero


def test_pow_copy_map_on_the_restated_pow_element():
    """A fixed-exponent pow element (e = 3: sq(x, x), mul(1, x), sq(r0, r0), mul(r1, r0)) restated record by record from the oracle, under
    h2r_pow_copy_map on a host context: green with the operands x and n, 2 + 4 * 250 rows, and the same free cells as one record."""
    from test_copymap_layout import _host_ctx
    from halo2_rsa_amd import _lib
    w, L, field, e = 64, 4, "bn254_fr", 3
    P = FIELDS[field]
    o = Oracle(w, L)
    rng = random.Random(33)
    N = rng.getrandbits(256) | (1 << 255) | 1
    X = rng.randrange(N)
    lib, ctx = _host_ctx(w, w * L)
    pl = _lib.H2RPowLayout()
    eb = bytes([e])
    assert lib.h2r_pow_fixed_layout(ctx, eb, 1, ctypes.byref(pl)) == 0 and pl.num_mul_mods == 4
    a_src, b_src = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    assert lib.h2r_pow_operand_sources(ctx, ctypes.byref(pl), eb, 1, a_src, b_src) == 0
    n_pairs = int(lib.h2r_pow_copy_map(ctx, ctypes.byref(pl), eb, 1, 0, None, 0))
    buf = (_lib.H2RCopy * n_pairs)()
    assert int(lib.h2r_pow_copy_map(ctx, ctypes.byref(pl), eb, 1, 0, buf, n_pairs)) == n_pairs
    lib.h2r_ctx_destroy(ctx)
    im = AR.Image(w, L, P)
    im.assign_constant(1)
    im.assign_constant(0)
    results = []
    value = {_lib.H2R_SRC_X: X, _lib.H2R_SRC_ONE: 1}
    for t in range(4):
        a, b = (value[s] if s < 0 else results[s] for s in (a_src[t], b_src[t]))
        rc, r, st = o.mul_mod(o.limbs(a), o.limbs(b), o.limbs(N))
        assert rc == 0
        rec = AR.mul_mod_image(o.p, [int(v) for v in o.limbs(a)], [int(v) for v in o.limbs(b)], [int(v) for v in o.limbs(N)], st, P)
        im.rows += rec.rows
        im.kinds += rec.kinds
        results.append(o.to_int(r))
    assert results[-1] == pow(X, e, N) and len(im.rows) == 2 + 4 * 250
    ops = {MP.COPY_SRC_A: [int(v) for v in o.limbs(X)], MP.COPY_SRC_N: [int(v) for v in o.limbs(N)]}
    pr = _prover(im, w, L, field, copies=[(c.row, c.col, c.src_row, c.src_col) for c in buf], operands=ops)
    assert pr.violations() == []
    nonzero = {cls for cls, cells in MP.unseen_cells(pr).items() if any(v for _, v in cells)}
    assert nonzero == {(AR.ROW_ISZERO_INV, 1)}, nonzero
