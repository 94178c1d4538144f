"""TEST HELPER: a plain-Python MockProver for an advice image -- what halo2's `MockProver::verify` checks of these rows (gate, lookup,
permutation), on Python integers.  The model h2r_advice_check (advice_check_rows_kernel / advice_check_copies_kernel) is compared with,
cell by cell, in tests/test_advice_check_sweep.py.

Independent of the library: the selectors come from tests/advice_ref.py (fixed_row / fixed_row_bits_compose), the lookup from
LookupConfig.table(), the set of kinds that HAVE a fixed row from the row tables of DESIGN.md section 2b restated in valid_kind();
neither h2r_advice_fixed_row nor the library's per-kind table is read.

Semantics (the ones documented at h2r_advice_check in include/h2r.h).  Per row, in this order:
  * a kind without a fixed row: one violation, code 4, and nothing else for the row;
  * otherwise any of the row's five cells >= p: one violation, code 5, and nothing else for the row;
  * otherwise one code 2 if the composition lookup fails on any of a..d or the overflow lookup fails on a (at most one per row), and
    one code 1 if the gate residual is nonzero (e_next = column e of the next row; a row with se_next != 0 that is the image's last
    row is a gate violation).
Per copy pair: one code 3 if the pair names a row or column outside the image, if its two cells differ, or -- H2R_COPY_SRC_* -- if
the cell is not the operand limb (or the operand is not given).  A violation is (row, code); a pair reports its own (destination) row.

`rows` are the image as it lies: PHYSICAL columns.  `layout` = {kind: [physical column of logical cell a..e]} moves the selectors with
the cells, as the gate of a re-pinned row shape would be configured; the lookups read the physical columns 0..3 / 0 and se_next the
physical column 4 of the next row (halo2 queries columns, not logical cells -- a layout has to keep a and e of a decompose row in place)."""
import advice_ref as AR

GATE, LOOKUP, COPY, KIND, RANGE = 1, 2, 3, 4, 5
COPY_SRC_BASE = 0xFFFFFF00          # H2R_COPY_SRC_A / _B / _N = base + 1 / 2 / 3
COPY_SRC_A, COPY_SRC_B, COPY_SRC_N = COPY_SRC_BASE + 1, COPY_SRC_BASE + 2, COPY_SRC_BASE + 3
_SEL = ("sa", "sb", "sc", "sd", "se")
_ALL_LENS = AR.LookupConfig(range(1, 65))       # stands in for "no table": every tag is looked up, then dropped


class Geometry:
    """(w, L) and the carry geometry of is_equal_muled's range assigns (big_integer/chip.rs:1220-1249, restated)."""

    def __init__(self, w, L):
        self.w, self.L = w, L
        wm = AR.word_max(w, L)
        self.carry_bits = (2 * wm).bit_length() - w
        self.carry_sub_bits = max(1, self.carry_bits // 8)
        self.carry_nsub = -(-self.carry_bits // self.carry_sub_bits)
        self.limb_nrows = 2                                   # eight sub-limbs of w / 8 bits
        self.carry_nrows = (self.carry_nsub + 3) // 4


def rows_per_mul_mod(L, carry_nrows):
    """The closed form of one mul_mod's rows."""
    C = 2 * L - 1
    return 4 * L + 2 * (C + L * L) + L + 4 + (C - 1) * (23 + carry_nrows) + 23 + 1


def valid_kind(kind, g):
    """Does the kind have a fixed row?  (H2R_ROW_* of include/h2r.h.)  Restated, and pinned against the library only as far as the sweep's
    images reach: the kinds that occur in them (valid), kind 200 and a limb row under a table without its bit length (invalid).  The gaps
    of 0..25 are taken wholesale, and RANGE_U32 without a table counts as valid here; no image tries either arm on the device."""
    if 0 <= kind <= 25:                                       # the main-gate ops, CONST_EM + 0..5
        return True
    if AR.ROW_RANGE_LIMB <= kind < AR.ROW_RANGE_LIMB + g.limb_nrows or AR.ROW_RANGE_CARRY <= kind < AR.ROW_RANGE_CARRY + g.carry_nrows:
        return True
    if kind in (AR.ROW_RANGE_U32, AR.ROW_RANGE_U32 + 1) or AR.ROW_CONST_COEFF8 <= kind < AR.ROW_CONST_COEFF8 + 8:
        return True
    return AR.ROW_BITS_COMPOSE <= kind < AR.ROW_BITS_COMPOSE_LAST + 64


class MockProver:
    def __init__(self, rows, kinds, geometry, P, cfg=None, layout=None, copies=None, operands=None):
        """rows: [[5 integers]] (canonical values the cells stand for, or anything >= p for a non-canonical cell); kinds: one per row;
        cfg: AR.LookupConfig or None (no lookups); layout: {kind: [5 physical columns]}; copies: [(row, col, src_row, src_col)] with
        LOGICAL columns; operands: {COPY_SRC_A: limbs, COPY_SRC_B: limbs, COPY_SRC_N: limbs} (missing = not given)."""
        self.rows = [list(r) for r in rows]
        self.kinds = [int(k) for k in kinds]
        self.g, self.P, self.cfg = geometry, P, cfg
        self.layout = {int(k): list(v) for k, v in (layout or {}).items()}
        self.copies = [tuple(int(v) for v in c) for c in (copies or [])]
        self.operands = dict(operands or {})
        self._fixed = {}
        self._pairs_of = {}                                   # physical (row, column) -> pairs that name the cell
        for i, (r, c, sr, sc) in enumerate(self.copies):
            for cell in (self._phys(r, c), self._phys(sr, sc) if sr < COPY_SRC_BASE else None):
                if cell is not None:
                    self._pairs_of.setdefault(cell, []).append(i)
        self._row_v = [self._check_row(r) for r in range(len(self.rows))]
        self._pair_v = [self._check_pair(i) for i in range(len(self.copies))]
        self._base_rows = [(q, v) for q, v in enumerate(self._row_v) if v]
        self._base_pairs = [i for i, bad in enumerate(self._pair_v) if bad]

    # ---- the per-kind table ----
    def _kind_row(self, kind):
        """(selectors under the layout [sa..se, s_mul_ab, s_mul_cd, se_next, s_const], composition bits, overflow bits) or None."""
        if kind not in self._fixed:
            self._fixed[kind] = self._build_kind(kind)
        return self._fixed[kind]

    def _build_kind(self, kind):
        g = self.g
        if not valid_kind(kind, g):
            return None
        if AR.ROW_BITS_COMPOSE <= kind < AR.ROW_BITS_COMPOSE_LAST + 64:
            f = AR.fixed_row_bits_compose(kind)
        elif kind in (0, AR.ROW_VALUE):                        # NOP, VALUE: no selector, no lookup
            f = dict.fromkeys(AR.FIXED_NAMES, 0)
            f["tag_composition"] = f["tag_overflow"] = 0
        else:
            try:                                               # (without a table every row keeps its gate and has no lookup)
                f = AR.fixed_row(kind, g.w, g.L, g.carry_bits, g.carry_sub_bits, g.carry_nsub, self.cfg if self.cfg is not None else _ALL_LENS)
            except KeyError:                                   # a lookup row whose bit length the table does not hold: no fixed row
                return None
            if self.cfg is None:
                f["tag_composition"] = f["tag_overflow"] = 0
            elif kind in (AR.ROW_RANGE_U32, AR.ROW_RANGE_U32 + 1) and not f["tag_composition"]:
                return None
        col = self.layout.get(kind, [0, 1, 2, 3, 4])
        s = [0] * 9
        for k, nm in enumerate(_SEL):
            s[col[k]] = f[nm] % self.P
        ab, cd = f["s_mul_ab"] % self.P, f["s_mul_cd"] % self.P
        if ab:
            s[5 if col[0] <= 1 else 6] = ab                    # the product follows its pair of columns
            assert sorted((col[0], col[1])) in ([0, 1], [2, 3])
        if cd:
            s[5 if col[2] <= 1 else 6] = cd
            assert sorted((col[2], col[3])) in ([0, 1], [2, 3]) and not (ab and (col[0] <= 1) == (col[2] <= 1))
        s[7], s[8] = f["se_next"] % self.P, f["s_const"] % self.P
        bits = {t: b for b, t in self.cfg.tag_of.items()} if self.cfg is not None else {}
        comp, ov = bits.get(f["tag_composition"], 0), bits.get(f["tag_overflow"], 0)
        if comp or ov or s[7]:
            assert col[0] == 0 and col[4] == 4                 # a decompose row keeps a and e where the queries read them
        return s, comp, ov

    def _phys(self, row, col):
        if row >= len(self.rows) or col > 4:
            return None
        return (row, self.layout.get(self.kinds[row], (0, 1, 2, 3, 4))[col])

    # ---- the checks ----
    def _check_row(self, r):
        """The codes of row r's violations (a list of at most two)."""
        kr = self._kind_row(self.kinds[r])
        if kr is None:
            return [KIND]
        s, comp, ov = kr
        c = self.rows[r]
        P = self.P
        if c[0] >= P or c[1] >= P or c[2] >= P or c[3] >= P or c[4] >= P:
            return [RANGE]
        out = []
        if comp and (c[0] >> comp or c[1] >> comp or c[2] >> comp or c[3] >> comp):
            out.append(LOOKUP)
        elif ov and c[0] >> ov:                                # (both lookups are always evaluated; `elif` only keeps it at ONE code 2 per row)
            out.append(LOOKUP)
        if s[7] and r + 1 >= len(self.rows):
            out.append(GATE)
        else:
            e_next = self.rows[r + 1][4] if s[7] else 0
            if (s[0] * c[0] + s[1] * c[1] + s[2] * c[2] + s[3] * c[3] + s[4] * c[4] + s[5] * c[0] * c[1] + s[6] * c[2] * c[3] +
                    s[7] * e_next + s[8]) % P:
                out.append(GATE)
        return out

    def _check_pair(self, i):
        """True = pair i is violated."""
        r, c, sr, sc = self.copies[i]
        dst = self._phys(r, c)
        if dst is None:
            return True
        x = self.rows[dst[0]][dst[1]]
        if sr >= COPY_SRC_BASE:
            limbs = self.operands.get(sr)
            return limbs is None or sc >= len(limbs) or x != int(limbs[sc])
        src = self._phys(sr, sc)
        return src is None or x != self.rows[src[0]][src[1]]

    # ---- results ----
    def violations(self):
        """The multiset of (row, code) of the image, sorted."""
        out = [(r, code) for r, v in enumerate(self._row_v) for code in v]
        out += [(self.copies[i][0], COPY) for i, bad in enumerate(self._pair_v) if bad]
        return sorted(out)

    def with_cell(self, r, c, value):
        """The multiset of (row, code) of the image with PHYSICAL cell (r, c) replaced by `value` -- incremental: only row r, row r - 1
        when c is the physical e column, and the pairs that name the cell are evaluated again.  The image is left unchanged."""
        old = self.rows[r][c]
        self.rows[r][c] = value
        try:
            touched = [r] + ([r - 1] if (c == 4 and r > 0) else [])
            pairs = self._pairs_of.get((r, c), ())
            new_rows = {q: self._check_row(q) for q in touched}
            new_pairs = {i: self._check_pair(i) for i in pairs}
        finally:
            self.rows[r][c] = old
        out = [(q, code) for q, v in self._base_rows if q not in new_rows for code in v]     # (what the good image already violates: short)
        out += [(self.copies[i][0], COPY) for i in self._base_pairs if i not in new_pairs]
        out += [(q, code) for q, v in new_rows.items() for code in v]
        out += [(self.copies[i][0], COPY) for i, bad in new_pairs.items() if bad]
        return sorted(out)


# ---- the mutation set of the differential sweep -----------------------------------------------------------------------------
def mutation_set(prover, raw_patterns=True):
    """[(row, physical column, value, canonical)] in a fixed order: for every cell v + 1, v - 1 (mod p), p - 1; for columns a..d of a
    lookup-enabled row 2^bits - 1, 2^bits, 2^64; for column a of an overflow row 2^ov_bits - 1, 2^ov_bits; and -- canonical False -- the
    raw patterns p and 2^256 - 1.  Values are what the cell STANDS FOR (a raw pattern: the bytes as stored, in either representation).
    A mutant equal to the original value is not listed."""
    P = prover.P
    out = []
    for r, (cells, kind) in enumerate(zip(prover.rows, prover.kinds)):
        kr = prover._kind_row(kind)
        comp, ov = (kr[1], kr[2]) if kr is not None else (0, 0)
        for c in range(5):
            v = cells[c]
            cand = [(v + 1) % P, (v - 1) % P, P - 1]
            if comp and c < 4:
                cand += [(1 << comp) - 1, 1 << comp, 1 << 64]
            if ov and c == 0:
                cand += [(1 << ov) - 1, 1 << ov]
            seen = {v}
            for m in cand:
                if m not in seen:
                    seen.add(m)
                    out.append((r, c, m, True))
            if raw_patterns:
                out.append((r, c, P, False))
                out.append((r, c, (1 << 256) - 1, False))
    return out


def unseen_cells(prover, mutants=None, verdicts=None):
    """{(kind, LOGICAL column): [(row, good value)]}: the cells with at least one canonical mutant on which the model -- gate, lookup and
    copies -- reports nothing beyond what the good image already violates.  What the copy-map completeness check classifies.
    verdicts: the with_cell() results of `mutants`, where the caller already holds them (None entries: not canonical)."""
    if mutants is None:
        mutants = mutation_set(prover, raw_patterns=False)
    base = prover.violations()
    out = {}
    done = set()
    for i, (r, c, v, canonical) in enumerate(mutants):
        if not canonical or (r, c) in done:
            continue
        if (verdicts[i] if verdicts is not None else prover.with_cell(r, c, v)) != base:
            continue
        done.add((r, c))
        kind = prover.kinds[r]
        logical = prover.layout.get(kind, [0, 1, 2, 3, 4]).index(c)
        out.setdefault((kind, logical), []).append((r, prover.rows[r][c]))
    return out
