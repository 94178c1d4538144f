"""TEST HELPER: a recorded advice image as a whole halo2 circuit -- the image, the fixed columns of its row kinds, the sigma columns of its
copy pairs, the permutation and lookup products -- for the vanishing argument's quotient, plain Python.

Nothing here is a model of its own: `circuit_from_image` only places what the existing models give (advice_ref: fixed rows, lookup inputs,
the table, A' / S'; permutation_ref: sigma, Z; quotient_ref: the lookup product, l, the configuration) into the columns of a QR.Circuit.
If the conventions of those models agree -- which fixed column is which, rotation +1 for se_next, theta * tag + enable * advice, labels
delta^c * omega^i, Z_s[0] = Z_{s-1}[u], where u and the blinding rows lie, where the image starts -- the quotient of a satisfying image is
a polynomial of degree < 4n; if one of them slips it is not.

Fixed columns: 0..8 the gate's in AR.FIXED_NAMES order, then (QR.F_*) the table's tag and value, the composition arguments' tag and
enable, the overflow argument's tag and enable; enable is 1 exactly where the tag is nonzero.  The table starts at row 0 whatever
first_row is; the image's rows, and their fixed rows with them, start at first_row; every other row of a fixed column is 0."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advice_ref as AR
import mockprover_ref as MP
import ntt_ref as NR
import permutation_ref as PR
import quotient_ref as QR

LOOKUP_ADVICE = (0, 1, 2, 3, 0)                                       # composition_a..d read columns a..d, overflow_a column a
LOOKUP_TAG = (QR.F_COMP_TAG,) * 4 + (QR.F_OVER_TAG,)
LOOKUP_ENABLE = (QR.F_COMP_ENABLE,) * 4 + (QR.F_OVER_ENABLE,)


def fixed_rows_of(kinds, w, L, lcfg):
    """The model's fixed row (AR.fixed_row: a dict of integers) of every row kind of an image."""
    g = MP.Geometry(w, L)
    return [AR.fixed_row(int(kind), w, L, g.carry_bits, g.carry_sub_bits, g.carry_nsub, lcfg) for kind in kinds]


def fixed_columns(fixed_rows, table, n, first_row, P):
    """[QR.NUM_FIXED][n]: the fixed rows of the image from first_row on, the (tag, value) rows of `table` from row 0 on, 0 elsewhere."""
    fixed = [[0] * n for _ in range(QR.NUM_FIXED)]
    for i, f in enumerate(fixed_rows):
        r = first_row + i
        for g, name in enumerate(AR.FIXED_NAMES):
            fixed[g][r] = f[name] % P
        for tag_col, enable_col, tag in ((QR.F_COMP_TAG, QR.F_COMP_ENABLE, f["tag_composition"]), (QR.F_OVER_TAG, QR.F_OVER_ENABLE, f["tag_overflow"])):
            fixed[tag_col][r], fixed[enable_col][r] = tag, 1 if tag else 0
    for i, (tag, value) in enumerate(table):
        fixed[QR.F_TABLE_TAG][i], fixed[QR.F_TABLE_VALUE][i] = tag, value
    return fixed


def shifted_pairs(pairs, first_row):
    """Copy pairs counted inside the image -> counted over the circuit's rows (a source outside the image stays what it is)."""
    return [(r + first_row, c, sr if sr in PR.H2R_COPY_SRC else sr + first_row, sc) for (r, c, sr, sc) in pairs]


def config(P, k, blinding_factors=5, column_src=(0, 1, 2, 3, 4), chunk_len=2, lookup_mask=31, log_ext=None):
    """The QR.Config of an image's circuit over F_P: halo2's omega, delta and zeta, the fixed columns in the order described above."""
    log_ext = k + 3 if log_ext is None else log_ext
    return QR.Config(k, log_ext, blinding_factors, NR.omega_of(P, log_ext), NR.cube_root_of_unity(P), PR.domain(P, k)[1], QR.NUM_FIXED, range(9),
                     column_src, chunk_len, lookup_mask, LOOKUP_ADVICE, LOOKUP_TAG, LOOKUP_ENABLE, QR.F_TABLE_TAG, QR.F_TABLE_VALUE)


def circuit_from_image(rows, kinds, pairs, w, L, P, lcfg, k, ch, rng, blinding_factors=5, first_row=0, column_src=(0, 1, 2, 3, 4), chunk_len=2,
                       fixed_rows=None, table=None, lookup_mask=31, log_ext=None):
    """rows: [[5 integers]], the image's PHYSICAL cells; kinds: one row kind per row; pairs: (row, col, src_row, src_col) counted inside
    the image; lcfg: AR.LookupConfig; ch = (theta, beta, gamma, y); rng: where the tails behind row u come from.  fixed_rows / table: the
    image's fixed rows (dicts as AR.fixed_row's) and the table's (tag, value) rows where the caller has its own -- the library's, say --
    instead of the model's.  column_src entries >= 5 are extra columns of random values that no pair names.
    Returns a QR.Circuit with cfg, P, ch, lag, and pairs (shifted to first_row), lcfg, fixed_rows, first_row, image_rows."""
    cfg = config(P, k, blinding_factors, column_src, chunk_len, lookup_mask, log_ext)
    n, u, m, omega, delta = cfg.n, cfg.u, cfg.m, cfg.omega(P), cfg.delta
    theta, beta, gamma, _ = ch
    fixed_rows = fixed_rows_of(kinds, w, L, lcfg) if fixed_rows is None else fixed_rows
    table = lcfg.table() if table is None else table
    assert len(rows) == len(kinds) == len(fixed_rows) and first_row + len(rows) <= u and len(table) <= u, "the image or the table does not fit 2^k rows"

    def tail(col):
        return list(col) + [rng.randrange(P) for _ in range(n - len(col))]

    fixed = fixed_columns(fixed_rows, table, n, first_row, P)
    advice = PR.columns(rows, None, range(5), u, first_row)
    extra = [[rng.randrange(P) for _ in range(u)] for _ in range(cfg.n_extra)]
    moved = shifted_pairs(pairs, first_row)
    sigma = PR.sigma_from_pairs(moved, m, n, delta, omega, P, column_of={src: c for c, src in enumerate(column_src) if src < 5})
    lag = dict(advice=[tail(c) for c in advice], extra=[tail(c) for c in extra], fixed=fixed, sigma=sigma, l=QR.vanishing_lagrange(cfg))
    circ = QR.Circuit(cfg=cfg, P=P, ch=ch, lag=lag, pairs=moved, lcfg=lcfg, fixed_rows=fixed_rows, first_row=first_row, image_rows=len(rows))

    inputs = AR.lookup_inputs(rows, fixed_rows, u)
    S = AR.table_column(lcfg, theta, u, P)
    assert S == [(theta * t + v) % P for t, v in zip(fixed[QR.F_TABLE_TAG][:u], fixed[QR.F_TABLE_VALUE][:u])], "the table the caller gave is not lcfg's"
    lag["lookup_a_perm"], lag["lookup_s_perm"], lag["lookup_z"] = [None] * 5, [None] * 5, [None] * 5
    for a in cfg.args:
        A = AR.compress([(0, 0)] * first_row + inputs[AR.ARGS[a]][:u - first_row], theta, P)
        assert A == circ.lookup_input(a), "AR.lookup_inputs and the fixed columns disagree on " + AR.ARGS[a]
        Ap, Sp = AR.permute_expression_pair(A, S)
        Z = QR.lookup_product(A, S, Ap, Sp, beta, gamma, P)
        lag["lookup_a_perm"][a], lag["lookup_s_perm"][a], lag["lookup_z"][a] = tail(Ap), tail(Sp), tail(Z)
    # (the permutation's Z last: its tails are the only ones whose number depends on chunk_len, so the others do not move with it)
    z = PR.product(rows, extra, sigma, column_src, chunk_len, delta, omega, beta, gamma, u, P, first_row)
    assert None not in z, "a zero denominator under these challenges"
    lag["perm_z"] = [tail(col) for col in z]
    return circ


# ---- evaluation, with the extended form of unchanged columns kept ---------------------------------------------------------------------------
def extended(circ, cache=None):
    """circ.extended(); cache: a dict that keeps (Lagrange column, extended column) per extension, so that a circuit which shares columns
    with an earlier one -- the same key, the same image with one cell changed -- transforms only what differs."""
    if cache is None:
        return circ.extended()
    cfg, P, out = circ.cfg, circ.P, {}
    for name, group in circ.lag.items():
        out[name] = []
        for col in group:
            if col is None:
                out[name].append(None)
                continue
            key = (cfg.k, cfg.log_ext, P, hash(tuple(col)))
            hit = cache.get(key)
            if hit is None or hit[0] != col:
                hit = cache[key] = (list(col), QR.extend(cfg, col, P))
            out[name].append(hit[1])
    return out


def quotient_coefficients(circ, cache=None):
    """The N coefficients of the model's h of the circuit."""
    return QR.coefficients(circ.cfg, QR.quotient(circ.cfg, extended(circ, cache), circ.ch, circ.P), circ.P)
