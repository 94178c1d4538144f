"""Plain model of the vanishing argument's quotient h on the extended domain (h2r_quotient_columns; halo2 plonk::evaluation::evaluate_h [3P],
restated in DESIGN.md section 2g), Python big integers only, point by point, on top of ntt_ref / permutation_ref / advice_ref.

n = 2^k, N = 2^log_ext, r = N / n, u = n - blinding_factors - 1; X_j = zeta * omega_ext^j; f<t>[j] = f[(j + t * r) mod N].  `terms` lists the
terms of one point in the contract's order, `quotient` folds them (acc = acc * y + t) and divides by X_j^n - 1.  `satisfying_circuit` builds
a small synthetic circuit whose constraints hold, so that h is a polynomial of degree < 4n (every constraint has degree <= 5)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import advice_ref as AR
import ntt_ref as NR
import permutation_ref as PR

GATE = AR.FIXED_NAMES           # sa, sb, sc, sd, se, s_mul_ab, s_mul_cd, se_next, s_const: the order of gate_fixed
LOOKUP_ARGS = 5
PER_CIRCUIT = ("advice", "extra", "perm_z", "lookup_a_perm", "lookup_s_perm", "lookup_z")
KEY = ("fixed", "sigma", "l")


class Config:
    def __init__(self, k, log_ext, blinding_factors, omega_ext, zeta, delta, num_fixed, gate_fixed, column_src, chunk_len, lookup_mask=0,
                 lookup_advice=(0, 1, 2, 3, 0), lookup_tag=(0,) * 5, lookup_enable=(0,) * 5, table_tag=0, table_value=0):
        self.k, self.log_ext, self.blinding_factors = k, log_ext, blinding_factors
        self.omega_ext, self.zeta, self.delta = omega_ext, zeta, delta
        self.num_fixed, self.gate_fixed, self.column_src, self.chunk_len = num_fixed, list(gate_fixed), list(column_src), chunk_len
        self.lookup_mask, self.lookup_advice, self.lookup_tag, self.lookup_enable = lookup_mask, list(lookup_advice), list(lookup_tag), list(lookup_enable)
        self.table_tag, self.table_value = table_tag, table_value
        self.n, self.N = 1 << k, 1 << log_ext
        self.r, self.u, self.m = self.N // self.n, self.n - blinding_factors - 1, len(column_src)
        self.n_extra = max([s - 4 for s in column_src if s >= 5] + [0])
        chunk = min(chunk_len, self.m)
        self.sets = [range(c0, min(self.m, c0 + chunk)) for c0 in range(0, self.m, chunk)]
        self.args = [a for a in range(LOOKUP_ARGS) if (lookup_mask >> a) & 1]

    def omega(self, P):
        return pow(self.omega_ext, self.r, P)


def terms(cfg, cols, ch, j, P):
    """The terms of point j, in order: the gate; the permutation argument's; per selected lookup argument its five."""
    theta, beta, gamma, _ = ch
    N, r = cfg.N, cfg.r

    def rot(col, t):
        return col[(j + t * r) % N]

    adv, fx = cols["advice"], cols["fixed"]
    s = [fx[i][j] for i in cfg.gate_fixed]
    v = [adv[i][j] for i in range(5)]
    out = [sum(s[i] * v[i] for i in range(5)) + s[5] * v[0] * v[1] + s[6] * v[2] * v[3] + s[7] * rot(adv[4], 1) + s[8]]
    l0, l_last, l_active = (c[j] for c in cols["l"])
    Z, S = cols["perm_z"], len(cfg.sets)
    X = cfg.zeta * pow(cfg.omega_ext, j, P) % P
    out.append(l0 * (1 - Z[0][j]))
    out.append(l_last * (Z[S - 1][j] ** 2 - Z[S - 1][j]))
    for si in range(1, S):
        out.append(l0 * (Z[si][j] - rot(Z[si - 1], -(cfg.blinding_factors + 1))))
    for si, cs in enumerate(cfg.sets):
        left, right = rot(Z[si], 1), Z[si][j]
        for c in cs:
            src = cfg.column_src[c]
            vc = adv[src][j] if src < 5 else cols["extra"][src - 5][j]
            left = left * (vc + beta * cols["sigma"][c][j] + gamma) % P
            right = right * (vc + pow(cfg.delta, c, P) * beta % P * X + gamma) % P
        out.append(l_active * (left - right))
    for a in cfg.args:
        Ak = theta * fx[cfg.lookup_tag[a]][j] + fx[cfg.lookup_enable[a]][j] * adv[cfg.lookup_advice[a]][j]
        Sk = theta * fx[cfg.table_tag][j] + fx[cfg.table_value][j]
        Ap, Sp, Zk = cols["lookup_a_perm"][a], cols["lookup_s_perm"][a], cols["lookup_z"][a]
        out.append(l0 * (1 - Zk[j]))
        out.append(l_last * (Zk[j] ** 2 - Zk[j]))
        out.append(l_active * (rot(Zk, 1) * (Ap[j] + beta) % P * (Sp[j] + gamma) - Zk[j] * (Ak + beta) % P * (Sk + gamma)))
        out.append(l0 * (Ap[j] - Sp[j]))
        out.append(l_active * (Ap[j] - Sp[j]) % P * (Ap[j] - rot(Ap, -1)))
    return [t % P for t in out]


def vanishing_inverses(cfg, P):
    """1 / (X_j^n - 1) for j mod r = 0 .. r - 1."""
    zn, wn = pow(cfg.zeta, cfg.n, P), pow(cfg.omega_ext, cfg.n, P)
    den = [(zn * pow(wn, i, P) - 1) % P for i in range(cfg.r)]
    assert all(den), "zeta^n lies in the subgroup"
    return [pow(d, -1, P) for d in den]


def quotient(cfg, cols, ch, P):
    y, inv = ch[3], vanishing_inverses(cfg, P)
    h = []
    for j in range(cfg.N):
        acc = 0
        for t in terms(cfg, cols, ch, j, P):
            acc = (acc * y + t) % P
        h.append(acc * inv[j % cfg.r] % P)
    return h


def extend(cfg, col, P):
    """A Lagrange column of n values -> its N values on the coset zeta * <omega_ext>."""
    return NR.forward(NR.inverse(col, cfg.k, cfg.omega(P), 1, P), cfg.log_ext, cfg.omega_ext, cfg.zeta, P)


def coefficients(cfg, h, P):
    return NR.inverse(h, cfg.log_ext, cfg.omega_ext, cfg.zeta, P)


def vanishing_lagrange(cfg):
    """l0, l_last, l_active = 1 - l_last - l_blind over the n rows."""
    n, u = cfg.n, cfg.u
    return [[1] + [0] * (n - 1), [0] * u + [1] + [0] * (n - u - 1), [1] * u + [0] * (n - u)]


def extend_all(cfg, lag, P):
    """Every column of a dict of Lagrange columns (None where an argument has none) in extended form."""
    return {name: [None if c is None else extend(cfg, c, P) for c in group] for name, group in lag.items()}


def random_columns(rng, cfg, P):
    """Random extended columns (an unsatisfied circuit): equality with the device matters there, not satisfaction."""
    def col():
        return [rng.randrange(P) for _ in range(cfg.N)]
    sel = [col() if (cfg.lookup_mask >> a) & 1 else None for a in range(LOOKUP_ARGS)]
    return dict(advice=[col() for _ in range(5)], extra=[col() for _ in range(cfg.n_extra)], perm_z=[col() for _ in cfg.sets],
                lookup_a_perm=sel, lookup_s_perm=[None if c is None else col() for c in sel], lookup_z=[None if c is None else col() for c in sel],
                fixed=[col() for _ in range(cfg.num_fixed)], sigma=[col() for _ in range(cfg.m)], l=[col() for _ in range(3)])


# ---- a small circuit whose constraints hold ------------------------------------------------------------------------------------------------
F_TABLE_TAG, F_TABLE_VALUE, F_COMP_TAG, F_COMP_ENABLE, F_OVER_TAG, F_OVER_ENABLE, NUM_FIXED = 9, 10, 11, 12, 13, 14, 15


def lookup_product(A, S, Ap, Sp, beta, gamma, P):
    """Z[0] = 1, Z[i+1] = Z[i] (A+beta)(S+gamma) / ((A'+beta)(S'+gamma))."""
    Z = [1]
    for i in range(len(A)):
        den = (Ap[i] + beta) * (Sp[i] + gamma) % P
        assert den, "a zero denominator under these challenges"
        Z.append(Z[-1] * (A[i] + beta) % P * (S[i] + gamma) % P * pow(den, -1, P) % P)
    return Z


class Circuit:
    """cfg, ch = (theta, beta, gamma, y), lag = the Lagrange columns by group; what the faults need: the copy pairs, the range-constrained
    cells and the lookup configuration."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def solve_s_const(self):
        """s_const of every usable row so that the gate holds there."""
        c, P = self.cfg, self.P
        adv, fx = self.lag["advice"], self.lag["fixed"]
        for i in range(c.u):
            s = [fx[g][i] for g in c.gate_fixed]
            v = [adv[q][i] for q in range(5)]
            rest = sum(s[q] * v[q] for q in range(5)) + s[5] * v[0] * v[1] + s[6] * v[2] * v[3] + s[7] * adv[4][(i + 1) % c.n]
            fx[c.gate_fixed[8]][i] = -rest % P

    def lookup_input(self, a):
        c, P, fx = self.cfg, self.P, self.lag["fixed"]
        return [(self.ch[0] * fx[c.lookup_tag[a]][i] + fx[c.lookup_enable[a]][i] * self.lag["advice"][c.lookup_advice[a]][i]) % P for i in range(c.u)]

    def extended(self):
        return extend_all(self.cfg, self.lag, self.P)

    def h(self):
        return quotient(self.cfg, self.extended(), self.ch, self.P)


def satisfying_circuit(rng, P, k, log_ext=None, blinding_factors=5, chunk_len=2, lookup_mask=31, n_cycles=4, bit_lens=(1, 2)):
    """Six permutation columns (the five advice columns and one extra) with random copy cycles, random main-gate rows (some with se_next)
    whose s_const is solved, a table of two bit lengths with range-constrained cells on random rows (arguments 0..3 read columns a..d under
    one tag column, argument 4 column a under another) and A' / S' / Z of the existing models, random blinding tails behind row u."""
    log_ext = k + 3 if log_ext is None else log_ext
    omega_ext, (_, delta) = NR.omega_of(P, log_ext), PR.domain(P, k)
    column_src = [0, 1, 2, 3, 4, 5]
    cfg = Config(k, log_ext, blinding_factors, omega_ext, NR.cube_root_of_unity(P), delta, NUM_FIXED, range(9), column_src, chunk_len, lookup_mask,
                 (0, 1, 2, 3, 0), (F_COMP_TAG,) * 4 + (F_OVER_TAG,), (F_COMP_ENABLE,) * 4 + (F_OVER_ENABLE,), F_TABLE_TAG, F_TABLE_VALUE)
    n, u, m, omega = cfg.n, cfg.u, cfg.m, cfg.omega(P)
    lcfg = AR.LookupConfig(bit_lens)
    assert lcfg.n_rows <= u
    ch = tuple(rng.randrange(1, P) for _ in range(4))
    theta, beta, gamma, _ = ch

    def tail(col):
        return list(col) + [rng.randrange(P) for _ in range(n - len(col))]

    # copy cycles, then the range constraints: a cell's class takes a value below the smallest bound any of its cells carries
    v, pairs = PR.satisfying_cells(rng, m, u, n_cycles, P)
    comp_bits = [rng.choice((0, 0) + tuple(lcfg.bit_lens)) for _ in range(u)]
    over_bits = [rng.choice((0, 0, 0) + tuple(lcfg.bit_lens)) for _ in range(u)]
    bound = {}
    for i in range(u):
        for c in range(4):
            if comp_bits[i]:
                bound[(c, i)] = 1 << comp_bits[i]
        if over_bits[i]:
            bound[(0, i)] = min(bound.get((0, i), P), 1 << over_bits[i])
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            x = parent[x]
        return x

    for (row, col, src_row, src_col) in pairs:
        parent[find((col, row))] = find((src_col, src_row))
    cls_bound = {}
    for cell, b in bound.items():
        cls_bound[find(cell)] = min(cls_bound.get(find(cell), P), b)
    cls_value = {root: rng.randrange(b) for root, b in sorted(cls_bound.items())}
    for c in range(m):
        for i in range(u):
            if find((c, i)) in cls_value:
                v[c][i] = cls_value[find((c, i))]
    constrained = sorted(bound)

    fixed = [[0] * n for _ in range(NUM_FIXED)]
    for i in range(u):
        for g in range(8):
            if rng.random() < (0.3 if g == 7 else 0.6):
                fixed[g][i] = rng.randrange(P)
        fixed[F_COMP_TAG][i] = lcfg.tag_of[comp_bits[i]] if comp_bits[i] else 0
        fixed[F_COMP_ENABLE][i] = 1 if comp_bits[i] else 0
        fixed[F_OVER_TAG][i] = lcfg.tag_of[over_bits[i]] if over_bits[i] else 0
        fixed[F_OVER_ENABLE][i] = 1 if over_bits[i] else 0
    for i, (t, val) in enumerate(lcfg.table()):
        fixed[F_TABLE_TAG][i], fixed[F_TABLE_VALUE][i] = t, val

    lag = dict(advice=[tail(v[c]) for c in range(5)], extra=[tail(v[5])], fixed=fixed, l=vanishing_lagrange(cfg),
               sigma=PR.sigma_from_pairs(pairs, m, n, delta, omega, P))
    circ = Circuit(cfg=cfg, P=P, ch=ch, lag=lag, pairs=pairs, constrained=constrained, lcfg=lcfg, comp_bits=comp_bits, over_bits=over_bits)
    circ.solve_s_const()
    cells = [[lag["advice"][c][i] for c in range(5)] for i in range(u)]
    z = PR.product(cells, [lag["extra"][0][:u]], lag["sigma"], column_src, chunk_len, delta, omega, beta, gamma, u, P)
    assert None not in z and z[-1][u] == 1
    lag["perm_z"] = [tail(col) for col in z]
    table = AR.table_column(lcfg, theta, u, P)
    lag["lookup_a_perm"], lag["lookup_s_perm"], lag["lookup_z"] = [None] * 5, [None] * 5, [None] * 5
    for a in cfg.args:
        A = circ.lookup_input(a)
        Ap, Sp = AR.permute_expression_pair(A, table)
        Z = lookup_product(A, table, Ap, Sp, beta, gamma, P)
        assert Z[u] == 1
        lag["lookup_a_perm"][a], lag["lookup_s_perm"][a], lag["lookup_z"][a] = tail(Ap), tail(Sp), tail(Z)
    return circ
