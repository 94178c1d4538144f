"""Plain model of the openings (h2r_fold_columns, h2r_open_eval_columns, h2r_open_witness_columns; halo2 vanishing::prover::evaluate,
poly::eval_polynomial and the GWC multi-open's kate_division [3P], restated in DESIGN.md section 2h), Python big integers only.

A column is a list of coefficients, lowest first.  `constraint_at_point` is quotient_ref.terms restated on EVALUATIONS instead of coset
values -- what a verifier computes: X_j becomes x, a rotated read becomes the evaluation at the rotated point, l0 / l_last / l_active become
their own evaluations at x -- so that for a satisfied circuit the terms folded with y equal h(x) * (x^n - 1).  `query_plan` is THIS
circuit's query pattern over the points (x, omega x, omega^-1 x, omega^-(blinding_factors + 1) x), in one fixed order that the tests use
for the device's descriptors as well; the order is the caller's, not upstream's transcript order."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quotient_ref as QR

LAST = "last"                              # the rotation by -(blinding_factors + 1) rows
POINT_ROT = (0, 1, -1, LAST)               # the rotation of point p: x, omega x, omega^-1 x, omega^-(blinding_factors + 1) x


def evaluate(col, z, P):
    acc = 0
    for c in reversed(col):
        acc = (acc * z + c) % P
    return acc


def kate_division(g, z, P):
    """(W, remainder) with W * (X - z) + remainder = g, len(W) = len(g) and W[-1] = 0: upstream's loop, from the top coefficient down."""
    b = -z % P
    W = [0] * len(g)
    tmp = 0
    for i in range(len(g) - 1, 0, -1):
        lead = (g[i] - tmp) % P
        W[i - 1] = lead
        tmp = lead * b % P
    return W, (g[0] - tmp) % P


def witness(cols, masks, points, v, P):
    """Per point p: None where no column's mask names it, else (W, remainder) of g = sum_{c in Q_p} v^idx(c) cols[c], idx counted within Q_p."""
    out = []
    for p, z in enumerate(points):
        sel = [c for c, m in enumerate(masks) if (m >> p) & 1]
        if not sel:
            out.append(None)
            continue
        g = [0] * len(cols[sel[0]])
        for idx, c in enumerate(sel):
            vp = pow(v, idx, P)
            g = [(a + vp * b) % P for a, b in zip(g, cols[c])]
        out.append(kate_division(g, z, P))
    return out


def queries(masks, num_points):
    """The query list: (column, point) over the set bits in column order, points ascending within a column."""
    return [(c, p) for c, m in enumerate(masks) for p in range(num_points) if (m >> p) & 1]


def fold(cols, s, P):
    """out[i] = sum_c s^c cols[c][i]."""
    return [sum(pow(s, c, P) * col[i] for c, col in enumerate(cols)) % P for i in range(len(cols[0]))]


def points_of(cfg, x, P):
    """x, omega x, omega^-1 x, omega^-(blinding_factors + 1) x."""
    w = cfg.omega(P)
    wi = pow(w, -1, P)
    return [x, w * x % P, wi * x % P, pow(wi, cfg.blinding_factors + 1, P) * x % P]


def query_plan(cfg):
    """[(group, index, point mask)] of this circuit's queries, the folded h (group "h") last: advice at x, the column under se_next (4) also at
    omega x; every permutation Z at x and omega x, all but the last set's also at omega^-(blinding_factors + 1) x; a lookup's Z at x and
    omega x, A' at x and omega^-1 x, S' at x; extra, fixed, sigma and the three l columns at x."""
    plan = [("advice", c, 3 if c == 4 else 1) for c in range(5)] + [("extra", j, 1) for j in range(cfg.n_extra)]
    S = len(cfg.sets)
    plan += [("perm_z", s, 3 | (8 if s < S - 1 else 0)) for s in range(S)]
    for a in cfg.args:
        plan += [("lookup_z", a, 3), ("lookup_a_perm", a, 5), ("lookup_s_perm", a, 1)]
    plan += [("fixed", i, 1) for i in range(cfg.num_fixed)] + [("sigma", c, 1) for c in range(cfg.m)] + [("l", i, 1) for i in range(3)]
    return plan + [("h", 0, 1)]


def evals_of(plan, values):
    """The flat values of the plan's query list -> {group: {index: {rotation: value}}}."""
    out, q = {}, 0
    for group, i, mask in plan:
        for p in range(4):
            if (mask >> p) & 1:
                out.setdefault(group, {}).setdefault(i, {})[POINT_ROT[p]] = values[q]
                q += 1
    assert q == len(values)
    return out


def constraint_at_point(cfg, evals, ch, x, P):
    """quotient_ref.terms on evaluations: the terms at x, in the contract's order.  evals[group][index][rotation]."""
    theta, beta, gamma, _ = ch
    adv, fx = evals["advice"], evals["fixed"]
    s = [fx[i][0] for i in cfg.gate_fixed]
    v = [adv[i][0] for i in range(5)]
    out = [sum(s[i] * v[i] for i in range(5)) + s[5] * v[0] * v[1] + s[6] * v[2] * v[3] + s[7] * adv[4][1] + s[8]]
    l0, l_last, l_active = (evals["l"][i][0] for i in range(3))
    Z, S = evals["perm_z"], len(cfg.sets)
    out.append(l0 * (1 - Z[0][0]))
    out.append(l_last * (Z[S - 1][0] ** 2 - Z[S - 1][0]))
    for si in range(1, S):
        out.append(l0 * (Z[si][0] - Z[si - 1][LAST]))
    for si, cs in enumerate(cfg.sets):
        left, right = Z[si][1], Z[si][0]
        for c in cs:
            src = cfg.column_src[c]
            vc = adv[src][0] if src < 5 else evals["extra"][src - 5][0]
            left = left * (vc + beta * evals["sigma"][c][0] + gamma) % P
            right = right * (vc + pow(cfg.delta, c, P) * beta % P * x + gamma) % P
        out.append(l_active * (left - right))
    for a in cfg.args:
        Ak = theta * fx[cfg.lookup_tag[a]][0] + fx[cfg.lookup_enable[a]][0] * adv[cfg.lookup_advice[a]][0]
        Sk = theta * fx[cfg.table_tag][0] + fx[cfg.table_value][0]
        Ap, Sp, Zk = evals["lookup_a_perm"][a], evals["lookup_s_perm"][a], evals["lookup_z"][a]
        out.append(l0 * (1 - Zk[0]))
        out.append(l_last * (Zk[0] ** 2 - Zk[0]))
        out.append(l_active * (Zk[1] * (Ap[0] + beta) % P * (Sp[0] + gamma) - Zk[0] * (Ak + beta) % P * (Sk + gamma)))
        out.append(l0 * (Ap[0] - Sp[0]))
        out.append(l_active * (Ap[0] - Sp[0]) % P * (Ap[0] - Ap[-1]))
    return [t % P for t in out]


def identity_sides(cfg, evals, ch, x, P):
    """(the terms at x folded with y, h(x) * (x^n - 1)): equal for a satisfied circuit."""
    acc = 0
    for t in constraint_at_point(cfg, evals, ch, x, P):
        acc = (acc * ch[3] + t) % P
    return acc, evals["h"][0][0] * (pow(x, cfg.n, P) - 1) % P
