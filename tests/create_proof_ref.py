"""Plain model of the prover's randomness (h2r_random_columns, h2r_random_eval): the counter-based generator of the
blinding values and its table of tags.  The hash is Python's hashlib -- a true oracle, not a restatement of the library's compression
function -- and everything else is Python integers.  The tag table restates DESIGN's independently of the library.  Nothing here is shared
with the library."""
import hashlib

from transcript_ref import R, reduce_wide, to_repr

PERSON = b"H2R-Blinding-v1\0"
assert len(PERSON) == 16

# column kind x index: tag = kind * 256 + index
KIND_ADVICE, KIND_LOOKUP_A_PERM, KIND_LOOKUP_S_PERM, KIND_PERM_Z, KIND_LOOKUP_Z, KIND_RANDOM_POLY = range(6)
KIND_COUNTS = {KIND_ADVICE: 5, KIND_LOOKUP_A_PERM: 5, KIND_LOOKUP_S_PERM: 5, KIND_PERM_Z: 8, KIND_LOOKUP_Z: 5, KIND_RANDOM_POLY: 1}


def tag(kind: int, index: int = 0) -> int:
    assert 0 <= index < KIND_COUNTS[kind]
    return kind * 256 + index


TAGS = [tag(kind, i) for kind, count in sorted(KIND_COUNTS.items()) for i in range(count)]


def message(seed: bytes, circuit: int, tag_: int, row: int) -> bytes:
    assert len(seed) == 32
    return seed + circuit.to_bytes(8, "little") + tag_.to_bytes(4, "little") + (0).to_bytes(4, "little") + row.to_bytes(8, "little")


def digest(seed: bytes, circuit: int, tag_: int, row: int) -> bytes:
    return hashlib.blake2b(message(seed, circuit, tag_, row), digest_size=64, person=PERSON).digest()


def random_element(seed: bytes, circuit: int, tag_: int, row: int) -> int:
    """The canonical value of one element."""
    return reduce_wide(digest(seed, circuit, tag_, row))


def random_bytes(seed: bytes, circuit: int, tag_: int, rows, montgomery: bool) -> bytes:
    """Rows `rows` of one column of one circuit as they lie in the ctx's memory."""
    return b"".join(to_repr(random_element(seed, circuit, tag_, i), R, montgomery).to_bytes(32, "little") for i in rows)


# ---- the model prover and the model verifier (prover.create_proof; DESIGN.md section 2m, the round table) -------------------------------------
# Written from the table in DESIGN, over the existing plain models; with bases [tau^i]G a commitment is [f(tau)]G, so a column costs one
# fixed-base multiplication.  The point sets, in order of first appearance in the GWC query list: x, omega x, omega^-(bf+1) x, omega^-1 x.
import advice_ref as AR
import msm_ref as M
import ntt_ref as NR
import opening_ref as OR
import permutation_ref as PR
import quotient_ref as QR
from transcript_ref import Q, Transcript

ROT = (0, 1, OR.LAST, -1)                                # the rotation of point set p
H_PIECES = 4


class Key:
    """The model's proving and verifying key of one circuit shape: the configuration, the fixed and sigma columns (Lagrange, integers), what
    the lookup inputs need, and the caller's vk_repr."""

    def __init__(self, cfg, fixed, sigma, fixed_rows, lcfg, first_row, vk_repr):
        self.cfg, self.fixed, self.sigma, self.fixed_rows, self.lcfg, self.first_row, self.vk_repr = cfg, fixed, sigma, fixed_rows, lcfg, first_row, vk_repr
        assert cfg.N == 8 * cfg.n and cfg.n_extra == 0
        self._coeff, self._commit = {}, {}

    def coeff(self, group):
        if group not in self._coeff:
            self._coeff[group] = [to_coeff(self.cfg, col) for col in getattr(self, group)]
        return self._coeff[group]

    def commitments(self, group, tau):
        if (group, tau) not in self._commit:
            self._commit[(group, tau)] = [commit(c, tau) for c in self.coeff(group)]
        return self._commit[(group, tau)]


def to_coeff(cfg, lagrange):
    return NR.inverse(lagrange, cfg.k, cfg.omega(R), 1, R)


def commit(coeffs, tau):
    return M.mul_g(NR.horner(coeffs, tau, R))


def eval_plan(cfg):
    """[(group, index, point-set mask)] in the order the evaluations are written."""
    S = len(cfg.sets)
    plan = [("advice", c, 3 if c == 4 else 1) for c in range(5)] + [("fixed", i, 1) for i in range(cfg.num_fixed)] + [("random", 0, 1)]
    plan += [("sigma", c, 1) for c in range(cfg.m)] + [("perm_z", s, 3 | (4 if s < S - 1 else 0)) for s in range(S)]
    for a in cfg.args:
        plan += [("lookup_z", a, 3), ("lookup_a_perm", a, 9), ("lookup_s_perm", a, 1)]
    return plan


def open_plan(cfg):
    """The GWC query list: the same columns and masks in the multi-open's order, the folded h and the random polynomial last."""
    by_group = {}
    for q in eval_plan(cfg):
        by_group.setdefault(q[0], []).append(q)
    plan = by_group["advice"] + by_group["perm_z"]
    for a in cfg.args:
        plan += [q for g in ("lookup_z", "lookup_a_perm", "lookup_s_perm") for q in by_group[g] if q[1] == a]
    return plan + by_group["fixed"] + by_group["sigma"] + [("h", 0, 1)] + by_group["random"]


def queries(plan):
    return [(g, i, p) for g, i, m in plan for p in range(4) if (m >> p) & 1]


def points_of(cfg, x):
    w = cfg.omega(R)
    wi = pow(w, -1, R)
    return [x, w * x % R, pow(wi, cfg.blinding_factors + 1, R) * x % R, wi * x % R]


def proof_layout(cfg):
    """(name, kind, count) of every section of the proof, in order."""
    return [("advice", "point", 5), ("lookup_perm", "point", 2 * len(cfg.args)), ("perm_z", "point", len(cfg.sets)), ("lookup_z", "point", len(cfg.args)),
            ("random", "point", 1), ("h", "point", H_PIECES), ("evals", "scalar", len(queries(eval_plan(cfg)))), ("w", "point", 4)]


def prove(rows, key, seed, circuit_index, tau, instances=(), strict=True):
    """The proof bytes of one circuit whose image is `rows` ([[5 integers]], PHYSICAL cells).  strict=False: an image that does not satisfy
    the circuit gets the proof an honest prover's code would write for it (h truncated to its four pieces)."""
    cfg, e = key.cfg, circuit_index
    n, u, k, omega, fr = cfg.n, cfg.u, cfg.k, cfg.omega(R), key.first_row

    def tail(col, kind, i, used):
        assert len(col) >= used
        return list(col[:used]) + [random_element(seed, e, tag(kind, i), r) for r in range(used, n)]

    T = Transcript()
    assert T.round([("scalar", key.vk_repr)] + [("scalar", v) for v in instances], common=True)[0] == 0
    lag, co, C = {"fixed": key.fixed, "sigma": key.sigma, "l": QR.vanishing_lagrange(cfg), "extra": []}, {}, {}

    def group(name, cols):
        lag[name] = cols
        co[name] = [to_coeff(cfg, c) for c in cols]
        C[name] = [commit(c, tau) for c in co[name]]

    group("advice", [tail(c, KIND_ADVICE, i, u) for i, c in enumerate(PR.columns(rows, None, range(5), u, fr))])
    _, (theta,), _ = T.round([("point", p) for p in C["advice"]], squeeze=1)
    inputs = AR.lookup_inputs(rows, key.fixed_rows, u)
    table = AR.table_column(key.lcfg, theta, u, R)
    A, Ap, Sp = {}, [], []
    for a in cfg.args:
        A[a] = AR.compress([(0, 0)] * fr + inputs[AR.ARGS[a]][:u - fr], theta, R)
        ap, sp = AR.permute_expression_pair(A[a], table)
        Ap.append(tail(ap, KIND_LOOKUP_A_PERM, a, u))
        Sp.append(tail(sp, KIND_LOOKUP_S_PERM, a, u))
    group("lookup_a_perm", Ap)
    group("lookup_s_perm", Sp)
    _, (beta, gamma), _ = T.round([("point", p) for a in range(len(cfg.args)) for p in (C["lookup_a_perm"][a], C["lookup_s_perm"][a])], squeeze=2)
    z = PR.product(rows, [], key.sigma, cfg.column_src, cfg.chunk_len, cfg.delta, omega, beta, gamma, u, R, fr)
    assert None not in z
    group("perm_z", [tail(c, KIND_PERM_Z, s, u + 1) for s, c in enumerate(z)])
    group("lookup_z", [tail(QR.lookup_product(A[a], table, Ap[a][:u], Sp[a][:u], beta, gamma, R), KIND_LOOKUP_Z, a, u + 1) for a in cfg.args])
    co["random"] = [[random_element(seed, e, tag(KIND_RANDOM_POLY), r) for r in range(n)]]
    C["random"] = [commit(co["random"][0], tau)]
    _, (y,), _ = T.round([("point", p) for p in C["perm_z"] + C["lookup_z"] + C["random"]], squeeze=1)
    h = QR.coefficients(cfg, QR.quotient(cfg, QR.extend_all(cfg, lag, R), (theta, beta, gamma, y), R), R)
    assert not strict or not any(h[H_PIECES * n:]), "the image does not satisfy the circuit"
    pieces = [h[i * n:(i + 1) * n] for i in range(H_PIECES)]
    _, (x,), _ = T.round([("point", commit(p, tau)) for p in pieces], squeeze=1)
    points = points_of(cfg, x)
    co["fixed"], co["sigma"], co["h"] = key.coeff("fixed"), key.coeff("sigma"), [OR.fold(pieces, pow(x, n, R), R)]
    evals = [NR.horner(co[g][i], points[p], R) for g, i, p in queries(eval_plan(cfg))]
    _, (v,), _ = T.round([("scalar", s) for s in evals], squeeze=1)
    plan = open_plan(cfg)
    W = OR.witness([co[g][i] for g, i, _ in plan], [m for _, _, m in plan], points, v, R)
    T.round([("point", commit(w, tau)) for w, _ in W])
    return T.proof


def decompress(raw):
    """32 proof bytes -> the affine point, or None where x >= q or x is the abscissa of no point."""
    val = int.from_bytes(raw, "little")
    x, sign = val & ((1 << 255) - 1), val >> 255
    rhs = (x * x * x + M.B) % Q
    y = pow(rhs, (Q + 1) // 4, Q)
    if x >= Q or y * y % Q != rhs:
        return None
    return (x, y if y & 1 == sign else Q - y)


def lagrange_at(cfg, x):
    """l0(x), l_last(x), l_active(x) in closed form: l_i(x) = (x^n - 1) / n * omega^i / (x - omega^i)."""
    n, u, w = cfg.n, cfg.u, cfg.omega(R)
    zn = (pow(x, n, R) - 1) * pow(n, -1, R) % R

    def l(i):
        wi = pow(w, i, R)
        return zn * wi % R * pow((x - wi) % R, -1, R) % R

    l_last = l(u)
    return [l(0), l_last, (1 - l_last - sum(l(i) for i in range(u + 1, n))) % R]


def verify(key, proof, tau, instances=()):
    """Whether the model verifier accepts `proof` under the key's verifying half (its configuration, the commitments of its fixed and
    sigma columns, vk_repr) and the instances."""
    cfg, n = key.cfg, key.cfg.n
    layout = proof_layout(cfg)
    if len(proof) != 32 * sum(c for _, _, c in layout):
        return False
    sec, off = {}, 0
    for name, kind, count in layout:
        items = []
        for i in range(count):
            raw = proof[off:off + 32]
            off += 32
            val = decompress(raw) if kind == "point" else int.from_bytes(raw, "little")
            if val is None or (kind == "scalar" and val >= R):
                return False
            items.append(val)
        sec[name] = items
    T = Transcript()
    T.round([("scalar", key.vk_repr)] + [("scalar", v) for v in instances], common=True)

    def absorb(names, squeeze, kind="point"):
        return T.round([(kind, v) for nm in names for v in sec[nm]], squeeze=squeeze, common=True)[1]

    (theta,), (beta, gamma), (y,), (x,) = absorb(["advice"], 1), absorb(["lookup_perm"], 2), absorb(["perm_z", "lookup_z", "random"], 1), absorb(["h"], 1)
    (v,) = absorb(["evals"], 1, "scalar")
    if pow(x, n, R) == 1:
        return False
    ev = {}
    for (g, i, p), val in zip(queries(eval_plan(cfg)), sec["evals"]):
        ev.setdefault(g, {}).setdefault(i, {})[ROT[p]] = val
    ev["l"] = {i: {0: val} for i, val in enumerate(lagrange_at(cfg, x))}
    acc = 0
    for t in OR.constraint_at_point(cfg, ev, (theta, beta, gamma, y), x, R):
        acc = (acc * y + t) % R
    ev["h"] = {0: {0: acc * pow(pow(x, n, R) - 1, -1, R) % R}}
    Cm = {"advice": sec["advice"], "lookup_a_perm": sec["lookup_perm"][0::2], "lookup_s_perm": sec["lookup_perm"][1::2], "perm_z": sec["perm_z"],
          "lookup_z": sec["lookup_z"], "random": sec["random"], "fixed": key.commitments("fixed", tau), "sigma": key.commitments("sigma", tau)}
    folded, xn = M.JIDENT, pow(x, n, R)
    for i, c in enumerate(sec["h"]):
        folded = M.jadd(folded, M.jmul(pow(xn, i, R), c))
    Cm["h"] = [M.to_affine(folded)]
    points, plan = points_of(cfg, x), open_plan(cfg)
    for p in range(4):
        rhs, e_sum, vp = M.JIDENT, 0, 1
        for g, i, m in plan:
            if (m >> p) & 1:
                rhs, e_sum = M.jadd(rhs, M.jmul(vp, Cm[g][i])), (e_sum + vp * ev[g][i][ROT[p]]) % R
                vp = vp * v % R
        rhs = M.jadd(rhs, M.jmul_g(-e_sum % R))
        if M.mul((tau - points[p]) % R, sec["w"][p]) != M.to_affine(rhs):
            return False
    return True
