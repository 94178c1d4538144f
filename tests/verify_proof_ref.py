"""Plain model of the verifier's accumulators (prover.verify_proof, h2r_proof_decode, h2r_verify_scalars, h2r_msm_terms; DESIGN.md section
2n): everything of halo2's GWC verifier up to the pairing, over the plain models of create_proof_ref, transcript_ref and msm_ref (imported,
not edited).  Python integers only; nothing here is shared with the library.

A proof is ACCEPTED iff e(L, [tau]G2) = e(R, G2); with a known tau that is [tau] L = R, which `accepts` checks.  With the challenge u drawn
after the four W,
    L = sum_p u^p W_p
    R = sum_p u^p (z_p W_p + sum_i v^i C_{p,i} - [sum_i v^i e_{p,i}] G)
-- the four equations of create_proof_ref.verify, multiplied by u^p and summed.  R is formed as ONE sum of scalar x base over the fixed
base order of `bases_of`; `scalars_of` gives the scalars."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import create_proof_ref as C
import msm_ref as M
import opening_ref as OR
from transcript_ref import E_ASSERTION, E_SHAPE, Q, R, Transcript

KIND_COMBINE = 6                                   # the generator's column kind of combine's rho
TAG_COMBINE = KIND_COMBINE * 256


class VerifyingKey:
    """What a verifier holds of one circuit shape: the configuration, the commitments of the fixed and sigma columns, G and vk_repr."""

    def __init__(self, key, tau):
        self.cfg, self.vk_repr = key.cfg, key.vk_repr
        self.fixed, self.sigma, self.g = key.commitments("fixed", tau), key.commitments("sigma", tau), M.G


def decode_item(kind, raw):
    """(status, value) of 32 proof bytes: a scalar >= r or an abscissa >= q is E_SHAPE, an abscissa of no point E_ASSERTION."""
    val = int.from_bytes(raw, "little")
    if kind == "scalar":
        return (E_SHAPE, None) if val >= R else (0, val)
    x, sign = val & ((1 << 255) - 1), val >> 255
    if x >= Q:
        return E_SHAPE, None
    rhs = (x * x * x + M.B) % Q
    y = pow(rhs, (Q + 1) // 4, Q)
    if y * y % Q != rhs:
        return E_ASSERTION, None
    return 0, (x, y if y & 1 == sign else Q - y)


def decode(cfg, proof):
    """(status, {section: values}): E_SHAPE wins over E_ASSERTION wherever in the proof the two occur."""
    layout = C.proof_layout(cfg)
    assert len(proof) == 32 * sum(c for _, _, c in layout)
    sec, off, status = {}, 0, 0
    for name, kind, count in layout:
        sec[name] = []
        for _ in range(count):
            st, val = decode_item(kind, proof[off:off + 32])
            off += 32
            status = E_SHAPE if E_SHAPE in (st, status) else max(st, status)
            sec[name].append(val)
    return status, (sec if not status else None)


def challenges(vk, sec, instances):
    """theta, beta, gamma, y, x, v, u: the prover's rounds as common rounds, one more after the four W."""
    T = Transcript()
    st = T.round([("scalar", vk.vk_repr)] + [("scalar", s) for s in instances], common=True)[0]
    assert st == 0, "an instance is not canonical"

    def absorb(names, squeeze, kind="point"):
        st, ch, _ = T.round([(kind, v) for nm in names for v in sec[nm]], squeeze=squeeze, common=True)
        assert st == 0
        return ch

    (theta,), (beta, gamma), (y,), (x,) = absorb(["advice"], 1), absorb(["lookup_perm"], 2), absorb(["perm_z", "lookup_z", "random"], 1), absorb(["h"], 1)
    (v,) = absorb(["evals"], 1, "scalar")
    (u,) = absorb(["w"], 1)
    return theta, beta, gamma, y, x, v, u


def base_index(cfg):
    """{(group, index): position} of the fixed base order: the proof's points in proof order (5 advice, A' and S' interleaved per argument,
    the permutation Z, the lookup Z, the random polynomial, 4 h pieces, 4 W), then the key's fixed and sigma commitments, then G."""
    A, S = len(cfg.args), len(cfg.sets)
    order = [("advice", c) for c in range(5)]
    for a in range(A):
        order += [("lookup_a_perm", a), ("lookup_s_perm", a)]
    order += [("perm_z", s) for s in range(S)] + [("lookup_z", a) for a in range(A)] + [("random", 0)]
    order += [("h", i) for i in range(C.H_PIECES)] + [("w", p) for p in range(4)]
    order += [("fixed", i) for i in range(cfg.num_fixed)] + [("sigma", c) for c in range(cfg.m)] + [("g", 0)]
    return {key: pos for pos, key in enumerate(order)}


def bases_of(vk, sec):
    return sec["advice"] + sec["lookup_perm"] + sec["perm_z"] + sec["lookup_z"] + sec["random"] + sec["h"] + sec["w"] + vk.fixed + vk.sigma + [vk.g]


def scalars_of(cfg, evals, ch):
    """(status, the scalars of R in base order, the four scalars u^p of L) from the evaluations (proof order) and the seven challenges."""
    theta, beta, gamma, y, x, v, u = ch
    n = cfg.n
    xn = pow(x, n, R)
    if xn == 1:
        return E_ASSERTION, None, None
    ev = {}
    for (g, i, p), val in zip(C.queries(C.eval_plan(cfg)), evals):
        ev.setdefault(g, {}).setdefault(i, {})[C.ROT[p]] = val
    ev["l"] = {i: {0: val} for i, val in enumerate(C.lagrange_at(cfg, x))}
    acc = 0
    for t in OR.constraint_at_point(cfg, ev, (theta, beta, gamma, y), x, R):
        acc = (acc * y + t) % R
    ev["h"] = {0: {0: acc * pow(xn - 1, -1, R) % R}}
    pos = base_index(cfg)
    args = {a: k for k, a in enumerate(cfg.args)}                  # a lookup column's place among the proof's points
    out = [0] * len(pos)
    points, up, g_sum, left = C.points_of(cfg, x), 1, 0, []
    for p in range(4):
        vp, e_sum = 1, 0
        for g, i, m in C.open_plan(cfg):
            if not (m >> p) & 1:
                continue
            coeff = up * vp % R
            if g == "h":
                for j in range(C.H_PIECES):
                    out[pos[("h", j)]] = (out[pos[("h", j)]] + coeff * pow(xn, j, R)) % R
            else:
                at = pos[(g, args[i] if g.startswith("lookup") else i)]
                out[at] = (out[at] + coeff) % R
            e_sum = (e_sum + vp * ev[g][i][C.ROT[p]]) % R
            vp = vp * v % R
        out[pos[("w", p)]] = up * points[p] % R
        g_sum = (g_sum + up * e_sum) % R
        left.append(up)
        up = up * u % R
    out[pos[("g", 0)]] = -g_sum % R
    return 0, out, left


def accumulate(vk, proof, instances=()):
    """(status, L, R): affine points, None under a status."""
    cfg = vk.cfg
    status, sec = decode(cfg, proof)
    if status:
        return status, None, None
    ch = challenges(vk, sec, instances)
    status, right, left = scalars_of(cfg, sec["evals"], ch)
    if status:
        return status, None, None
    return 0, M.naive_msm(left, sec["w"]), M.naive_msm(right, bases_of(vk, sec))


def accepts(left, right, tau):
    return M.mul(tau % R, left) == right


def rho(seed, circuit):
    return C.random_element(seed, circuit, TAG_COMBINE, 0)


def combine(lefts, rights, statuses, seed):
    """(L*, R*) = (sum rho_e L_e, sum rho_e R_e) over the circuits whose status is 0; rho_e of the generator under TAG_COMBINE, row 0."""
    rhos = [0 if st else rho(seed, e) for e, st in enumerate(statuses)]
    clean = lambda pts: [M.IDENT if st else p for p, st in zip(pts, statuses)]
    return M.naive_msm(rhos, clean(lefts)), M.naive_msm(rhos, clean(rights))
