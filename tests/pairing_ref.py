"""Plain model of the pairing check (h2r_pairing_prepare, h2r_pairing_products, h2r_pairing_eval) in Python integers:
the optimal ate pairing over bn256.  Fq2 = Fq[i] / (i^2 + 1) as (re, im), xi = 9 + i, Fq12 = Fq2[w] / (w^6 - xi) as a list of six Fq2
coefficients of w^0..w^5, G2 on the twist E': y^2 = x^3 + 3 / xi as affine (x, y) over Fq2, None for the identity.  A restatement; byte parity
with halo2curves' Gt is not claimed -- the pairing's properties are what tests/test_pairing_model.py holds it to."""
import msm_ref as M

Q = M.Q
R = M.R_ORDER
U = 4965661367192848881
LOOP = 6 * U + 2
R256 = 1 << 256
XI = (9, 1)
STEPS = 102
TABLE_BYTES = STEPS * 128
E_SHAPE, E_ASSERTION = 1, 9
assert Q == 36 * U ** 4 + 36 * U ** 3 + 24 * U ** 2 + 6 * U + 1 and R == 36 * U ** 4 + 36 * U ** 3 + 18 * U ** 2 + 6 * U + 1


# ---- Fq2 ----
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2neg(a):
    return ((-a[0]) % Q, (-a[1]) % Q)


def f2conj(a):
    return (a[0], (-a[1]) % Q)


def f2inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * d % Q, (-a[1]) * d % Q)


def f2pow(a, e):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2mul(r, r)
        if bit == "1":
            r = f2mul(r, a)
    return r


B2 = f2mul((3, 0), f2inv(XI))                        # the twist's b
Z2 = (0, 0)

# ---- Fq12 ----
ONE = [(1, 0)] + [Z2] * 5


def mul12(a, b):
    t = [Z2] * 11
    for i in range(6):
        if a[i] == Z2:
            continue
        for j in range(6):
            if b[j] != Z2:
                t[i + j] = f2add(t[i + j], f2mul(a[i], b[j]))
    return [f2add(t[k], f2mul(t[k + 6], XI)) if k < 5 else t[k] for k in range(6)]


def pow12(a, e):
    r = ONE
    for bit in bin(e)[2:]:
        r = mul12(r, r)
        if bit == "1":
            r = mul12(r, a)
    return r


def conj12(a):
    """a^(q^6): w -> -w"""
    return [f2neg(c) if j & 1 else c for j, c in enumerate(a)]


GAMMA = [[f2pow(XI, j * (Q ** k - 1) // 6) for j in range(6)] for k in (1, 2, 3)]


def frob12(a, k=1):
    """a^(q^k) for any k >= 0, by the maps of k = 1, 2, 3"""
    while k:
        s = min(k, 3)
        a = [f2mul(f2conj(c) if s & 1 else c, GAMMA[s - 1][j]) for j, c in enumerate(a)]
        k -= s
    return list(a)


def inv12(f):
    """the inverse with ONE Fq inversion: N = f conj(f) in Fq6, t = N^(q^2) N^(q^4), n = N t in Fq2, f^-1 = conj(f) t / n"""
    cf = conj12(f)
    n6 = mul12(f, cf)
    assert n6[1] == n6[3] == n6[5] == Z2
    t = mul12(frob12(n6, 2), frob12(n6, 4))
    n = mul12(n6, t)
    assert all(c == Z2 for c in n[1:])
    ni = f2inv(n[0])
    return [f2mul(c, ni) for c in mul12(cf, t)]


EXP = (Q ** 12 - 1) // R


def final_exp(f):
    return pow12(f, EXP)


def final_exp_chain(f):
    """The decomposition the device uses: (q^6 - 1)(q^2 + 1), then (q^4 - q^2 + 1) / r = q^3 + (6u^2 + 1) q^2 + (-36u^3 - 18u^2 - 12u + 1) q +
    (-36u^3 - 30u^2 - 18u - 2) with three powers by u; a negative exponent is a conjugation (the value is unitary after the easy part)."""
    g = mul12(conj12(f), inv12(f))
    m = mul12(frob12(g, 2), g)
    a = pow12(m, U)
    b = pow12(a, U)
    c = pow12(b, U)
    a6, b6 = pow12(a, 6), pow12(b, 6)
    t = mul12(mul12(pow12(c, 36), pow12(b6, 3)), mul12(a6, a6))
    s = mul12(mul12(t, mul12(b6, b6)), mul12(a6, mul12(m, m)))
    out = mul12(frob12(m, 3), frob12(mul12(b6, m), 2))
    return mul12(mul12(out, frob12(mul12(conj12(t), m), 1)), conj12(s))


# ---- G2 on the twist, affine ----
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))


def g2_on_curve(p):
    return p is None or f2mul(p[1], p[1]) == f2add(f2mul(f2mul(p[0], p[0]), p[0]), B2)


def g2_neg(p):
    return None if p is None else (p[0], f2neg(p[1]))


def g2_double(p):
    if p is None or p[1] == Z2:
        return None
    x, y = p
    lam = f2mul(f2mul((3, 0), f2mul(x, x)), f2inv(f2add(y, y)))
    nx = f2sub(f2mul(lam, lam), f2add(x, x))
    return (nx, f2sub(f2mul(lam, f2sub(x, nx)), y))


def g2_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        return g2_double(p) if p[1] == q[1] else None
    lam = f2mul(f2sub(q[1], p[1]), f2inv(f2sub(q[0], p[0])))
    nx = f2sub(f2sub(f2mul(lam, lam), p[0]), q[0])
    return (nx, f2sub(f2mul(lam, f2sub(p[0], nx)), p[1]))


def g2_mul(k, p):
    r = None
    for bit in bin(k)[2:]:
        r = g2_double(r)
        if bit == "1":
            r = g2_add(r, p)
    return r


def g2_frob(p):
    return (f2mul(f2conj(p[0]), GAMMA[0][2]), f2mul(f2conj(p[1]), GAMMA[0][3]))


# ---- the table of a fixed Q, the Miller value, the pairing ----
def prepare(q2):
    """(lambda, lambda x_T - y_T) per step: 64 doublings, an addition of Q after each set bit of 6u + 2 below the top one, then T += pi(Q) and
    the line through T and -pi^2(Q)"""
    tab = []
    t = q2

    def step(s):
        nonlocal t
        if s is None:
            lam = f2mul(f2mul((3, 0), f2mul(t[0], t[0])), f2inv(f2add(t[1], t[1])))
        else:
            lam = f2mul(f2sub(s[1], t[1]), f2inv(f2sub(s[0], t[0])))
        tab.append((lam, f2sub(f2mul(lam, t[0]), t[1])))
        return g2_double(t) if s is None else g2_add(t, s)

    for i in range(LOOP.bit_length() - 2, -1, -1):
        t = step(None)
        if (LOOP >> i) & 1:
            t = step(q2)
    q1 = g2_frob(q2)
    t = step(q1)
    step(g2_neg(g2_frob(q1)))
    return tab


def line(entry, p):
    lam, c = entry
    return [(p[1], 0), ((-lam[0] * p[0]) % Q, (-lam[1] * p[0]) % Q), Z2, c, Z2, Z2]


def miller(pairs):
    """pairs: (P, table) with P an affine G1 point, M.IDENT contributing no lines.  One squaring per loop bit for all pairs."""
    pairs = [(p, tab) for p, tab in pairs if p != M.IDENT]
    f, k = ONE, 0
    for i in range(LOOP.bit_length() - 2, -1, -1):
        f = mul12(f, f)
        for p, tab in pairs:
            f = mul12(f, line(tab[k], p))
        k += 1
        if (LOOP >> i) & 1:
            for p, tab in pairs:
                f = mul12(f, line(tab[k], p))
            k += 1
    for _ in range(2):
        for p, tab in pairs:
            f = mul12(f, line(tab[k], p))
        k += 1
    assert k == STEPS
    return f


def pairing(p, q2):
    return final_exp(miller([(p, prepare(q2))]))


def check(pairs):
    """the verdict of a product of pairings: (accept, Gt)"""
    gt = final_exp_chain(miller(pairs))
    return gt == ONE, gt


def miller_untwisted(p, q2):
    """A second route for the Miller value, with no table: T and the other point untwisted to E(Fq12) by (x', y') -> (x' w^2, y' w^3), the
    slope and the line l(P) = (y_P - y_T) - lambda (x_P - x_T) formed there with full Fq12 products and inversions."""
    def emb(c, d):
        v = [Z2] * 6
        v[d] = c
        return v

    def sub12(a, b):
        return [f2sub(x, y) for x, y in zip(a, b)]

    def untw(t):
        return emb(t[0], 2), emb(t[1], 3)

    xp, yp = emb((p[0], 0), 0), emb((p[1], 0), 0)

    def ell(t, s):
        xt, yt = untw(t)
        if s is None:
            lam = mul12(mul12(emb((3, 0), 0), mul12(xt, xt)), inv12(mul12(emb((2, 0), 0), yt)))
        else:
            xs, ys = untw(s)
            lam = mul12(sub12(ys, yt), inv12(sub12(xs, xt)))
        return sub12(sub12(yp, yt), mul12(lam, sub12(xp, xt)))

    f, t = ONE, q2
    for i in range(LOOP.bit_length() - 2, -1, -1):
        f = mul12(mul12(f, f), ell(t, None))
        t = g2_double(t)
        if (LOOP >> i) & 1:
            f = mul12(f, ell(t, q2))
            t = g2_add(t, q2)
    q1 = g2_frob(q2)
    f = mul12(f, ell(t, q1))
    t = g2_add(t, q1)
    return mul12(f, ell(t, g2_neg(g2_frob(q1))))


# ---- bytes in a ctx's representation ----
def fq_bytes(vals, montgomery):
    return b"".join(((v * R256 % Q) if montgomery else v).to_bytes(32, "little") for v in vals)


def fq_from_bytes(raw, montgomery):
    rinv = pow(R256, -1, Q)
    vals = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    return [v * rinv % Q for v in vals] if montgomery else vals


def fq12_bytes(a, montgomery):
    return fq_bytes([v for c in a for v in c], montgomery)


def fq12_from_bytes(raw, montgomery):
    v = fq_from_bytes(raw, montgomery)
    return [(v[2 * j], v[2 * j + 1]) for j in range(6)]


def g2_bytes(p, montgomery):
    return fq_bytes([p[0][0], p[0][1], p[1][0], p[1][1]], montgomery)


def table_bytes(tab, montgomery):
    return fq_bytes([v for lam, c in tab for v in (lam[0], lam[1], c[0], c[1])], montgomery)
