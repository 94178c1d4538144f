"""Plain model of the commitments (h2r_msm_columns, h2r_curve_eval): bn256 G1, y^2 = x^3 + 3 over Fq, of prime order
R_ORDER (= the modulus of bn254_fr), Python big integers only.  Jacobian arithmetic with every exceptional case spelled out (nothing here
shares a formula with the library's complete projective ones), a batch-inverted conversion to affine, naive double-and-add, and a
fixed-base table for [k]G.  Affine points are (x, y) tuples, (0, 0) the identity -- halo2curves' encoding [3P], restated, not pinned.

Expectations for large n cost ONE scalar multiplication because the bases are structured: P_i = [a0 + i d]G is made by one addition per
base, and sum_i s_i P_i = [sum_i s_i (a0 + i d) mod r]G."""
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617
B = 3
G = (1, 2)
IDENT = (0, 0)
JIDENT = (1, 1, 0)
R256 = 1 << 256


def on_curve(p):
    return p == IDENT or (p[1] * p[1] - p[0] * p[0] * p[0] - B) % Q == 0


def neg(p):
    return p if p == IDENT else (p[0], -p[1] % Q)


def jac(p):
    return JIDENT if p == IDENT else (p[0], p[1], 1)


def jdouble(p):
    X, Y, Z = p
    if Z == 0 or Y == 0:
        return JIDENT
    A, Bq = X * X % Q, Y * Y % Q
    C = Bq * Bq % Q
    D = 2 * ((X + Bq) * (X + Bq) - A - C) % Q
    E = 3 * A % Q
    X3 = (E * E - 2 * D) % Q
    return X3, (E * (D - X3) - 8 * C) % Q, 2 * Y * Z % Q


def jadd(p, q):
    X1, Y1, Z1 = p
    X2, Y2, Z2 = q
    if Z1 == 0:
        return q
    if Z2 == 0:
        return p
    Z1Z1, Z2Z2 = Z1 * Z1 % Q, Z2 * Z2 % Q
    U1, U2 = X1 * Z2Z2 % Q, X2 * Z1Z1 % Q
    S1, S2 = Y1 * Z2 * Z2Z2 % Q, Y2 * Z1 * Z1Z1 % Q
    if U1 == U2:
        return jdouble(p) if S1 == S2 else JIDENT
    H, Rr = (U2 - U1) % Q, (S2 - S1) % Q
    HH = H * H % Q
    HHH, V = H * HH % Q, U1 * HH % Q
    X3 = (Rr * Rr - HHH - 2 * V) % Q
    return X3, (Rr * (V - X3) - S1 * HHH) % Q, Z1 * Z2 * H % Q


def to_affine_batch(pts):
    """Jacobian points -> affine tuples with one inversion (Montgomery's trick); the identity -> (0, 0)."""
    pref, acc = [], 1
    for (_, _, Z) in pts:
        pref.append(acc)
        if Z:
            acc = acc * Z % Q
    inv = pow(acc, -1, Q)
    out = [IDENT] * len(pts)
    for i in range(len(pts) - 1, -1, -1):
        X, Y, Z = pts[i]
        if Z:
            zi = inv * pref[i] % Q
            inv = inv * Z % Q
            zi2 = zi * zi % Q
            out[i] = (X * zi2 % Q, Y * zi2 * zi % Q)
    return out


def to_affine(p):
    return to_affine_batch([p])[0]


def add(p, q):
    return to_affine(jadd(jac(p), jac(q)))


def jmul(k, p):
    """[k]p by naive double-and-add, k any non-negative integer; Jacobian result."""
    acc, base = JIDENT, jac(p)
    for bit in bin(k)[2:] if k else "":
        acc = jdouble(acc)
        if bit == "1":
            acc = jadd(acc, base)
    return acc


def mul(k, p):
    return to_affine(jmul(k, p))


def proj_to_affine(X, Y, Z):
    """A homogeneous projective triple (the library's form: x = X / Z, y = Y / Z) -> affine."""
    if Z % Q == 0:
        return IDENT
    zi = pow(Z, -1, Q)
    return (X * zi % Q, Y * zi % Q)


_TABLE = []


def g_table():
    """T[w][d] = [d * 256^w]G, affine, w < 32, d < 256: [k]G is then at most 32 additions."""
    if not _TABLE:
        rows, base = [], jac(G)
        for _ in range(32):
            row = [JIDENT, base]
            for _d in range(2, 256):
                row.append(jadd(row[-1], base))
            rows.append(row)
            base = jadd(row[-1], base)
        flat = to_affine_batch([p for row in rows for p in row])
        _TABLE.extend([flat[256 * w:256 * (w + 1)] for w in range(32)])
    return _TABLE


def jmul_g(k):
    T, acc = g_table(), JIDENT
    k %= R_ORDER
    for w in range(32):
        d = (k >> (8 * w)) & 255
        if d:
            acc = jadd(acc, jac(T[w][d]))
    return acc


def mul_g(k):
    return to_affine(jmul_g(k))


def mul_g_batch(ks):
    return to_affine_batch([jmul_g(k) for k in ks])


def structured_bases(n, a0, d):
    """P_i = [a0 + i d]G for i < n: one addition per base, one inversion in all."""
    step, cur, out = jac(mul_g(d)), jmul_g(a0), []
    for _ in range(n):
        out.append(cur)
        cur = jadd(cur, step)
    return to_affine_batch(out)


def structured_sum(scalars, a0, d, period=None):
    """sum_i scalars[i] * P_(i mod period) for the structured bases: one scalar multiplication."""
    if period is None:
        k = sum(s * (a0 + i * d) for i, s in enumerate(scalars))
    else:
        k = sum(s * (a0 + (i % period) * d) for i, s in enumerate(scalars))
    return mul_g(k % R_ORDER)


def naive_msm(scalars, bases):
    acc = JIDENT
    for s, p in zip(scalars, bases):
        acc = jadd(acc, jmul(s, p))
    return to_affine(acc)


def words(v):
    return [(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]


def point_bytes(pts, montgomery):
    """Affine points -> the bytes of a device array [n][2][4] uint64 in the ctx's representation (coordinates are Fq elements)."""
    if montgomery:
        return b"".join((x * R256 % Q).to_bytes(32, "little") + (y * R256 % Q).to_bytes(32, "little") for x, y in pts)
    return b"".join(x.to_bytes(32, "little") + y.to_bytes(32, "little") for x, y in pts)


def scalar_bytes(vals, montgomery):
    """Scalars (integers below 2^256) -> 32 bytes each in the ctx's representation; a Montgomery ctx holds s * R mod r."""
    if montgomery:
        return b"".join((s * R256 % R_ORDER).to_bytes(32, "little") for s in vals)
    return b"".join(s.to_bytes(32, "little") for s in vals)


def points_from_bytes(raw, montgomery):
    rinv = pow(R256, -1, Q)
    vals = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
    if montgomery:
        vals = [v * rinv % Q for v in vals]
    return [(vals[i], vals[i + 1]) for i in range(0, len(vals), 2)]
