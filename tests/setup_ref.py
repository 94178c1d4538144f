"""Plain model of the two scalar families of the KZG setup (h2r_kzg_setup_scalars) in Python integers: the powers
tau^i and the Lagrange values l_i(tau) = omega^i (tau^n - 1) / (n (tau - omega^i)) of the domain of omega, with `pow` and ONE batched
inversion.  The points of a key are then msm_ref.mul_g_batch of these."""
import msm_ref as M

R = M.R_ORDER


def powers(tau, n):
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * tau % R
    assert out[-1] == pow(tau, n - 1, R)
    return out


def batch_inverse(vals):
    """The inverses of nonzero residues with one `pow` (Montgomery's trick)."""
    pref, acc = [], 1
    for v in vals:
        pref.append(acc)
        acc = acc * v % R
    inv = pow(acc, -1, R)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pref[i] % R
        inv = inv * vals[i] % R
    return out


def lagrange(tau, omega, k):
    """[l_i(tau)] for i < 2^k; tau must lie outside the domain."""
    n = 1 << k
    assert pow(omega, n // 2, R) == R - 1 and pow(tau, n, R) != 1
    ws = powers(omega, n)
    c = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    inv = batch_inverse([(tau - w) % R for w in ws])
    return [w * c % R * d % R for w, d in zip(ws, inv)]


def edge_scalars(rng, random_count=32):
    """The scalars the fixed-base walk is pinned on: 0, 1, 255, 256, 2^(8w) - 1 and 2^(8w) at w = 1, 8, 31, r - 1, r, r + 1, 2^256 - 1
    (all-0xFF digits), alternating 0 / 255 digits both ways, random values below 2^256."""
    vals = [0, 1, 255, 256]
    for w in (1, 8, 31):
        vals += [(1 << (8 * w)) - 1, 1 << (8 * w)]
    vals += [R - 1, R, R + 1, (1 << 256) - 1]
    vals += [int.from_bytes(bytes([0, 255] * 16), "little"), int.from_bytes(bytes([255, 0] * 16), "little")]
    return vals + [rng.getrandbits(256) for _ in range(random_count)]
