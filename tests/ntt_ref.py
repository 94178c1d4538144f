"""Plain model of the evaluation domain's transforms (h2r_ntt_columns; halo2 poly::domain::EvaluationDomain [3P], restated in DESIGN.md
section 2f), Python big integers only.  With n = 2^log_n_out, omega a primitive n-th root of unity, g != 0 the coset shift:
    forward:  out[j] = sum_{i < m} in[i] * (g * omega^j)^i,  j < n        (the coefficients zero-padded to n, evaluated on g * <omega>)
    inverse:  out[i] = g^-i * n^-1 * sum_{j < n} in[j] * omega^(-i * j)   (the exact inverse of forward with the same omega, g)
Natural index order on both sides.  `dft_naive` is the definition, `ntt` the recursive radix-2 form of it; the device is compared with
`forward` / `inverse` and, where 2^20 terms are too many for Python, with `horner` and the closed form of a sum of geometric sequences."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import permutation_ref as PR

FIELDS_WITH_DOMAINS = ("bn254_fr", "pasta_fp", "pasta_fq")   # p - 1 = 2^S * odd with S = 28, 32, 32 (bn254_fq: S = 1)


def omega_of(P, k):
    """A primitive 2^k-th root of unity of F_P (halo2's: PR.domain)."""
    return PR.domain(P, k)[0]


def cube_root_of_unity(P):
    """zeta != 1 with zeta^3 = 1 (P = 1 mod 3 for the fields with domains): the extended domain's coset shift in halo2."""
    assert P % 3 == 1
    g = 2
    while pow(g, (P - 1) // 3, P) == 1:
        g += 1
    return pow(g, (P - 1) // 3, P)


def dft_naive(x, w, P):
    """out[j] = sum_i x[i] * w^(i * j), len(x) terms each: O(n^2)."""
    n = len(x)
    return [sum(x[i] * pow(w, i * j, P) for i in range(n)) % P for j in range(n)]


def ntt(x, w, P):
    """The same by recursion on the even and odd coefficients; len(x) a power of two, w a primitive len(x)-th root of unity."""
    n = len(x)
    if n == 1:
        return list(x)
    w2 = w * w % P
    ev, od = ntt(x[0::2], w2, P), ntt(x[1::2], w2, P)
    out, t, h = [0] * n, 1, n // 2
    for j in range(h):
        o = od[j] * t % P
        out[j], out[j + h] = (ev[j] + o) % P, (ev[j] - o) % P
        t = t * w % P
    return out


def forward(coeffs, log_n_out, omega, g, P):
    n = 1 << log_n_out
    assert len(coeffs) <= n and len(coeffs) & (len(coeffs) - 1) == 0
    x, gi = [], 1
    for c in coeffs:
        x.append(c * gi % P)
        gi = gi * g % P
    return ntt(x + [0] * (n - len(x)), omega, P)


def inverse(evals, log_n_out, omega, g, P):
    n = 1 << log_n_out
    assert len(evals) == n
    y = ntt(list(evals), pow(omega, -1, P), P)
    ginv, f, out = pow(g, -1, P), pow(n, -1, P), []
    for v in y:
        out.append(v * f % P)
        f = f * ginv % P
    return out


def horner(coeffs, x, P):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def batch_inverse(xs, P):
    """1 / x for every x (all nonzero) with one modular inversion."""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % P
    inv, out = pow(acc, -1, P), [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * xs[i] % P
    return out


def geometric_forward(bases, js, log_n, omega, g, P):
    """forward(in, log_n, omega, g) at the indices js for in[i] = sum_b b^i, i < n = 2^log_n, without the n terms:
    sum_i (b * g * omega^j)^i = ((b * g)^n - 1) / (b * g * omega^j - 1)   (omega^(j * n) = 1; the denominators must be nonzero)."""
    n = 1 << log_n
    den = [(b * g % P * pow(omega, j, P) - 1) % P for b in bases for j in js]
    assert all(den)
    inv = batch_inverse(den, P)
    out = [0] * len(js)
    for bi, b in enumerate(bases):
        num = (pow(b * g % P, n, P) - 1) % P
        for t in range(len(js)):
            out[t] = (out[t] + num * inv[bi * len(js) + t]) % P
    return out
