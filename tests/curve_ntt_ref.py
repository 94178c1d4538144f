"""Plain model of the transform over curve points (h2r_curve_ntt, CommitKey.transform; halo2's g_to_lagrange [3P], restated in DESIGN.md
section 2k), on top of tests/msm_ref.py (the curve) and tests/ntt_ref.py (the field), Python big integers only.  With n = 2^k points P_j,
omega a primitive n-th root of unity of the scalar field (the group order r), natural index order on both sides:
    forward:  out[i] = sum_j [omega^(i j)] P_j            inverse:  out[i] = [n^-1] sum_j [omega^(-i j)] P_j
Two routes that share nothing with the library and little with each other:
  1. `naive`: the definition, n^2 naive scalar multiplications (jmul) and additions (jadd) -- any points, (0, 0) included;
  2. `by_logs`: for bases [a_j]G the transform is [ntt(a)_i]G, the field transform of the logarithms through the fixed-base table.
For the arithmetic-progression bases of msm_ref.structured_bases(n, a0, d) the inverse transform has a closed form (`closed_form_logs`):
sum_j omega^(-i j) = 0 and sum_j j x^j = n / (x - 1) for x = omega^(-i) != 1, so index i != 0 is [d / (omega^(-i) - 1)]G and index 0 is the
mean, [a0 + d (n - 1) / 2]G."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_ref as M
import ntt_ref as NR

R = M.R_ORDER


def omega_of(k):
    """halo2's primitive 2^k-th root of unity of the scalar field."""
    return NR.omega_of(R, k)


def naive(points, omega, inverse):
    """The definition on affine points ((0, 0) = the identity): n^2 scalar multiplications."""
    n = len(points)
    w = pow(omega, -1, R) if inverse else omega
    f = pow(n, -1, R) if inverse else 1
    out = []
    for i in range(n):
        acc = M.JIDENT
        for j, p in enumerate(points):
            acc = M.jadd(acc, M.jmul(pow(w, i * j, R), p))
        out.append(M.jmul(f, M.to_affine(acc)))
    return M.to_affine_batch(out)


def logs_transform(logs, omega, inverse):
    """The field transform of the logarithms: what the points' transform is the image of."""
    k = len(logs).bit_length() - 1
    assert len(logs) == 1 << k
    return NR.inverse(logs, k, omega, 1, R) if inverse else NR.forward(logs, k, omega, 1, R)


def by_logs(logs, omega, inverse):
    """The transform of the bases [logs[j]]G, through the fixed-base table."""
    return M.mul_g_batch(logs_transform(logs, omega, inverse))


def closed_form_logs(n, a0, d, omega, indices):
    """The logarithms of the INVERSE transform of structured_bases(n, a0, d) at `indices`, without the n terms."""
    nz = [i for i in indices if i % n]
    inv = dict(zip(nz, NR.batch_inverse([(pow(omega, -i, R) - 1) % R for i in nz], R)))
    mean = (a0 + d * (n - 1) * pow(2, -1, R)) % R
    return [d * inv[i] % R if i % n else mean for i in indices]
