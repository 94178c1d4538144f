#!/usr/bin/env python3
"""Timing of the KZG setup on the device at the reference's sizes k = 15, 16, 17 and at k = 20, both
representations, bn254_fr.
Per stage, between two events on the stream, medians over the timed calls after one untimed call: the fixed-base table, the two scalar
launches (powers, Lagrange values), the two fixed-base multiplications; and prover.setup whole, as wall time around a synchronise (it
includes [tau]G2 on the host).  In the same process, bytes compared first: the Lagrange key by the direct route (l_i(tau) through
h2r_fixed_base_mul) against the existing curve transform over the monomial key (EvaluationDomain.lagrange_key), alternated call by call.
One inversion per lane is the only variant of the multiplication that was built; there is no batched-inversion variant to compare.
For scale only: the Python route the tests used before (tests/msm_ref.mul_g_batch of the powers of tau) at k = 11, wall time, per point.
No target is set and nothing rests on these numbers.
    python tools/setup_timing.py [calls] > profiles/kzg_setup.txt"""
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib, prover
import msm_ref as M
import setup_ref as S

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SIZES = (15, 16, 17, 20)
R, R256 = M.R_ORDER, 1 << 256
TAU = random.Random("setup/timing").randrange(2, R)


def stream_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def fmt(v):
    return "%.3f (min %.3f, max %.3f)" % (statistics.median(v), min(v), max(v))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: two events on the stream around each stage's call, medians of %d timed calls after one untimed; wall clock around a synchronise where stated." % REPS)
    print(torch.cuda.get_device_name(0), flush=True)
    for montgomery in (False, True):
        chip = H.BigIntChip(64, 256, field="bn254_fr", montgomery=montgomery)
        tau = TAU * R256 % R if montgomery else TAU
        for k in SIZES:
            n = 1 << k
            omega = prover.field_omega(chip, k)
            one = R256 % R if montgomery else 1
            dom = H.EvaluationDomain(chip, k, k, omega, one)
            params = prover.setup(chip, k, tau=tau)                 # the untimed call of every stage
            other = dom.lagrange_key(params.g)
            torch.cuda.synchronize()
            assert torch.equal(params.g_lagrange.bases.reshape(-1), other.bases.reshape(-1)), "the two routes to the Lagrange key differ"
            t = {name: [] for name in ("table", "powers", "lagrange", "mul powers", "mul lagrange", "transform", "setup wall")}
            table, pw, lag = prover.fixed_base_table(chip), None, None
            out_g, out_l = torch.empty_like(params.g.bases), torch.empty_like(params.g.bases)
            for _ in range(REPS):
                t["table"].append(stream_ms(lambda: prover.fixed_base_table(chip, out=table))[0])
                ms, pw = stream_ms(lambda: prover.setup_scalars(chip, _lib.H2R_SETUP_POWERS, n, tau, out=pw))
                t["powers"].append(ms)
                ms, lag = stream_ms(lambda: prover.setup_scalars(chip, _lib.H2R_SETUP_LAGRANGE, k, tau, omega, out=lag))
                t["lagrange"].append(ms)
                t["mul powers"].append(stream_ms(lambda: prover.fixed_base_mul(chip, table, pw, out=out_g))[0])
                t["mul lagrange"].append(stream_ms(lambda: prover.fixed_base_mul(chip, table, lag, out=out_l))[0])
                t["transform"].append(stream_ms(lambda: dom.lagrange_key(params.g))[0])          # (alternated with the direct route)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                prover.setup(chip, k, tau=tau)
                torch.cuda.synchronize()
                t["setup wall"].append(1e3 * (time.perf_counter() - t0))
            assert torch.equal(out_g, params.g.bases) and torch.equal(out_l, params.g_lagrange.bases)
            print("%s ctx, k = %d (%d points), ms:" % ("Montgomery" if montgomery else "canonical", k, n))
            print("    table %s; scalars: powers %s, Lagrange %s" % (fmt(t["table"]), fmt(t["powers"]), fmt(t["lagrange"])))
            print("    fixed-base multiplication: powers %s, Lagrange values %s (%.1f M points/s at the median)"
                  % (fmt(t["mul powers"]), fmt(t["mul lagrange"]), n / statistics.median(t["mul lagrange"]) / 1e3))
            print("    Lagrange key, bytes equal: direct route (scalars + multiplication) %.3f; curve transform over g %s"
                  % (statistics.median(t["lagrange"]) + statistics.median(t["mul lagrange"]), fmt(t["transform"])))
            print("    prover.setup whole, wall time with [tau]G2 on the host: %s" % fmt(t["setup wall"]), flush=True)
            del params, other, out_g, out_l, pw, lag
            torch.cuda.empty_cache()
    M.g_table()
    t0 = time.perf_counter()
    pts = M.mul_g_batch(S.powers(TAU, 1 << 11))
    dt = time.perf_counter() - t0
    print("for scale, the Python route (tests/msm_ref.mul_g_batch over the powers of tau) at k = 11: %.2f s wall, %.0f us per point (%d points, the model's own table of G made before the clock starts)"
          % (dt, 1e6 * dt / len(pts), len(pts)))
