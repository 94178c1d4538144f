#!/usr/bin/env python3
"""Timing of the evaluation domain's transforms (h2r_ntt_columns): 256 circuits x 6 columns of random field elements, canonical and
Montgomery ctx, three ways: k = 17 -> 17 inverse (lagrange_to_coeff), k = 17 -> 19 forward on a coset (coeff_to_extended), k = 19 -> 19
inverse on the coset (extended_to_coeff).  Per launch class (the events the dispatch itself stamps, h2r_profile_*) after three untimed
calls: the setup launch that fills the twiddle tables, and the passes one by one; every pass as a fraction of the 8 TB/s HBM roofline on
the bytes of ONE read and ONE write of the column per pass (the assumption; the first pass of 17 -> 19 reads only the 2^17 coefficients).
    python tools/ntt_timing.py [circuits] [repetitions] > profiles/ntt_columns.txt"""
import ctypes
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
import ntt_ref as NR

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
COLS = 6
K, EK = 17, 19
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R256 = 1 << 256
HBM = 8.0e12
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "halo2_rsa_amd", "csrc", "h2r_ntt.hpp")) as f:
    TILE_LOG = int(re.search(r"constexpr u32 NTT_TILE_LOG = (\d+);", f.read()).group(1))
WAYS = [("k = 17 -> 17, inverse (lagrange_to_coeff)", K, K, True, False),
        ("k = 17 -> 19, forward on the coset (coeff_to_extended)", K, EK, False, True),
        ("k = 19 -> 19, inverse on the coset (extended_to_coeff)", EK, EK, True, True)]


def stages(log_n):
    """The kernel's split of log_n stages into passes (ntt_plan in h2r_ntt.hpp)."""
    passes, left, out = (log_n + TILE_LOG - 1) // TILE_LOG, log_n, []
    for q in range(passes):
        out.append((left + (passes - q) - 1) // (passes - q))
        left -= out[-1]
    return out


def run(montgomery):
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    rep = (lambda v: v * R256 % P) if montgomery else (lambda v: v)
    dom = H.EvaluationDomain(chip, K, EK, rep(NR.omega_of(P, EK)), rep(NR.cube_root_of_unity(P)))
    print("%s ctx: %d circuits x %d columns, tiles of 2^%d elements, %d timed calls" % ("Montgomery" if montgomery else "canonical", B, COLS, TILE_LOG, REPS))
    for title, log_in, log_out, inverse, coset in WAYS:
        src = torch.randint(0, 256, (B, COLS, 1 << log_in, 32), dtype=torch.uint8, device="cuda")
        src[:, :, :, 31] &= 0x0F                                                       # below 2^252 < p: field elements in either representation
        out = torch.empty((B, COLS, 1 << log_out, 32), dtype=torch.uint8, device="cuda")

        def call():
            dom.ntt(src, log_out, inverse=inverse, shift=dom.zeta if coset else None, out=out)

        for _ in range(3):
            call()
        torch.cuda.synchronize()
        _lib.profile_enable(8 * REPS)
        for _ in range(REPS):
            call()
            torch.cuda.synchronize()
        setup = [float(x) for x in _lib.profile_read(_lib.KERNEL_NTT_SETUP)]
        passes = [float(x) for x in _lib.profile_read(_lib.KERNEL_NTT_PASS)]
        _lib.profile_enable(0)
        split = stages(log_out)
        assert len(setup) == REPS and len(passes) == REPS * len(split), (len(setup), len(passes))
        print("  " + title + ": %d passes of %s stages" % (len(split), " + ".join(map(str, split))))
        print("    setup  median %7.3f ms (min %7.3f, max %7.3f)   the twiddle tables: not column traffic" % (statistics.median(setup), min(setup), max(setup)))
        col_in, col_out, total_ms, total_bytes = B * COLS * (32 << log_in), B * COLS * (32 << log_out), 0.0, 0
        for q in range(len(split)):
            t = passes[q::len(split)]
            med = statistics.median(t)
            moved = (col_in if q == 0 else col_out) + col_out                          # ASSUMED: one read and one write of the column per pass
            total_ms, total_bytes = total_ms + med, total_bytes + moved
            print("    pass %d median %7.3f ms (min %7.3f, max %7.3f)   %6.2f GB  %5.2f TB/s = %.3f of the 8 TB/s roofline"
                  % (q + 1, med, min(t), max(t), moved / 1e9, moved / med / 1e9, moved / (med * 1e-3) / HBM))
        print("    the passes summed: %.3f ms = %.3f of the roofline on %.2f GB; %.4f ms per column (%d columns)"
              % (total_ms, total_bytes / (total_ms * 1e-3) / HBM, total_bytes / 1e9, total_ms / (B * COLS), B * COLS))
        del src, out
        torch.cuda.empty_cache()
    print(flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: every time below (HIP events stamped by the dispatches themselves, medians over the timed calls).")
    print("ASSUMED: the 8 TB/s HBM roofline (the data-sheet figure) and one read plus one write of the column per pass; no clock is read,")
    print("         and no figure below depends on one.")
    print(torch.cuda.get_device_name(0))
    for m in (False, True):
        run(m)
        torch.cuda.empty_cache()
