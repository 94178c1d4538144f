#!/usr/bin/env python3
"""Timing of the openings (h2r_fold_columns, h2r_open_eval_columns, h2r_open_witness_columns): 256 circuits of n = 2^17 coefficients, 30
columns with this circuit's query pattern over the four points x, omega x, omega^-1 x, omega^-(blinding_factors + 1) x -- per circuit five
advice columns (one also at omega x), three permutation Z (x, omega x; two of them also at the last rotation), per lookup argument Z (x,
omega x), A' (x, omega^-1 x) and S' (x), the folded h; from the key six columns at x -- 46 queries.  Random field elements (the work does not
depend on the values), canonical and Montgomery ctx.  Times are the events the dispatch itself stamps (h2r_profile_*), per launch class,
after three untimed calls.  Next to each call: the bytes under the ASSUMPTION stated in the output and that traffic against the 8 TB/s HBM
roofline.  No threshold: there is no earlier implementation to compare with.
    python tools/open_timing.py [circuits] [repetitions] > profiles/opening.txt"""
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
LOG_N, PIECES = 17, 4
N = 1 << LOG_N
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R256 = 1 << 256
HBM = 8.0e12
# (per-circuit?, point mask) in query order
PATTERN = [(True, 1)] * 4 + [(True, 3)] + [(True, 11), (True, 11), (True, 3)] + [(True, 3), (True, 5), (True, 1)] * 5 + [(False, 1)] * 6 + [(True, 1)]
assert len(PATTERN) == 30


def columns(*lead):
    t = torch.randint(0, 256, lead + (N, 32), dtype=torch.uint8, device="cuda")
    t[..., 31] &= 0x0F                                                                  # below 2^252 < p: field elements in either representation
    return t


def timed(call, classes):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    _lib.profile_enable(8 * REPS)
    for _ in range(REPS):
        call()
        torch.cuda.synchronize()
    out = {k: [float(x) for x in _lib.profile_read(k)] for k in classes}
    _lib.profile_enable(0)
    assert all(len(t) == REPS for t in out.values()), {k: len(t) for k, t in out.items()}
    return out


def report(what, names, times, moved):
    total = [sum(times[k][i] for k in times) for i in range(REPS)]
    med = statistics.median(total)
    for k, nm in names:
        print("  %-18s median %9.3f ms (min %9.3f, max %9.3f)" % (nm, statistics.median(times[k]), min(times[k]), max(times[k])))
    print("  %-18s median %9.3f ms   %7.2f GB  %5.2f TB/s = %.3f of the 8 TB/s roofline; %.4f ms per circuit"
          % (what, med, moved / 1e9, moved / med / 1e9, moved / (med * 1e-3) / HBM, med / B))


def run(montgomery):
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    rep = (lambda v: v * R256 % P) if montgomery else (lambda v: v)
    dom = H.EvaluationDomain(chip, 1, 1, rep(P - 1), rep(1))                            # the openings use no root of unity
    cols = [(columns(B) if per_circuit else columns(), mask) for per_circuit, mask in PATTERN]
    points = [[rep(pow(5 + p, 3 + e, P)) for p in range(4)] for e in range(B)]
    vs = [rep(pow(11, 7 + e, P)) for e in range(B)]
    queries = sum(bin(m).count("1") for _, m in PATTERN)
    per_circuit = sum(1 for pc, _ in PATTERN if pc)
    print("%s ctx: %d circuits, n = 2^%d; %d columns (%d per circuit, %d of the key), %d queries; %d timed calls"
          % ("Montgomery" if montgomery else "canonical", B, LOG_N, len(PATTERN), per_circuit, len(PATTERN) - per_circuit, queries, REPS))
    col_bytes = N * 32

    h = columns(B, PIECES)
    folded, status = torch.empty((B, N, 32), dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    t = timed(lambda: dom.fold(h, vs, out=(folded, status)), [_lib.KERNEL_FOLD])
    report("fold (%d pieces)" % PIECES, [], t, B * (PIECES + 1) * col_bytes)            # ASSUMED: every piece read once, the folded h written once
    del h, folded

    evals = torch.zeros((B, queries, 4), dtype=torch.int64, device="cuda")
    t = timed(lambda: dom.open_eval(cols, points, out=(evals, status)), [_lib.KERNEL_OPEN_TILES, _lib.KERNEL_OPEN_CARRY])
    report("open_eval", [(_lib.KERNEL_OPEN_TILES, "open_tiles_kernel"), (_lib.KERNEL_OPEN_CARRY, "open_carry_kernel")], t,
           (B * per_circuit + len(PATTERN) - per_circuit) * col_bytes)                  # ASSUMED: every column read once (the key's once in all)

    W = torch.empty((B, 4, N, 32), dtype=torch.uint8, device="cuda")
    be = torch.zeros((B, 4, 4), dtype=torch.int64, device="cuda")
    t = timed(lambda: dom.open_witness(cols, points, vs, out=(W, be, status)), [_lib.KERNEL_OPEN_TILES, _lib.KERNEL_OPEN_CARRY, _lib.KERNEL_OPEN_SCAN])
    report("open_witness", [(_lib.KERNEL_OPEN_TILES, "open_tiles_kernel"), (_lib.KERNEL_OPEN_CARRY, "open_carry_kernel"), (_lib.KERNEL_OPEN_SCAN, "open_scan_kernel")], t,
           (2 * B * queries + 4 * B) * col_bytes)                                       # ASSUMED: per circuit a column (the key's too) read once per query in each of two launches, W written once
    assert status.cpu().sum().item() == 0
    print(flush=True)
    del cols, W
    torch.cuda.empty_cache()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: every time below (HIP events stamped by the dispatch itself, medians over the timed calls; a call's time = the sum of its launches).")
    print("ASSUMED: the 8 TB/s HBM roofline (the data-sheet figure) and the byte counts: fold = every piece read once and the folded h written once;")
    print("         open_eval = every column read once (the proving key's columns once for the whole batch); open_witness = per circuit a column (a key column")
    print("         too) read once per query in the tiles launch and again in the scan launch, W written once.  No clock is read, and no figure below depends on one.")
    print(torch.cuda.get_device_name(0))
    for m in (False, True):
        run(m)
        torch.cuda.empty_cache()
