#!/usr/bin/env python3
"""Timing of the generator of the blinding values (h2r_random_columns) on the two shapes a k = 17 proof draws:
the vanishing argument's random polynomial -- one whole column of 2^17 elements per circuit -- and the tails: rows u..n of the 15 advice,
A' and S' columns and u+1..n of the 8 Z columns (two calls).  Batches of 1 and 8 circuits, canonical and Montgomery ctx; whole columns
also eight at a time, to see the rate once the device is full.
Per call: the events the dispatch itself stamps (h2r_profile_*) and two events on the stream around the call, medians over the timed
calls after one untimed call.  The rate is elements over the kernel's own time; one element is one BLAKE2b compression, a 512-bit
reduction (two Montgomery products) and 32 bytes stored, so the bytes written over the kernel's time are given next to it.  Element 0,
a middle one and the last one of every timed column are compared with hashlib.
No threshold: there is no earlier device implementation and nothing rests on these numbers.
    python tools/random_columns_timing.py [calls] > profiles/random_columns.txt"""
import hashlib
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib, prover

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
K, BF = 17, 5
N, U = 1 << K, (1 << K) - BF - 1
SEED = bytes(range(32))


def model(circuit, tag, row, montgomery):
    msg = SEED + circuit.to_bytes(8, "little") + tag.to_bytes(4, "little") + bytes(4) + row.to_bytes(8, "little")
    v = int.from_bytes(hashlib.blake2b(msg, digest_size=64, person=b"H2R-Blinding-v1\0").digest(), "little") % R
    return ((v << 256) % R if montgomery else v).to_bytes(32, "little")


def timed(chip, calls, elements, label, check):
    """calls: [(columns, tags, rows)] enqueued back to back = one draw."""
    def draw():
        for cols, tags, rows in calls:
            prover.random_columns(chip, cols, tags, rows, SEED)
    draw()                                                                        # untimed: code objects
    torch.cuda.synchronize()
    for cols, tags, rows in calls:
        for t, tag in zip(cols, tags):
            for e in {0, t.shape[0] - 1}:
                for row in {rows[0], (rows[0] + rows[1]) // 2, rows[1] - 1}:
                    assert bytes(t[e, row].cpu().numpy()) == model(e, tag, row, check), "the device and hashlib disagree"
    _lib.profile_enable(REPS * len(calls))
    stream_ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        draw()
        b.record()
        torch.cuda.synchronize()
        stream_ms.append(a.elapsed_time(b))
    per_launch = _lib.profile_read(_lib.KERNEL_RANDOM)
    _lib.profile_enable(0)
    assert len(per_launch) == REPS * len(calls)
    kernel_ms = [sum(per_launch[r * len(calls):(r + 1) * len(calls)]) for r in range(REPS)]
    km = statistics.median(kernel_ms)
    print("    %-58s %9d elements: kernel %8.4f ms median (min %.4f, max %.4f) = %7.2f G elements/s, %6.1f GB/s stored; stream %8.4f ms median"
          % (label, elements, km, min(kernel_ms), max(kernel_ms), elements / km / 1e6, elements * 32 / km / 1e6, statistics.median(stream_ms)))


def run(montgomery):
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    print("%s ctx (%d timed calls after one untimed)" % ("Montgomery" if montgomery else "canonical", REPS))
    for batch in (1, 8):
        poly = [torch.empty((batch, N, 32), dtype=torch.uint8, device="cuda")]
        timed(chip, [(poly, [0x500], (0, N))], batch * N, "batch %d: the random polynomial, one column of 2^17" % batch, montgomery)
        cols15 = [torch.zeros((batch, N, 32), dtype=torch.uint8, device="cuda") for _ in range(15)]
        cols8 = [torch.zeros((batch, N, 32), dtype=torch.uint8, device="cuda") for _ in range(8)]
        timed(chip, [(cols15, list(range(15)), (U, N)), (cols8, [0x300 + i for i in range(8)], (U + 1, N))], batch * (15 * (N - U) + 8 * (N - U - 1)),
              "batch %d: the tails of 15 + 8 columns, two calls" % batch, montgomery)
        del cols15, cols8
        eight = [torch.empty((batch, N, 32), dtype=torch.uint8, device="cuda") for _ in range(8)]
        timed(chip, [(eight, list(range(8)), (0, N))], batch * 8 * N, "batch %d: eight whole columns of 2^17, one call" % batch, montgomery)
        del eight, poly
    print(flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: per call the HIP events stamped by the dispatch itself (kernel) and two events on the stream around the call (stream); medians over the timed")
    print("calls after one untimed call.  Shape: k = 17, %d blinding factors: tails of %d and %d rows.  Rates are elements, and bytes stored, over the kernel's time." % (BF, N - U, N - U - 1))
    print(torch.cuda.get_device_name(0))
    for m in (False, True):
        run(m)
