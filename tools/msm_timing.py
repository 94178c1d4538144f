#!/usr/bin/env python3
"""Timing of the commitments (h2r_msm_columns): n = 2^17 points, 30 columns per circuit, 1 and 8 circuits, canonical
and Montgomery ctx, three distributions of the scalars:
    uniform    random field elements (every window digit uniform)
    ones       every scalar 1 (one bucket of one window holds every point; every other digit is zero)
    recorded   the columns of recorded RSA-2048 emit_modpow_advice images (planar, the ctx's representation): short integers, runs of
               equal values and constants -- what an advice commitment really sees.  An image has five columns of `rows` rows; a column is
               repeated up to n where rows < n, and the 30 columns of a circuit are the columns of six recorded elements.
The bases are 4,096 points of bn256 G1 repeated to n (repeats are legal input and cost what distinct points cost).  Times are the events
the dispatch itself stamps (h2r_profile_*), per launch, after three untimed calls.  Reported: time per column, bucket additions per second
(one mixed addition per NON-ZERO window digit, counted on the canonical form of the same scalars; for the uniform Montgomery columns the
canonical count of the same size is used), and per (ctx, batch) the slowest distribution's time over the uniform one's -- the evidence for
the skew bound.  No threshold: there is no earlier implementation, and upstream's best_multiexp is not here to compare with.
    python tools/msm_timing.py [repetitions] > profiles/msm.txt"""
import os
import random
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib
import msm_ref as M

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LOG_N, COLS, BLOCK, PER_IMAGE = 17, 30, 4096, 5
N = 1 << LOG_N
P = M.R_ORDER
R256 = 1 << 256


def timed(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    _lib.profile_enable(8 * REPS)
    for _ in range(REPS):
        call()
        torch.cuda.synchronize()
    out = {k: [float(x) for x in _lib.profile_read(k)] for k in (_lib.KERNEL_MSM_BUCKET, _lib.KERNEL_MSM_FOLD)}
    _lib.profile_enable(0)
    assert all(len(t) == REPS for t in out.values()), {k: len(t) for k, t in out.items()}
    return out


def uniform(batch):
    t = torch.randint(0, 256, (batch, COLS, N, 32), dtype=torch.uint8, device="cuda")
    t[..., 31] &= 0x0F                                                                  # below 2^252 < p: field elements in either representation
    return t


def ones(batch, montgomery):
    one = (R256 % P if montgomery else 1).to_bytes(32, "little")
    return torch.frombuffer(bytearray(one), dtype=torch.uint8).cuda().expand(batch, COLS, N, 32).contiguous()


def recorded(batch, montgomery):
    """[batch, COLS, N, 32] from batch * COLS / 5 recorded elements; also the image's row count."""
    chip = H.BigIntChip(64, 2048, columns=True, montgomery=montgomery)
    elems = batch * COLS // PER_IMAGE
    rng = random.Random(17)
    mod = [rng.getrandbits(2048) | (1 << 2047) | 1 for _ in range(elems)]
    x = [rng.randrange(n) for n in mod]
    res = chip.pow_mod_fixed_exp(chip.assign_integer(x), 65537, chip.assign_integer(mod), check_in_field=True)
    image = res.emit_modpow_advice()
    torch.cuda.synchronize()
    rows = image.shape[1] // 160
    cols = image.view(elems * PER_IMAGE, rows, 32)                                      # planar: an element's five columns follow each other
    reps = -(-N // rows)
    out = cols.repeat(1, reps, 1)[:, :N].reshape(batch, COLS, N, 32).contiguous()
    del res, image
    return out, rows


def nonzero_digits(t):
    return int((t != 0).sum().item())


def run(montgomery, batch, bases, counts):
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    ck = H.CommitKey(chip, torch.frombuffer(bytearray(M.point_bytes(bases, montgomery) * (N // BLOCK)), dtype=torch.uint8).reshape(N, 64).cuda())
    info = ck.plan(COLS, batch)
    print("%s ctx, %d circuit(s): n = 2^%d, %d columns; windows %d x %d bits, slices %d x %d points, workspace %.1f MB; %d timed calls"
          % ("Montgomery" if montgomery else "canonical", batch, LOG_N, COLS, info.num_windows, info.window_bits, info.num_slices, info.slice_points,
             info.workspace_bytes / 1e6, REPS))
    out = torch.zeros((batch, COLS, 2, 4), dtype=torch.int64, device="cuda")
    ws = torch.empty(info.workspace_bytes, dtype=torch.uint8, device="cuda")
    totals = {}
    for name in ("uniform", "ones", "recorded"):
        if name == "uniform":
            t = uniform(batch)
        elif name == "ones":
            t = ones(batch, montgomery)
        else:
            t, rows = recorded(batch, montgomery)
        if not montgomery:
            counts[(name, batch)] = nonzero_digits(t)                                    # the canonical bytes are the window digits
        adds = counts[(name, batch)]
        columns = [t[:, c] for c in range(COLS)]
        ms = timed(lambda: ck.commit(columns, out=out, workspace=ws))
        total = [ms[_lib.KERNEL_MSM_BUCKET][i] + ms[_lib.KERNEL_MSM_FOLD][i] for i in range(REPS)]
        med, bucket = statistics.median(total), statistics.median(ms[_lib.KERNEL_MSM_BUCKET])
        totals[name] = med
        note = " (image of %d rows)" % rows if name == "recorded" else ""
        print("  %-9s bucket %9.3f ms (min %9.3f, max %9.3f)  fold %7.3f ms  call %9.3f ms = %8.4f ms per column; %.4g non-zero digits, %.3g bucket additions/s%s"
              % (name, bucket, min(ms[_lib.KERNEL_MSM_BUCKET]), max(ms[_lib.KERNEL_MSM_BUCKET]), statistics.median(ms[_lib.KERNEL_MSM_FOLD]), med,
                 med / (COLS * batch), adds, adds / (bucket * 1e-3), note))
        del t, columns
        torch.cuda.empty_cache()
    slow = max(totals, key=totals.get)
    print("  slowest over uniform: %.3f (%s)" % (totals[slow] / totals["uniform"], slow))
    print(flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: every time below (HIP events stamped by the dispatch itself, medians over the timed calls; a call's time = its two launches).")
    print("COUNTED: the non-zero window digits (= mixed additions of the bucket kernel), on the canonical form of the scalars.  No clock is read.")
    print(torch.cuda.get_device_name(0))
    bases = M.structured_bases(BLOCK, 0x1234567890abcdef, 0xfedcba987654321)
    counts = {}
    for batch in (1, 8):
        for m in (False, True):
            run(m, batch, bases, counts)
            torch.cuda.empty_cache()
