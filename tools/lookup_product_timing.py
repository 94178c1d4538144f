#!/usr/bin/env python3
"""Timing of the lookup argument's input columns and grand product (h2r_lookup_input_columns / h2r_lookup_product_columns): 256 circuits x 5
arguments at usable_rows = 2^17 - 6, canonical and Montgomery ctx.  Per launch (the events the dispatch itself stamps, h2r_profile_*) after three
untimed calls of each export; every launch as a fraction of the 8 TB/s HBM roofline on its algorithmic bytes, the product launches also as
Montgomery products per second against the v_mad_u64_u32 issue rate (4.8 cycles per wave instruction; clock assumed 2.4 GHz).
    python tools/lookup_product_timing.py [circuits] [repetitions] > profiles/lookup_product.txt"""
import os
import random
import re
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import ctypes
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
USABLE = (1 << 17) - 6
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HBM = 8.0e12
# This tool's own count of a 256-bit Montgomery product in 32-bit digits: 8 x 8 digit products + 8 x 8 reduction products + 8 quotient digits = 136
# multiply-adds.  DESIGN section 4 quotes 4.8 cycles per v_mad_u64_u32 wave instruction and SIMD; the 2.4 GHz clock is ASSUMED (the peak engine
# clock, not read from the device), so the issue-rate fractions below are lower bounds of what the kernels reach at the clock they really ran at.
CLOCK, MADS_PER_PRODUCT = 2.4e9, 136
PEAK_PRODUCTS = 256 * 4 * 64 * CLOCK / 4.8 / MADS_PER_PRODUCT
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "halo2_rsa_amd", "csrc", "h2r_grand_product.hpp")) as f:
    TILE = int(re.search(r"GRAND_PRODUCT_TILE = (\d+);", f.read()).group(1))
# Montgomery products per lane (four rows) that the algorithm needs, (Montgomery ctx, + the conversions of a canonical ctx):
#   tiles: n, d of four rows 8 (+12 loads into the domain), the lane's two products 6, the wave's two reductions 12
#   scan:  n, d 8 (+12), serial scans 6, wave scans 12, the waves' carries 3, the lane's carries 2, Z of four rows 11 (+4 stores out of the domain)
PRODUCTS = {"tiles": (26, 12), "scan": (42, 16)}
KERNELS = [("input", _lib.KERNEL_LOOKUP_INPUT), ("tiles", _lib.KERNEL_LOOKUP_PRODUCT_TILES), ("carry", _lib.KERNEL_LOOKUP_PRODUCT_CARRY),
           ("scan", _lib.KERNEL_LOOKUP_PRODUCT_SCAN)]


def run(montgomery):
    chip = H.BigIntChip(64, 2048, montgomery=montgomery)
    la = H.LookupArgument(chip, rsa_chip=False)
    rng = random.Random(1)
    N = [rng.getrandbits(2048) | (1 << 2047) | 1 for _ in range(B)]
    X = [rng.randrange(n) for n in N]
    res = chip.pow_mod_fixed_exp(chip.assign_integer(X), 65537, chip.assign_integer(N), check_in_field=True)
    pl = res.trace.pow_layout
    k_pow = np.zeros(int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl))), dtype=np.uint8)
    assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k_pow.ctypes.data) == 0
    kinds = np.concatenate([chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True), k_pow])
    image = res.emit_modpow_advice()
    torch.cuda.synchronize()
    del res
    torch.cuda.empty_cache()
    hist = la.hist_advice(kinds, image, B, la.new_hist(B))
    ch = [[rng.randrange(P) for _ in range(B)] for _ in range(3)]      # (field elements in the ctx's representation, whichever it is)
    a_perm, s_perm, st = la.permuted_columns(hist, ch[0], USABLE)
    a_in = torch.empty((B, 5, USABLE, 32), dtype=torch.uint8, device="cuda")
    z = torch.empty((B, 5, USABLE + 1, 32), dtype=torch.uint8, device="cuda")
    zst = torch.zeros(B, dtype=torch.uint8, device="cuda")

    # the C exports themselves on buffers built once: nothing of the host (challenge uploads, allocations) lies inside a timed window
    kd = torch.from_numpy(np.ascontiguousarray(kinds)).cuda()
    th, be, ga = (H._marshal.challenges(v, "cuda", B) for v in ch)
    ws = torch.empty(int(lib().h2r_lookup_product_workspace_bytes(USABLE, B)), dtype=torch.uint8, device="cuda")
    col, stream = (USABLE + 1) * 32, chip._stream()

    def inputs():
        _lib.check(lib().h2r_lookup_input_columns(chip._ctx, ctypes.byref(la.cfg), None, kd.data_ptr(), kd.numel(), image.data_ptr(), image.shape[1], B, None,
                                                  th.data_ptr(), USABLE, 0, 31, a_in.data_ptr(), 5 * USABLE * 32, stream), "h2r_lookup_input_columns")

    def product():
        _lib.check(lib().h2r_lookup_product_columns(chip._ctx, ctypes.byref(la.cfg), a_in.data_ptr(), a_perm.data_ptr(), s_perm.data_ptr(), 5 * USABLE * 32,
                                                    th.data_ptr(), be.data_ptr(), ga.data_ptr(), B, USABLE, 31, z.data_ptr(), 5 * col, col, zst.data_ptr(),
                                                    ws.data_ptr(), stream), "h2r_lookup_product_columns")

    for _ in range(3):
        inputs()
        product()
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not zst.cpu().numpy().any(), "the argument is not well formed"
    _lib.profile_enable(8 * REPS)
    whole = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        product()
        b.record()
        inputs()
        torch.cuda.synchronize()
        whole.append(a.elapsed_time(b))
    ms = {name: [float(x) for x in _lib.profile_read(k)] for name, k in KERNELS}
    _lib.profile_enable(0)
    rows = B * 5 * USABLE
    bytes_ = {"input": rows * 32, "tiles": rows * 96, "carry": 0, "scan": rows * 128}
    print("%s ctx: %d circuits x 5 arguments x %d rows (image %d rows), tile %d rows, %d timed calls" %
          ("Montgomery" if montgomery else "canonical", B, USABLE, len(kinds), TILE, REPS))
    for name, _ in KERNELS:
        t = ms[name]
        med = statistics.median(t)
        line = "  %-6s median %7.3f ms (min %7.3f, max %7.3f)" % (name, med, min(t), max(t))
        if bytes_[name]:
            line += "   %6.2f GB  %5.2f TB/s = %.3f of the 8 TB/s roofline" % (bytes_[name] / 1e9, bytes_[name] / med / 1e9, bytes_[name] / (med * 1e-3) / HBM)
        if name in PRODUCTS:
            per_lane = PRODUCTS[name][0] + (0 if montgomery else PRODUCTS[name][1])
            rate = rows / 4 * per_lane / (med * 1e-3)
            line += "   %.1f products/row, %.3g products/s = %.3f of the v_mad_u64_u32 issue rate (%.3g/s at 2.4 GHz)" % (per_lane / 4, rate, rate / PEAK_PRODUCTS, PEAK_PRODUCTS)
        print(line)
    three = [sum(ms[n][i] for n in ("tiles", "carry", "scan")) for i in range(REPS)]
    med = statistics.median(whole)
    print("  product, the three launches summed: median %.3f ms; the whole call (events around it): median %.3f ms = %.3f of the roofline on %.2f GB"
          % (statistics.median(three), med, rows * 224 / (med * 1e-3) / HBM, rows * 224 / 1e9))
    print(flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print(torch.cuda.get_device_name(0))
    for m in (False, True):
        run(m)
        torch.cuda.empty_cache()
