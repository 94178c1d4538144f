#!/usr/bin/env python3
"""Timing of the permutation argument's grand product (h2r_permutation_product_columns): 256 RSA-2048 modpow_public_key images at
usable_rows = 2^17 - 6, six permutation columns (the five advice columns + one zero extra column) in three sets (chunk_len 2), canonical and
Montgomery ctx.  Per launch (the events the dispatch itself stamps, h2r_profile_*) after three untimed calls; every launch as a fraction of the
8 TB/s HBM roofline on its algorithmic bytes.  The sigma columns are the identity (no copy pair: the kernels do the same work whatever
sigma holds, and the argument is then trivially satisfied, status 0).  The lookup product's launches are measured in the same process on
the same images: its time per Z column is the yardstick for the time per Z column here.
    python tools/permutation_product_timing.py [circuits] [repetitions] > profiles/permutation_product.txt"""
import os
import random
import re
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
import torch
import ctypes
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
import permutation_ref as PR

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
K = 17
USABLE = (1 << K) - 6
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R256 = 1 << 256
HBM = 8.0e12
SRC, CHUNK = (0, 1, 2, 3, 4, 5), 2
M, SETS = len(SRC), 3
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "halo2_rsa_amd", "csrc", "h2r_grand_product.hpp")) as f:
    TILE = int(re.search(r"GRAND_PRODUCT_TILE = (\d+);", f.read()).group(1))
PERM = [("tiles", _lib.KERNEL_PERM_PRODUCT_TILES), ("carry", _lib.KERNEL_PERM_PRODUCT_CARRY), ("scan", _lib.KERNEL_PERM_PRODUCT_SCAN)]
LOOKUP = [("tiles", _lib.KERNEL_LOOKUP_PRODUCT_TILES), ("carry", _lib.KERNEL_LOOKUP_PRODUCT_CARRY), ("scan", _lib.KERNEL_LOOKUP_PRODUCT_SCAN)]


def fe_bytes(vals):
    out = np.empty((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        out[i] = [(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    return out.view(np.uint8).reshape(len(vals), 32)


def report(title, kernels, ms, bytes_, cols):
    print("  " + title)
    for name, _ in kernels:
        t = ms[name]
        med = statistics.median(t)
        line = "    %-6s median %7.3f ms (min %7.3f, max %7.3f)" % (name, med, min(t), max(t))
        if bytes_[name]:
            line += "   %6.2f GB  %5.2f TB/s = %.3f of the 8 TB/s roofline" % (bytes_[name] / 1e9, bytes_[name] / med / 1e9, bytes_[name] / (med * 1e-3) / HBM)
        print(line)
    three = [sum(ms[n][i] for n, _ in kernels) for i in range(len(ms["tiles"]))]
    med = statistics.median(three)
    total = sum(bytes_.values())
    print("    the three launches summed: median %.3f ms = %.3f of the roofline on %.2f GB; %.4f ms per Z column (%d columns)"
          % (med, total / (med * 1e-3) / HBM, total / 1e9, med / cols, cols))
    return med / cols


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
    rows = len(kinds)
    image = res.emit_modpow_advice()
    torch.cuda.synchronize()
    del res
    torch.cuda.empty_cache()
    stream = chip._stream()
    scale = R256 if montgomery else 1

    # ---- the permutation product: the C export itself on buffers built once ----
    omega, delta = PR.domain(P, K)
    pa = H.PermutationArgument(chip, SRC, CHUNK, delta * scale % P, omega * scale % P)
    assert pa.sets == SETS
    sigma = torch.from_numpy(np.stack([fe_bytes([x * scale % P for x in col]) for col in PR.labels(M, USABLE, delta, omega, P)])).cuda()
    extra = torch.zeros((1, 1, USABLE, 32), dtype=torch.uint8, device="cuda")          # one zero column, the same for every circuit (element stride 0)
    ch = [[rng.randrange(P) for _ in range(B)] for _ in range(3)]                      # (field elements in the ctx's representation, whichever it is)
    th, be, ga = (H._marshal.challenges(v, "cuda", B) for v in ch)
    pz = torch.empty((B, SETS, USABLE + 1, 32), dtype=torch.uint8, device="cuda")
    pst = torch.zeros(B, dtype=torch.uint8, device="cuda")
    pws = torch.empty(int(lib().h2r_permutation_product_workspace_bytes(ctypes.byref(pa.cfg), USABLE, B)), dtype=torch.uint8, device="cuda")
    col = (USABLE + 1) * 32

    def perm_product():
        _lib.check(lib().h2r_permutation_product_columns(chip._ctx, ctypes.byref(pa.cfg), image.data_ptr(), image.shape[1], rows, 0, B, extra.data_ptr(), 0,
                                                         USABLE * 32, sigma.data_ptr(), USABLE * 32, be.data_ptr(), ga.data_ptr(), USABLE, pz.data_ptr(),
                                                         SETS * col, col, pst.data_ptr(), pws.data_ptr(), stream), "h2r_permutation_product_columns")

    for _ in range(3):
        perm_product()
    torch.cuda.synchronize()
    assert not pst.cpu().numpy().any(), "the identity permutation is not satisfied"
    _lib.profile_enable(8 * REPS)
    for _ in range(REPS):
        perm_product()
        torch.cuda.synchronize()
    pms = {name: [float(x) for x in _lib.profile_read(k)] for name, k in PERM}
    _lib.profile_enable(0)
    del pz, pws
    torch.cuda.empty_cache()

    # ---- the lookup product on the same images, the same process ----
    hist = la.hist_advice(kinds, image, B, la.new_hist(B))
    a_perm, s_perm, st = la.permuted_columns(hist, ch[0], USABLE)
    a_in = la.input_columns(kinds, image, B, ch[0], USABLE)
    z = torch.empty((B, 5, USABLE + 1, 32), dtype=torch.uint8, device="cuda")
    zst = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(lib().h2r_lookup_product_workspace_bytes(USABLE, B)), dtype=torch.uint8, device="cuda")

    def lookup_product():
        _lib.check(lib().h2r_lookup_product_columns(chip._ctx, ctypes.byref(la.cfg), a_in.data_ptr(), a_perm.data_ptr(), s_perm.data_ptr(), 5 * USABLE * 32,
                                                    th.data_ptr(), be.data_ptr(), ga.data_ptr(), B, USABLE, 31, z.data_ptr(), 5 * col, col, zst.data_ptr(),
                                                    ws.data_ptr(), stream), "h2r_lookup_product_columns")

    for _ in range(3):
        lookup_product()
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not zst.cpu().numpy().any(), "the lookup argument is not well formed"
    _lib.profile_enable(8 * REPS)
    for _ in range(REPS):
        lookup_product()
        torch.cuda.synchronize()
    lms = {name: [float(x) for x in _lib.profile_read(k)] for name, k in LOOKUP}
    _lib.profile_enable(0)

    print("%s ctx: %d circuits x %d usable rows (image %d rows), tile %d rows, %d timed calls" %
          ("Montgomery" if montgomery else "canonical", B, USABLE, rows, TILE, REPS))
    # Algorithmic bytes of the permutation product, spelled out.  Per circuit: the image's five columns are read where the image has rows
    # (rows x 5 x 32; the other usable rows of an advice column read nothing), the extra column on every usable row (u x 32); sigma is SHARED by
    # the circuits and counted ONCE per call (m x u x 32: after the first circuit it is served from the caches); Z is written once (S x (u + 1) x 32).
    # The tiles launch reads, the scan launch reads the same again and writes Z; the carry launch moves two products per tile (not counted).
    reads = B * (rows * 5 * 32 + USABLE * 32) + M * USABLE * 32
    writes = B * SETS * (USABLE + 1) * 32
    per_perm = report("permutation product: %d columns in %d sets (chunk_len %d)" % (M, SETS, CHUNK), PERM, pms,
                      {"tiles": reads, "carry": 0, "scan": reads + writes}, B * SETS)
    lrows = B * 5 * USABLE
    per_look = report("lookup product: 5 arguments (the yardstick)", LOOKUP, lms, {"tiles": lrows * 96, "carry": 0, "scan": lrows * 128}, B * 5)
    print("  per Z column: permutation %.4f ms, lookup %.4f ms (ratio %.2f); a permutation column multiplies %d columns' terms per row, a lookup column one pair"
          % (per_perm, per_look, per_perm / per_look, CHUNK))
    print(flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: every time below (HIP events stamped by the dispatches themselves, medians over the timed calls).")
    print("ASSUMED: the 8 TB/s HBM roofline (the data-sheet figure) and the algorithmic byte counts spelled out in this tool; no clock is read,")
    print("         and no figure below depends on one.")
    print(torch.cuda.get_device_name(0))
    for m in (False, True):
        run(m)
        torch.cuda.empty_cache()
