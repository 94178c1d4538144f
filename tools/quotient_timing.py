#!/usr/bin/env python3
"""Timing of the vanishing argument's quotient (h2r_quotient_columns): 256 circuits at k = 17 on the extended domain of 2^19 points, five
advice columns plus one extra permutation column in sets of chunk_len = 2 (three Z columns), all five lookup arguments, 15 fixed columns;
random field elements (an unsatisfied circuit: the work per point does not depend on the values), canonical and Montgomery ctx.  Times are
the events the dispatch itself stamps (h2r_profile_*), after three untimed calls.  Next to each: the bytes under the ASSUMPTION "every
column read once, h written once" (the key columns once for the whole batch; rotated reads and the re-reads of advice cells counted as
hits) and that traffic against the 8 TB/s HBM roofline.  No threshold: there is no earlier implementation to compare with.
    python tools/quotient_timing.py [circuits] [repetitions] > profiles/quotient.txt"""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import lib
import ntt_ref as NR
import permutation_ref as PR

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
K, EK, BLINDING = 17, 19, 5
COLUMN_SRC, CHUNK_LEN, LOOKUP_MASK, NUM_FIXED = (0, 1, 2, 3, 4, 5), 2, 31, 15
GATE_FIXED, TABLE_TAG, TABLE_VALUE = tuple(range(9)), 9, 10
LOOKUP_ADVICE, LOOKUP_TAG, LOOKUP_ENABLE = (0, 1, 2, 3, 0), (11, 11, 11, 11, 13), (12, 12, 12, 12, 14)
P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R256 = 1 << 256
HBM = 8.0e12
N = 1 << EK


def columns(*lead):
    t = torch.randint(0, 256, lead + (N, 32), dtype=torch.uint8, device="cuda")
    t[..., 31] &= 0x0F                                                                  # below 2^252 < p: field elements in either representation
    return t


def run(montgomery):
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    rep = (lambda v: v * R256 % P) if montgomery else (lambda v: v)
    dom = H.EvaluationDomain(chip, K, EK, rep(NR.omega_of(P, EK)), rep(NR.cube_root_of_unity(P)))
    delta = rep(PR.domain(P, K)[1])
    sets = -(-len(COLUMN_SRC) // CHUNK_LEN)
    groups = dict(advice=columns(B, 5), extra=columns(B, 1), perm_z=columns(B, sets), lookup_a_perm=columns(B, 5), lookup_s_perm=columns(B, 5),
                  lookup_z=columns(B, 5), fixed=columns(NUM_FIXED), sigma=columns(len(COLUMN_SRC)), l=columns(3))
    h = torch.empty((B, N, 32), dtype=torch.uint8, device="cuda")
    status = torch.zeros(B, dtype=torch.uint8, device="cuda")
    ch = [[rep(pow(7 + i, 5 + e, P)) for e in range(B)] for i in range(4)]

    def call():
        dom.quotient(BLINDING, delta, GATE_FIXED, COLUMN_SRC, CHUNK_LEN, groups["advice"], groups["perm_z"], groups["fixed"], groups["sigma"], groups["l"],
                     *ch, extra=groups["extra"], lookup_mask=LOOKUP_MASK, lookup_advice=LOOKUP_ADVICE, lookup_tag=LOOKUP_TAG, lookup_enable=LOOKUP_ENABLE,
                     table_tag=TABLE_TAG, table_value=TABLE_VALUE, lookup_a_perm=groups["lookup_a_perm"], lookup_s_perm=groups["lookup_s_perm"],
                     lookup_z=groups["lookup_z"], out=(h, status))

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    assert status.cpu().sum().item() == 0
    _lib.profile_enable(4 * REPS)
    for _ in range(REPS):
        call()
        torch.cuda.synchronize()
    t = [float(x) for x in _lib.profile_read(_lib.KERNEL_QUOTIENT)]
    _lib.profile_enable(0)
    assert len(t) == REPS, len(t)
    # the columns the call reads, from the library itself
    cfg = _lib.H2RQuotientConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    cfg.log_n, cfg.log_ext, cfg.blinding_factors, cfg.num_fixed = K, EK, BLINDING, NUM_FIXED
    cfg.num_columns, cfg.chunk_len, cfg.n_extra, cfg.lookup_mask, cfg.table_tag, cfg.table_value = len(COLUMN_SRC), CHUNK_LEN, 1, LOOKUP_MASK, TABLE_TAG, TABLE_VALUE
    for i in range(9):
        cfg.gate_fixed[i] = GATE_FIXED[i]
    for i, s in enumerate(COLUMN_SRC):
        cfg.column_src[i] = s
    for k in range(5):
        cfg.lookup_advice[k], cfg.lookup_tag[k], cfg.lookup_enable[k] = LOOKUP_ADVICE[k], LOOKUP_TAG[k], LOOKUP_ENABLE[k]
    per, key = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib().h2r_quotient_sets(ctypes.byref(cfg), ctypes.byref(per), ctypes.byref(key)) == sets
    moved = (B * (per.value + 1) + key.value) * N * 32                                  # ASSUMED: every column read once (the key's once in all), h written once
    med = statistics.median(t)
    print("%s ctx: %d circuits, k = %d, 2^%d points; per circuit %d columns + h, %d key columns; %d timed calls"
          % ("Montgomery" if montgomery else "canonical", B, K, EK, per.value, key.value, REPS))
    print("  quotient_kernel  median %9.3f ms (min %9.3f, max %9.3f)   %7.2f GB  %5.2f TB/s = %.3f of the 8 TB/s roofline; %.4f ms per circuit, %.2f ns per point"
          % (med, min(t), max(t), moved / 1e9, moved / med / 1e9, moved / (med * 1e-3) / HBM, med / B, med * 1e6 / (B * N)))
    print(flush=True)
    del groups, h
    torch.cuda.empty_cache()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: every time below (HIP events stamped by the dispatch itself, medians over the timed calls).")
    print("ASSUMED: the 8 TB/s HBM roofline (the data-sheet figure) and the byte count: every column read once (the proving key's columns once for the")
    print("         whole batch), h written once; no clock is read, and no figure below depends on one.")
    print(torch.cuda.get_device_name(0))
    for m in (False, True):
        run(m)
        torch.cuda.empty_cache()
