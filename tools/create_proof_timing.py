#!/usr/bin/env python3
"""Timing of prover.create_proof on recorded circuits: the k = 9 mul_mod image of the tests (the smallest k they use)
and the k = 17 image of one RSA-2048, e = 65537 modpow_public_key element (77,040 rows), batches of 1 and 8 circuits, Montgomery ctx.
Total: the stream time of one create_proof between two events on the stream.  Per stage: the events the dispatch itself stamps
(h2r_profile_*), summed per kernel class over one proof -- transforms, quotient, commitments, openings and fold, grand products, lookup
columns, transcript, generator; what is left of the total is launch gaps and torch's copies.  Medians over the timed proofs after one
untimed proof.  The keys' fixed and sigma columns come from the tests' plain helpers (tests/prover_chain_ref.py); the bases are
structured points, not powers of tau: a timing needs no opening to verify.  Every status is checked to be 0: a skipped circuit would
time nothing.  No comparison figure exists (the reference's prover cannot be built here) and nothing rests on these numbers.
    python tools/create_proof_timing.py [proofs] > profiles/create_proof.txt"""
import ctypes
import os
import random
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib, prover
from halo2_rsa_amd._lib import lib
import advice_ref as AR
import msm_ref as M
import permutation_ref as PR
import prover_chain_ref as CR

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
P = M.R_ORDER
R256 = 1 << 256
BF = 5
STAGES = (("generator", (_lib.KERNEL_RANDOM,)), ("transcript", (_lib.KERNEL_TRANSCRIPT,)),
          ("lookup columns", (_lib.KERNEL_LOOKUP, _lib.KERNEL_LOOKUP_INPUT, _lib.KERNEL_HIST)),
          ("grand products", (_lib.KERNEL_LOOKUP_PRODUCT_TILES, _lib.KERNEL_LOOKUP_PRODUCT_CARRY, _lib.KERNEL_LOOKUP_PRODUCT_SCAN,
                              _lib.KERNEL_PERM_PRODUCT_TILES, _lib.KERNEL_PERM_PRODUCT_CARRY, _lib.KERNEL_PERM_PRODUCT_SCAN)),
          ("transforms", (_lib.KERNEL_NTT_SETUP, _lib.KERNEL_NTT_PASS)), ("quotient", (_lib.KERNEL_QUOTIENT,)),
          ("commitments", (_lib.KERNEL_MSM_BUCKET, _lib.KERNEL_MSM_FOLD)),
          ("openings and fold", (_lib.KERNEL_OPEN_TILES, _lib.KERNEL_OPEN_CARRY, _lib.KERNEL_OPEN_SCAN, _lib.KERNEL_FOLD)))


def columns_tensor(cols):
    """[[canonical integers]] -> uint8 [C, n, 32] in Montgomery form on the device."""
    out = np.empty((len(cols), len(cols[0]), 4), dtype=np.uint64)
    for c, col in enumerate(cols):
        for i, v in enumerate(col):
            v = v * R256 % P
            out[c, i] = (v & 0xFFFFFFFFFFFFFFFF, (v >> 64) & 0xFFFFFFFFFFFFFFFF, (v >> 128) & 0xFFFFFFFFFFFFFFFF, v >> 192)
    return torch.from_numpy(out.view(np.uint8).reshape(len(cols), len(cols[0]), 32)).cuda()


def recorded(w, L, e, k, batch):
    """A chip, the image of `batch` modpow_public_key elements, and the key of their circuit at 2^k rows."""
    chip = H.BigIntChip(w, w * L, field="bn254_fr", montgomery=True)
    rng = random.Random("create_proof/timing/%d" % k)
    mods = [rng.getrandbits(w * L) | (1 << (w * L - 1)) | 1 for _ in range(batch)]
    res = chip.pow_mod_fixed_exp(chip.assign_integer([rng.randrange(m) for m in mods]), e, chip.assign_integer(mods), check_in_field=True)
    pl = res.trace.pow_layout
    k_if = chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True)
    k_pow = np.zeros(int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl))), dtype=np.uint8)
    assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k_pow.ctypes.data) == 0
    kinds = np.concatenate([k_if, k_pow])
    pairs = [(c.row, c.col, c.src_row, c.src_col) for c in chip.pow_copy_map(pl, e, row_offset=len(k_if))]
    n = 1 << k
    assert len(kinds) <= n - BF - 1
    lcfg = AR.LookupConfig(AR.range_lens(w, L))
    cfg = CR.config(P, k, BF)
    fixed = CR.fixed_columns(CR.fixed_rows_of(kinds, w, L, lcfg), lcfg.table(), n, 0, P)
    sigma = PR.sigma_from_pairs(pairs, 5, n, cfg.delta, cfg.omega(P), P)
    rep = lambda v: v * R256 % P
    dom = H.EvaluationDomain(chip, k, k + 3, rep(cfg.omega_ext), rep(cfg.zeta))
    bases = torch.frombuffer(bytearray(M.point_bytes(M.structured_bases(n, 12345, 67891), True)), dtype=torch.uint8).reshape(n, 64).cuda()
    key = prover.ProvingKey(chip, dom, H.CommitKey(chip, bases), H.LookupArgument(chip, rsa_chip=False), columns_tensor(fixed), columns_tensor(sigma), kinds, BF,
                            rep(cfg.delta), cfg.gate_fixed, cfg.column_src, cfg.chunk_len, cfg.lookup_advice, cfg.lookup_tag, cfg.lookup_enable,
                            cfg.table_tag, cfg.table_value, rep(0xC0FFEE))
    return key, res.emit_modpow_advice(), len(kinds)


def measure(label, key, image, batch):
    seed = bytes(range(32))
    _, status = prover.create_proof(key, image, batch, seed=seed)                  # untimed: code objects, allocator
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * batch, "a circuit was flagged: %s" % status.cpu().tolist()
    total, per_stage = [], {name: [] for name, _ in STAGES}
    for _ in range(REPS):
        _lib.profile_enable(1 << 14)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        prover.create_proof(key, image, batch, seed=seed)
        b.record()
        torch.cuda.synchronize()
        total.append(a.elapsed_time(b))
        for name, classes in STAGES:
            per_stage[name].append(sum(sum(_lib.profile_read(c)) for c in classes))
        _lib.profile_enable(0)
    med = {name: statistics.median(v) for name, v in per_stage.items()}
    print("%s, batch %d: create_proof %9.3f ms of stream time, median (min %.3f, max %.3f; %d timed proofs after one untimed); kernels' own events summed %.3f ms"
          % (label, batch, statistics.median(total), min(total), max(total), REPS, sum(med.values())))
    print("    per stage, ms: " + "; ".join("%s %.3f" % (name, med[name]) for name, _ in STAGES), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: two events on the stream around one create_proof (total); per stage the HIP events stamped by each dispatch, summed per kernel class over the proof.")
    print("Montgomery ctx, bn254_fr, %d blinding factors, extended domain 2^(k+3), 60 evaluations, %d proof bytes per circuit." % (BF, 2944))
    print(torch.cuda.get_device_name(0), flush=True)
    for label, (w, L, e, k) in (("k = 10 (64 x 4 limbs, e = 1: 746 rows)", (64, 4, 1, 10)), ("k = 17 (RSA-2048, e = 65537)", (64, 32, 65537, 17))):
        key, image, rows = recorded(w, L, e, k, 8)                                # one key; the batch of 1 is the first circuit of the 8
        for batch in (1, 8):
            measure(label if "rows" in label else "%s: %d rows)" % (label[:-1], rows), key, image[:batch], batch)
        del key, image
        torch.cuda.empty_cache()
