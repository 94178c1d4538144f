#!/usr/bin/env python3
"""Timing of prover.verify_proof on proofs of the k = 10 recorded circuit (64 x 4 limbs, e = 1: 746 rows), batches of
1, 8 and 256 proofs, Montgomery ctx.  Total: the stream time of one verify_proof between two events on the stream.  Per launch class: the
events the dispatch itself stamps (h2r_profile_*) -- decoder (two launches), transcript (seven rounds), scalars, sums of terms (two).
Medians of the timed runs after one untimed run.  The eight proofs are create_proof's over a key of [tau^i]G, so the accumulators must
satisfy [tau] L = R (checked once, on the host model's curve); the batch of 256 repeats them (a verifier's work does not depend on the
bytes).  For scale only, the route tests/test_create_proof_gpu.py takes today: pull one proof to the host and run the plain-Python model
verifier on it.  No target is set and nothing rests on these numbers.
    python tools/verify_proof_timing.py [runs] > profiles/verify_proof.txt"""
import ctypes
import os
import random
import statistics
import sys
import time

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
import create_proof_ref as C
import msm_ref as M
import permutation_ref as PR
import prover_chain_ref as CR
import verify_proof_ref as V
from create_proof_timing import columns_tensor

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
P, R256, BF, W, L, E, K = M.R_ORDER, 1 << 256, 5, 64, 4, 1, 10
TAU, VK_REPR = random.Random("verify_proof/timing/tau").randrange(2, P), 0xC0FFEE
CLASSES = (("decoder", _lib.KERNEL_PROOF_DECODE), ("transcript", _lib.KERNEL_TRANSCRIPT), ("scalars", _lib.KERNEL_VERIFY_SCALARS), ("sums of terms", _lib.KERNEL_MSM_TERMS))


def recorded(batch):
    """The proving key of the recorded circuit over [tau^i]G, the image of `batch` elements, and the model's key of the same circuit."""
    chip = H.BigIntChip(W, W * L, field="bn254_fr", montgomery=True)
    rng = random.Random("verify_proof/timing")
    mods = [rng.getrandbits(W * L) | (1 << (W * L - 1)) | 1 for _ in range(batch)]
    res = chip.pow_mod_fixed_exp(chip.assign_integer([rng.randrange(m) for m in mods]), E, chip.assign_integer(mods), check_in_field=True)
    pl = res.trace.pow_layout
    k_if = chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True)
    k_pow = np.zeros(int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl))), dtype=np.uint8)
    assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k_pow.ctypes.data) == 0
    kinds = np.concatenate([k_if, k_pow])
    pairs = [(c.row, c.col, c.src_row, c.src_col) for c in chip.pow_copy_map(pl, E, row_offset=len(k_if))]
    n = 1 << K
    lcfg = AR.LookupConfig(AR.range_lens(W, L))
    cfg = CR.config(P, K, BF)
    fixed = CR.fixed_columns(CR.fixed_rows_of(kinds, W, L, lcfg), lcfg.table(), n, 0, P)
    sigma = PR.sigma_from_pairs(pairs, 5, n, cfg.delta, cfg.omega(P), P)
    rep = lambda v: v * R256 % P
    dom = H.EvaluationDomain(chip, K, K + 3, rep(cfg.omega_ext), rep(cfg.zeta))
    bases = torch.frombuffer(bytearray(M.point_bytes(M.mul_g_batch([pow(TAU, i, P) for i in range(n)]), True)), dtype=torch.uint8).reshape(n, 64).cuda()
    key = prover.ProvingKey(chip, dom, H.CommitKey(chip, bases), H.LookupArgument(chip, rsa_chip=False), columns_tensor(fixed), columns_tensor(sigma), kinds, BF,
                            rep(cfg.delta), cfg.gate_fixed, cfg.column_src, cfg.chunk_len, cfg.lookup_advice, cfg.lookup_tag, cfg.lookup_enable,
                            cfg.table_tag, cfg.table_value, rep(VK_REPR))
    return key, res.emit_modpow_advice(), C.Key(cfg, fixed, sigma, None, lcfg, 0, VK_REPR)


def measure(vk, proofs):
    batch = int(proofs.shape[0])
    _, _, status = prover.verify_proof(vk, proofs)                                 # untimed: code objects, allocator
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * batch
    total, per = [], {name: [] for name, _ in CLASSES}
    launches = {}
    for _ in range(REPS):
        _lib.profile_enable(1 << 10)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        prover.verify_proof(vk, proofs)
        b.record()
        torch.cuda.synchronize()
        total.append(a.elapsed_time(b))
        for name, cls in CLASSES:
            ms = _lib.profile_read(cls)
            per[name].append(sum(ms))
            launches[name] = len(ms)
        _lib.profile_enable(0)
    print("batch %3d: verify_proof %8.3f ms of stream time, median (min %.3f, max %.3f; %d timed runs after one untimed)"
          % (batch, statistics.median(total), min(total), max(total), REPS))
    print("    per launch class, ms: " + "; ".join("%s %.3f (min %.3f, max %.3f; %d launches)" % (name, statistics.median(per[name]), min(per[name]), max(per[name]), launches[name])
                                               for name, _ in CLASSES), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: two events on the stream around one verify_proof (total); per launch class the HIP events stamped by each dispatch, summed.")
    print("Montgomery ctx, bn254_fr, k = %d, %d blinding factors; G2 and the pairing are not part of the call." % (K, BF))
    print(torch.cuda.get_device_name(0), flush=True)
    key, image, model_key = recorded(8)
    proofs, status = prover.create_proof(key, image, 8, seed=bytes(range(32)))
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * 8
    vk = key.verifying_key()
    left, right, vstatus = prover.verify_proof(vk, proofs)
    torch.cuda.synchronize()
    Lp, Rp = (M.points_from_bytes(bytes(t[0].cpu().numpy()), True)[0] for t in (left, right))
    assert vstatus.cpu().tolist() == [0] * 8 and V.accepts(Lp, Rp, TAU), "the device's accumulators do not satisfy [tau] L = R"
    print("%d proof bytes, %d evaluations, %d bases of R per circuit" % (vk.proof_bytes, vk.num_evals, vk.num_bases))
    for batch in (1, 8, 256):
        measure(vk, proofs.repeat((batch + 7) // 8, 1)[:batch].contiguous())
    C.verify(model_key, bytes(proofs[0].cpu().numpy()), TAU)                       # untimed: the model key's commitments are made once
    t0 = time.perf_counter()
    raw = bytes(proofs[0].cpu().numpy())
    ok = C.verify(model_key, raw, TAU)
    print("for scale only -- the host route (pull one proof, the plain-Python model verifier): %.0f ms per proof, accepted = %s" % (1e3 * (time.perf_counter() - t0), ok))
