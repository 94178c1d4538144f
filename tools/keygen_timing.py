#!/usr/bin/env python3
"""Timing of key generation at the reference's size: one RSA-2048, e = 65537 modpow_public_key element, k = 17,
77,040 rows, five permutation columns, fifteen fixed columns, Montgomery ctx.
Device route (the code under test): the stream time of h2r_keygen_fixed_columns' launch, of h2r_keygen_sigma_columns per phase -- the
components (init, mark, hook / compress rounds, with the round count), the compaction, the sort passes, the write-out -- from the events
the dispatches stamp (h2r_profile_*), and of the two commit calls between two events on the stream; medians over the timed calls after
one untimed call.  The sigma call reads a word per round on the host, so its wall time is printed next to the sum of its kernels.
Host route (what callers did before prover.keygen: tests/permutation_ref.py::sigma_from_pairs + tests/prover_chain_ref.py::fixed_columns +
the upload, as tools/create_proof_timing.py does it): wall time, once, in the same process -- the parent's route, not the code under test.
The two keys' columns are compared byte for byte before any number is printed.  No target is set and nothing rests on these numbers.
    python tools/keygen_timing.py [calls] > profiles/keygen.txt"""
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
import msm_ref as M
import permutation_ref as PR
import prover_chain_ref as CR
from create_proof_timing import columns_tensor

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
P, R256, BF, W, L, E, K = M.R_ORDER, 1 << 256, 5, 64, 32, 65537, 17
PHASES = (("components", _lib.KERNEL_KEYGEN_COMPONENTS), ("compaction", _lib.KERNEL_KEYGEN_COMPACT), ("sort", _lib.KERNEL_KEYGEN_SORT),
          ("write-out", _lib.KERNEL_KEYGEN_WRITE))


def rep(v):
    return v * R256 % P


def stream_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: per launch the HIP events stamped by the dispatch (h2r_profile_*), summed per kernel class over one call; two events on the stream around the commit calls; host wall clock where stated.")
    print(torch.cuda.get_device_name(0), flush=True)
    chip = H.BigIntChip(W, W * L, field="bn254_fr", montgomery=True)
    rng = random.Random("keygen/timing")
    mod = rng.getrandbits(W * L) | (1 << (W * L - 1)) | 1
    res = chip.pow_mod_fixed_exp(chip.assign_integer([rng.randrange(mod)]), E, chip.assign_integer([mod]), check_in_field=True)
    pl = res.trace.pow_layout
    k_if = chip.fresh_op_row_kinds(_lib.FRESH_OPS.index("is_in_field"), assert_one=True)
    k_pow = np.zeros(int(lib().h2r_pow_advice_rows(chip._ctx, ctypes.byref(pl))), dtype=np.uint8)
    assert lib().h2r_pow_row_kinds(chip._ctx, ctypes.byref(pl), k_pow.ctypes.data) == 0
    kinds = np.concatenate([k_if, k_pow])
    copies = chip.pow_copy_map(pl, E, row_offset=len(k_if))
    n = 1 << K
    cfg = CR.config(P, K, BF)
    la = H.LookupArgument(chip, rsa_chip=False)
    dom = H.EvaluationDomain(chip, K, K + 3, rep(cfg.omega_ext), rep(cfg.zeta))
    bases = torch.frombuffer(bytearray(M.point_bytes(M.structured_bases(n, 12345, 67891), True)), dtype=torch.uint8).reshape(n, 64).cuda()
    ck = H.CommitKey(chip, bases)
    lk = dom.lagrange_key(ck)
    kinds_dev = torch.from_numpy(kinds).cuda()
    pairs_dev = prover.copy_pairs_tensor(copies, "cuda:0")
    delta = prover.field_delta(chip)
    print("k = %d, %d rows, %d copy pairs, m = 5, F = %d, Montgomery ctx, bn254_fr" % (K, len(kinds), len(copies), prover.NUM_FIXED), flush=True)

    # the host route, once: what a caller of ProvingKey did before keygen
    t0 = time.perf_counter()
    pairs = [(c.row, c.col, c.src_row, c.src_col) for c in copies]
    lcfg = AR.LookupConfig(AR.range_lens(W, L))
    fixed_host = CR.fixed_columns(CR.fixed_rows_of(kinds, W, L, lcfg), lcfg.table(), n, 0, P)
    t1 = time.perf_counter()
    sigma_host = PR.sigma_from_pairs(pairs, 5, n, cfg.delta, cfg.omega(P), P)
    t2 = time.perf_counter()
    fixed_up, sigma_up = columns_tensor(fixed_host), columns_tensor(sigma_host)
    torch.cuda.synchronize()
    t3 = time.perf_counter()

    # the device route: one untimed call of each, compared with the host's columns byte for byte
    fixed, st_f = prover.keygen_fixed_columns(chip, la, kinds_dev, K, BF)
    sigma, st_s, info = prover.keygen_sigma_columns(chip, pairs_dev, K, BF, delta, dom.omega)
    torch.cuda.synchronize()
    assert st_f.cpu().tolist() == [0] and st_s.cpu().tolist() == [0]
    assert torch.equal(fixed, fixed_up) and torch.equal(sigma, sigma_up), "the device's key is not the host's"
    assert delta == rep(cfg.delta)
    prover._key_commitments(lk, fixed, sigma)
    torch.cuda.synchronize()
    print("byte-compare of the two keys: equal (15 fixed and 5 sigma columns of %d rows)" % n)
    print("sigma: %d hook rounds (the last one changed nothing), %d touched cells, %d sort passes" % (info.hook_rounds, info.touched_cells, info.sort_passes))

    fixed_ms, phase_ms, sigma_wall, commit_ms = [], {name: [] for name, _ in PHASES}, [], []
    for _ in range(REPS):
        _lib.profile_enable(1 << 10)
        prover.keygen_fixed_columns(chip, la, kinds_dev, K, BF, out=(fixed, st_f))
        torch.cuda.synchronize()
        t = time.perf_counter()
        prover.keygen_sigma_columns(chip, pairs_dev, K, BF, delta, dom.omega, out=(sigma, st_s))
        torch.cuda.synchronize()
        sigma_wall.append(1e3 * (time.perf_counter() - t))
        fixed_ms.append(sum(_lib.profile_read(_lib.KERNEL_KEYGEN_FIXED)))
        for name, cls in PHASES:
            phase_ms[name].append(sum(_lib.profile_read(cls)))
        _lib.profile_enable(0)
        commit_ms.append(stream_ms(lambda: prover._key_commitments(lk, fixed, sigma))[0])
    med = statistics.median
    print("device route, medians of %d timed calls after one untimed:" % REPS)
    print("    fixed columns: %.3f ms of stream time (one launch; its two table uploads are waited for on the host before it)" % med(fixed_ms))
    print("    sigma, ms of stream time per phase: " + "; ".join("%s %.3f" % (name, med(phase_ms[name])) for name, _ in PHASES)
          + "; kernels summed %.3f; wall time of the call %.3f (min %.3f, max %.3f)" % (sum(med(v) for v in phase_ms.values()), med(sigma_wall), min(sigma_wall), max(sigma_wall)))
    print("    the two commit calls (15 + 5 columns, Lagrange key): %.3f ms of stream time (min %.3f, max %.3f)" % (med(commit_ms), min(commit_ms), max(commit_ms)))
    print("host route, wall time, once: fixed_rows_of + fixed_columns %.2f s; sigma_from_pairs %.2f s; conversion and upload of 20 columns %.2f s; together %.2f s"
          % (t1 - t0, t2 - t1, t3 - t2, t3 - t0))
