#!/usr/bin/env python3
"""Timing of the pairing check, Montgomery ctx: the stream time of one h2r_pairing_products call (prover.pairing_check) at
two pairs -- the verifier's e(L, [tau]G2) e(-R, G2) -- and batches of 1, 8 and 256 circuits, between two events on the stream and as the HIP
events stamped by the dispatch (h2r_profile_*); then prover.verify against prover.verify_proof alone on the proofs of
tools/verify_proof_timing.py, in the same process.  Medians of the timed runs after one untimed run.  The accumulators are create_proof's
over a key of [tau^i]G, so every circuit must be accepted (checked).  For scale only: the plain-Python model's time per pairing (the final
exponentiation by plain square-and-multiply).  halo2curves is not built here: there is no comparison figure.  No target is set and nothing
rests on these numbers.
    python tools/pairing_timing.py [runs] > profiles/pairing.txt"""
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from halo2_rsa_amd import _lib, prover
import msm_ref as M
import pairing_ref as P
import verify_proof_timing as VT

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
VT.REPS = REPS


def timed(fn):
    fn()                                                                           # untimed: code objects, allocator
    torch.cuda.synchronize()
    total, kernel = [], []
    for _ in range(REPS):
        _lib.profile_enable(1 << 10)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        total.append(a.elapsed_time(b))
        kernel.append(sum(_lib.profile_read(_lib.KERNEL_PAIRING)))
        _lib.profile_enable(0)
    return total, kernel


def line(name, ms):
    return "%s %8.3f ms median (min %.3f, max %.3f)" % (name, statistics.median(ms), min(ms), max(ms))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: two events on the stream around one call (stream time); pairing_kernel alone: the HIP events stamped by its dispatch, summed.")
    print("Montgomery ctx, bn254_fr; %d timed runs after one untimed.  Nothing rests on these numbers; no target is set." % REPS)
    print(torch.cuda.get_device_name(0), flush=True)
    key, image, _ = VT.recorded(8)
    proofs, status = prover.create_proof(key, image, 8, seed=bytes(range(32)))
    vk = key.verifying_key()
    pkey = prover.PairingKey(vk.chip, [P.g2_bytes(P.g2_mul(VT.TAU, P.G2), True), P.g2_bytes(P.G2, True)])
    left, right, vstatus = prover.verify_proof(vk, proofs)
    accept, gt = prover.pairing_check(pkey, torch.stack((left, right), dim=1), 0b10, vstatus)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == vstatus.cpu().tolist() == [0] * 8 and accept.cpu().tolist() == [1] * 8, "the device rejects create_proof's proofs"
    for batch in (1, 8, 256):
        pts = torch.stack((left, right), dim=1).repeat((batch + 7) // 8, 1, 1)[:batch].contiguous()
        out = (torch.empty(batch, dtype=torch.uint8, device="cuda"), torch.zeros((batch, 384), dtype=torch.uint8, device="cuda"))
        total, kernel = timed(lambda: prover.pairing_check(pkey, pts, 0b10, None, out=out))
        assert out[0].cpu().tolist() == [1] * batch
        print("batch %3d, 2 pairs: %s; %s" % (batch, line("h2r_pairing_products", total), line("pairing_kernel", kernel)), flush=True)
    for batch in (1, 8, 256):
        p = proofs.repeat((batch + 7) // 8, 1)[:batch].contiguous()
        t_vp, _ = timed(lambda: prover.verify_proof(vk, p))
        t_v, k_v = timed(lambda: prover.verify(vk, pkey, p))
        accept, st = prover.verify(vk, pkey, p)
        torch.cuda.synchronize()
        assert accept.cpu().tolist() == [1] * batch and st.cpu().tolist() == [0] * batch
        print("batch %3d: %s; %s; %s" % (batch, line("verify_proof alone", t_vp), line("verify", t_v), line("of which pairing_kernel", k_v)), flush=True)
    Lp, Rp = (M.points_from_bytes(bytes(t[0].cpu().numpy()), True)[0] for t in (left, right))
    tab = P.prepare(P.G2)
    t0 = time.perf_counter()
    f = P.miller([(Lp, tab)])
    t1 = time.perf_counter()
    P.final_exp(f)
    t2 = time.perf_counter()
    P.final_exp_chain(f)
    t3 = time.perf_counter()
    print("for scale only -- the plain-Python model, one pairing on the host: Miller loop %.0f ms, final exponentiation by square-and-multiply %.0f ms "
          "(by the device's decomposition %.0f ms)" % (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)))
