#!/usr/bin/env python3
"""Timing of the Fiat-Shamir transcript on the device (h2r_transcript_round) for the shape of a recorded k = 17
circuit: 35 commitments and 46 evaluations over six rounds (theta; beta, gamma; y; x with the three rotations and x^n; v; the W points),
at batches of 1, 8 and 256 circuits, canonical and Montgomery ctx.
Per round: the events the dispatch itself stamps (h2r_profile_*), medians over the timed proofs after one untimed proof.  Per proof: the
stream time of the six rounds between two events on the stream.  Against it, in the same process, what a caller does without the device
transcript at every one of the six boundaries: synchronise, copy the round's items to the host, hash them with hashlib, reduce, and upload
the challenges through _marshal.challenges (canonical ctx: the bytes on the device are the bytes hashed); a host clock around work that ends
in the upload's synchronise.  The two are compared challenge for challenge.
No threshold: there is no earlier device implementation.
    python tools/transcript_timing.py [proofs] > profiles/transcript.txt"""
import hashlib
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _lib, _marshal

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
BATCHES = (1, 8, 256)
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
R256 = 1 << 256
K = 17
OMEGA = pow(7, (R - 1) >> K, R)
# (name, common scalars shared by the batch, points, scalars, squeezes, derived values as (src, multiplier, log2_pow))
ROUNDS = (("theta", 1, 5, 0, 1, ()), ("beta, gamma", 0, 10, 0, 2, ()), ("y", 0, 9, 0, 1, ()),
          ("x", 0, 7, 0, 1, ((0, OMEGA, 0), (0, pow(OMEGA, -1, R), 0), (0, pow(OMEGA, -6, R), 0), (0, 1, K))),
          ("v", 0, 0, 46, 1, ()), ("W", 0, 4, 0, 0, ()))
PROOF_BYTES = 32 * sum(p + s for _, _, p, s, _, _ in ROUNDS)


def make_items(batch, montgomery, rng):
    """Per round: (shared common scalars or None, points [batch, P, 2, 4] or None, scalars [batch, S, 4] or None), random canonical values."""
    def tensor(vals, modulus, shape):
        raw = b"".join(((v * R256 % modulus) if montgomery else v).to_bytes(32, "little") for v in vals)
        return torch.frombuffer(bytearray(raw), dtype=torch.int64).reshape(shape).cuda()
    out = []
    for _, c, p, s, _, _ in ROUNDS:
        out.append((tensor([rng.randrange(R) for _ in range(c)], R, (c, 4)) if c else None,
                    tensor([rng.randrange(Q) for _ in range(batch * p * 2)], Q, (batch, p, 2, 4)) if p else None,
                    tensor([rng.randrange(R) for _ in range(batch * s)], R, (batch, s, 4)) if s else None))
    return out


def device_proof(chip, batch, items, montgomery):
    """One proof's six rounds, enqueued back to back; (challenges per round, the transcript)."""
    tr = H.Transcript(chip, batch, PROOF_BYTES)
    rep = (lambda v: v * R256 % R) if montgomery else (lambda v: v)
    out = []
    for (_, _, _, _, squeeze, derive), (common, points, scalars) in zip(ROUNDS, items):
        if common is not None:
            tr.common_scalars(common)
        written = [(t, k) for t, k in ((points, tr.POINT), (scalars, tr.SCALAR)) if t is not None]
        out.append(tr.round(written, squeeze, [(s, rep(m), l) for s, m, l in derive])[0])
    return out, tr


def host_proof(batch, items, dev):
    """The same six boundaries through the host (canonical ctx): synchronise, download, hashlib, reduce, upload."""
    hs = [hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript") for _ in range(batch)]
    out = []
    for (_, _, _, _, squeeze, _), (common, points, scalars) in zip(ROUNDS, items):
        torch.cuda.synchronize()
        if common is not None:
            raw = common.cpu().numpy().tobytes()
            for h in hs:
                for i in range(0, len(raw), 32):
                    h.update(b"\x02" + raw[i:i + 32])
        for t, prefix, size in ((points, b"\x01", 64), (scalars, b"\x02", 32)):
            if t is None:
                continue
            host = t.cpu().numpy()
            for e, h in enumerate(hs):
                raw = host[e].tobytes()
                for i in range(0, len(raw), size):
                    h.update(prefix + raw[i:i + size])
        if squeeze:
            ch = []
            for h in hs:
                row = []
                for _ in range(squeeze):
                    h.update(b"\x00")
                    row.append(int.from_bytes(h.copy().digest(), "little") % R)
                ch.append(row)
            out.append(_marshal.challenges(ch, dev))
        else:
            out.append(None)
    torch.cuda.synchronize()
    return out


def run(montgomery):
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    name = "Montgomery" if montgomery else "canonical"
    dev = "cuda:%d" % chip.device
    for batch in BATCHES:
        items = make_items(batch, montgomery, random.Random("transcript/timing/%d" % batch))
        got, _ = device_proof(chip, batch, items, montgomery)                     # untimed: code objects, allocations
        torch.cuda.synchronize()
        launches = len(ROUNDS) + sum(1 for r in ROUNDS if r[1])
        _lib.profile_enable(REPS * launches)
        stream_ms = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            device_proof(chip, batch, items, montgomery)
            b.record()
            torch.cuda.synchronize()
            stream_ms.append(a.elapsed_time(b))
        per_launch = _lib.profile_read(_lib.KERNEL_TRANSCRIPT)
        _lib.profile_enable(0)
        assert len(per_launch) == REPS * launches
        rounds = [statistics.median(per_launch[r * launches + 1 + i] + (per_launch[r * launches] if i == 0 else 0.0) for r in range(REPS))
                  for i in range(len(ROUNDS))]
        print("%s ctx, batch %3d: proof (six rounds, %d launches, stream time) %8.3f ms median (min %.3f, max %.3f; %d timed proofs); kernels' own events summed %.3f ms"
              % (name, batch, launches, statistics.median(stream_ms), min(stream_ms), max(stream_ms), REPS, sum(rounds)))
        print("    per round, ms: " + "; ".join("%s %.4f" % (r[0], t) for r, t in zip(ROUNDS, rounds)))
        if not montgomery:
            ref = host_proof(batch, items, dev)                                  # untimed, and the cross-check
            for g, w in zip(got, ref):
                assert w is None or torch.equal(g, w), "the device and hashlib disagree"
            host_ms = []
            for _ in range(max(3, REPS // 4)):
                t0 = time.perf_counter()
                host_proof(batch, items, dev)
                host_ms.append((time.perf_counter() - t0) * 1e3)
            print("    through the host (synchronise, download, hashlib, upload at each boundary): %8.3f ms median (min %.3f, max %.3f; %d timed); challenges equal"
                  % (statistics.median(host_ms), min(host_ms), max(host_ms), len(host_ms)))
    print(flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: per round the HIP events stamped by the dispatch itself; per proof two events on the stream around the six rounds; the host path a host clock")
    print("around work that ends in a synchronise.  Medians over the timed proofs after one untimed proof.  Shape: k = 17, %d points and %d evaluations, %d proof bytes."
          % (sum(r[2] for r in ROUNDS), sum(r[3] for r in ROUNDS), PROOF_BYTES))
    print("The first round is two launches (the common scalar, then the written points); its time is their sum.")
    print(torch.cuda.get_device_name(0))
    for m in (False, True):
        run(m)
