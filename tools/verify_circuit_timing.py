#!/usr/bin/env python3
"""Timing of keygen, create_proof and verify on the closed verify_pkcs1v15_signature circuit at the reference's sizes:
RSA-1024, e = 65537 at k = 15 (benches/bench.rs:369-377, 28,748 rows) and RSA-2048, e = 65537 at k = 17 (src/chip.rs:674, 77,356 rows),
one circuit each, Montgomery ctx, bn254_fr -- next to the same three calls on the parent's OPEN circuit: the element image alone under
h2r_pow_copy_map's pairs (what a key was made of before the closed map existed).
Per call: wall time (host clock around the call and a synchronisation) and stream time (two events on the stream), medians over the
timed calls after one untimed call.  The closed circuit's proof must be accepted and the open one's too before any number is printed.
No target is set and nothing rests on these numbers.
    python tools/verify_circuit_timing.py [calls] > profiles/verify_circuit.txt"""
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import prover
import msm_ref as M
import prover_chain_ref as CR

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
P, R256, BF, E = M.R_ORDER, 1 << 256, 5, 65537
DIGEST_INFO = bytes.fromhex("3031300d060960864801650304020105000420")


def rep(v):
    return v * R256 % P


def is_prime(n, rng):
    if n % 2 == 0 or any(n % q == 0 for q in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)):
        return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(24):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def signed_1024():
    """(n, signature, digest as an integer) of a fresh RSA-1024 key, e = 65537; EM = 00 01 ff.. 00 DigestInfo digest"""
    rng = random.Random("verify-circuit/timing")
    ps = []
    while len(ps) < 2:
        c = rng.getrandbits(512) | (3 << 510) | 1
        if (c - 1) % E and is_prime(c, rng):
            ps.append(c)
    n, d = ps[0] * ps[1], pow(E, -1, (ps[0] - 1) * (ps[1] - 1))
    digest = hashlib.sha256(b"verify circuit timing").digest()
    em = b"\x00\x01" + b"\xff" * (128 - 3 - len(DIGEST_INFO) - 32) + b"\x00" + DIGEST_INFO + digest
    return n, pow(int.from_bytes(em, "big"), d, n), int.from_bytes(digest, "big")


def signed_2048():
    with open(os.path.join(ROOT, "tests", "golden", "halo2_rsa_golden.json")) as f:
        kat = json.load(f)["rsa_kats"][0]
    return int(kat["n"]), int(kat["sig"]), int(kat["hashed"])


def timed(fn):
    """(wall ms, stream ms, result) of one call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t), a.elapsed_time(b), out


def medians(fn):
    fn()
    torch.cuda.synchronize()
    runs = [timed(fn) for _ in range(REPS)]
    return statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs), runs[-1][2]


def circuit(bits, k, n, sig, hashed):
    nl = bits // 64
    rsa = H.RSAChip(bits, 5, montgomery=True)
    chip = rsa.bigint_chip()
    pk = rsa.assign_public_key(H.RSAPublicKey(H.UnassignedInteger.from_ints([n], nl, 64), H.Fix(E)))
    sg = rsa.assign_signature(H.RSASignature(H.UnassignedInteger.from_ints([sig], nl, 64)))
    res = rsa.verify_pkcs1v15_signature(pk, [hashed], sg)
    assert res.status.cpu().tolist() == [0] and res.is_valid.cpu().tolist() == [1]
    vl = res.layout
    rows, sec = chip.verify_circuit_rows(vl)
    _, sec4 = res.advice_sections()
    cfg = CR.config(P, k, BF)
    dom = H.EvaluationDomain(chip, k, k + 3, rep(cfg.omega_ext), rep(cfg.zeta))
    params = prover.setup(chip, k, seed=bytes(range(32)), omega=dom.omega)
    la = H.LookupArgument(chip, rsa_chip=True)
    shapes = (("closed circuit", chip.verify_circuit_row_kinds(vl), chip.verify_circuit_copy_map(vl, E), res.emit_verify_circuit(direct=True)),
              ("open element (parent: pow-only map)", res.row_kinds(), chip.pow_copy_map(vl.pow, E, row_offset=sec4[0] + sec4[1]), res.emit_advice(direct=True)))
    print("RSA-%d, e = %d, k = %d: closed circuit %d rows (%d + %d + 1), one circuit, Montgomery ctx, bn254_fr" % (bits, E, k, rows, sec[0], sec[1]), flush=True)
    for name, kinds, pairs, image in shapes:
        pairs_dev = prover.copy_pairs_tensor(pairs, "cuda:0")
        outside = sum(1 for c in pairs if c.src_row >= 0xFFFFFF00)
        kg = medians(lambda: prover.keygen(chip, dom, params.g, la, kinds, pairs_dev, BF, lagrange_key=params.g_lagrange))
        key = kg[2]
        vk, pkey = key.verifying_key(), params.pairing_key()
        cp = medians(lambda: prover.create_proof(key, image, 1, seed=bytes(32)))
        proof, status = cp[2]
        vf = medians(lambda: prover.verify(vk, pkey, proof))
        accept, vstatus = vf[2]
        assert status.cpu().tolist() == [0] and accept.cpu().tolist() == [1] and vstatus.cpu().tolist() == [0], name
        print("    %s: %d rows, %d copy pairs (%d with a source outside the image, dropped by keygen), proof accepted" % (name, len(kinds), len(pairs), outside))
        print("        keygen       wall %8.2f ms   stream %8.2f ms" % kg[:2])
        print("        create_proof wall %8.2f ms   stream %8.2f ms" % cp[:2])
        print("        verify       wall %8.2f ms   stream %8.2f ms" % vf[:2], flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: host wall clock around each call and a synchronisation; two events on the stream around the same call; medians of %d timed calls after one untimed." % REPS)
    print(torch.cuda.get_device_name(0), flush=True)
    circuit(1024, 15, *signed_1024())
    circuit(2048, 17, *signed_2048())
