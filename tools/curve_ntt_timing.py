#!/usr/bin/env python3
"""Timing of the Lagrange-key transform (h2r_curve_ntt): k = 15, 16, 17 and 20, canonical and Montgomery ctx, inverse
and forward, per stage and for the whole call.  The bases are n generic points of bn256 G1 (the forward transform of 4,096 points spread among identities, made on
the device, untimed).  Times are the events the dispatch itself stamps (h2r_profile_*), per launch, medians over the timed calls after one
untimed call.  Reported next to them: the point operations of the call (doublings and complete additions; COUNTED from the twiddles, no
clock read) and their rate, to be read next to profiles/msm.txt's bucket additions per second on the same box.
The choice of scalar multiplication by number: at k = 17 the same call through a build whose every butterfly runs plain per-lane bit-by-bit
double-and-add (the developer-knob variant lib/variants/curve_ntt_per_lane.so with H2R_CURVE_NTT_FORM=1, loaded into this process next to
the product library; built when missing), with the two outputs compared byte for byte.
No threshold: there is no earlier implementation, and upstream's g_to_lagrange is not here to compare with.
    python tools/curve_ntt_timing.py [repetitions] > profiles/curve_ntt.txt"""
import ctypes
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import halo2_rsa_amd as H
from halo2_rsa_amd import _build, _lib
import curve_ntt_ref as C
import msm_ref as M

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SIZES, BLOCK = (15, 16, 17, 20), 4096
R, R256 = M.R_ORDER, 1 << 256
CLASSES = (_lib.KERNEL_CURVE_NTT_TWIDDLE, _lib.KERNEL_CURVE_NTT_LOAD, _lib.KERNEL_CURVE_NTT_STAGE, _lib.KERNEL_CURVE_NTT_STORE)
UNIFORM_MIN_GROUPS = 64                       # h2r_curve_ntt.hpp: butterflies per twiddle from which a stage is twiddle-major
WINDOW_OPS = 2 + 256 + 128                    # the lane's table, 128 windows of two doublings and one addition


def naf_weight(k):
    return bin(((3 * k) ^ k) >> 1).count("1")


def dense_key(chip, block, k, montgomery):
    """n generic points: the forward transform (untimed) of the block's points spread n / BLOCK apart among (0, 0).  A block merely repeated
    would transform to identities almost everywhere, which the conversion to affine skips."""
    n = 1 << k
    raw = torch.frombuffer(bytearray(M.point_bytes(block, montgomery)), dtype=torch.uint8).reshape(BLOCK, 64).cuda()
    sparse = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    sparse[::n // BLOCK] = raw
    key = H.CommitKey(chip, sparse).transform(C.omega_of(k) * (R256 if montgomery else 1) % R, inverse=False)
    torch.cuda.synchronize()
    assert bool(key.bases.view(n, 64).any(dim=1).all())
    return key


OPS = {}


def counted_ops(k, inverse):
    """(per stage, store): doublings + complete additions, from the twiddles themselves."""
    if (k, inverse) not in OPS:
        OPS[(k, inverse)] = _counted_ops(k, inverse)
    return OPS[(k, inverse)]


def _counted_ops(k, inverse):
    n, w = 1 << k, pow(C.omega_of(k), -1, R) if inverse else C.omega_of(k)
    tw, x = [], 1
    for _ in range(n // 2):
        tw.append(x)
        x = x * w % R
    stages = []
    for s in range(1, k + 1):
        groups, ops = n >> s, 0
        for j in range(1 << (s - 1)):
            if j == 0:
                ops += 2
            elif groups >= UNIFORM_MIN_GROUPS:
                ops += 256 + naf_weight(tw[j * groups]) + 2
            else:
                ops += WINDOW_OPS + 2
        stages.append(ops * groups)
    return stages, n * (256 + naf_weight(pow(n, -1, R))) if inverse else 0


def timed(call, log_n, read=_lib.profile_read, enable=_lib.profile_enable):
    call()
    torch.cuda.synchronize()
    enable(REPS * (log_n + 8))
    for _ in range(REPS):
        call()
        torch.cuda.synchronize()
    out = {c: [float(x) for x in read(c)] for c in CLASSES}
    enable(0)
    assert len(out[_lib.KERNEL_CURVE_NTT_STAGE]) == REPS * log_n and all(len(out[c]) == REPS for c in CLASSES if c != _lib.KERNEL_CURVE_NTT_STAGE)
    return out


def summary(ms, log_n):
    stage = ms[_lib.KERNEL_CURVE_NTT_STAGE]
    per_stage = [statistics.median(stage[r * log_n + s] for r in range(REPS)) for s in range(log_n)]
    edges = {c: statistics.median(ms[c]) for c in CLASSES if c != _lib.KERNEL_CURVE_NTT_STAGE}
    calls = [sum(stage[r * log_n:(r + 1) * log_n]) + sum(ms[c][r] for c in edges) for r in range(REPS)]
    return per_stage, edges, statistics.median(calls), min(calls), max(calls)


def run(montgomery, block):
    chip = H.BigIntChip(64, 256, montgomery=montgomery)
    name = "Montgomery" if montgomery else "canonical"
    for k in SIZES:
        n = 1 << k
        key = dense_key(chip, block, k, montgomery)
        out = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        cfg = _lib.H2RCurveNttConfig()
        cfg.struct_size, cfg.log_n = ctypes.sizeof(cfg), k
        ws = torch.empty(int(_lib.lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(cfg))), dtype=torch.uint8, device="cuda")
        omega = C.omega_of(k) * (R256 if montgomery else 1) % R
        for inverse in (True, False):
            ms = timed(lambda: key.transform(omega, inverse=inverse, out=out, workspace=ws), k)
            per_stage, edges, med, lo, hi = summary(ms, k)
            ops_stage, ops_store = counted_ops(k, inverse)
            ops = sum(ops_stage) + ops_store
            print("%s ctx, k = %d, %s: call %9.3f ms (min %9.3f, max %9.3f; %d timed calls); twiddles %.3f, load %.3f, store %.3f ms; %.4g point operations, %.3g per second"
                  % (name, k, "inverse" if inverse else "forward", med, lo, hi, REPS, edges[CLASSES[0]], edges[CLASSES[1]], edges[CLASSES[3]], ops, ops / (med * 1e-3)))
            print("    stage ms: " + " ".join("%.3f" % t for t in per_stage))
            print("    stage point operations per second: " + " ".join("%.3g" % (o / (t * 1e-3)) for o, t in zip(ops_stage, per_stage)))
        del key, out, ws
        torch.cuda.empty_cache()
    print(flush=True)


def baseline(block):
    """k = 17, inverse: the shipped forms against per-lane bit-by-bit double-and-add in every butterfly, in this process."""
    k = 17
    n = 1 << k
    path = os.environ.get("H2R_CURVE_NTT_BASELINE_LIB") or os.path.join(_build.PKG, "lib", "variants", "curve_ntt_per_lane.so")
    if not os.path.exists(path) or _build.lib_id(path) != _build.source_id(["H2R_DEV_KNOBS"]):
        _build.build_lib(out=path, defines=["H2R_DEV_KNOBS"])
    os.environ["H2R_CURVE_NTT_FORM"] = "1"                        # read once by the variant; the product library never reads the environment
    V = ctypes.CDLL(path)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    V.h2r_ctx_create_ex.argtypes = [ctypes.POINTER(_lib.H2RParams), ctypes.POINTER(_lib.H2RAdviceRepr), ctypes.POINTER(vp)]
    V.h2r_ctx_destroy.argtypes, V.h2r_ctx_destroy.restype = [vp], None
    V.h2r_curve_ntt.argtypes = [vp, ctypes.POINTER(_lib.H2RCurveNttConfig), vp, vp, vp, vp]
    V.h2r_profile_enable.argtypes = [u32]
    V.h2r_profile_read.argtypes = [u32, ctypes.POINTER(ctypes.c_float), u32, ctypes.POINTER(u32)]

    def v_read(kernel):
        cnt = u32(0)
        assert V.h2r_profile_read(kernel, None, 0, ctypes.byref(cnt)) == 0
        buf = (ctypes.c_float * max(cnt.value, 1))()
        assert V.h2r_profile_read(kernel, buf, cnt.value, ctypes.byref(cnt)) == 0
        return [float(buf[i]) for i in range(cnt.value)]

    def v_enable(cap):
        assert V.h2r_profile_enable(cap) == 0

    print("The choice of scalar multiplication, k = 17, inverse, whole call (the same process, the same buffers):")
    for montgomery in (False, True):
        chip = H.BigIntChip(64, 256, montgomery=montgomery)
        key = dense_key(chip, block, k, montgomery)
        out, out_v = (torch.zeros((n, 64), dtype=torch.uint8, device="cuda") for _ in range(2))
        cfg = _lib.H2RCurveNttConfig()
        cfg.struct_size, cfg.log_n, cfg.flags = ctypes.sizeof(cfg), k, _lib.H2R_CURVE_NTT_INVERSE
        omega = C.omega_of(k) * (R256 if montgomery else 1) % R
        for i in range(4):
            cfg.omega[i] = (omega >> (64 * i)) & (2 ** 64 - 1)
        ws = torch.empty(int(_lib.lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(cfg))), dtype=torch.uint8, device="cuda")
        ctx, params, rep = vp(), _lib.H2RParams(64, 256, 0, chip.device), _lib.H2RAdviceRepr()
        rep.struct_size, rep.flags = ctypes.sizeof(rep), _lib.H2R_ADVICE_MONTGOMERY if montgomery else 0
        assert V.h2r_ctx_create_ex(ctypes.byref(params), ctypes.byref(rep), ctypes.byref(ctx)) == 0

        def v_call():
            assert V.h2r_curve_ntt(ctx, ctypes.byref(cfg), key.bases.data_ptr(), out_v.data_ptr(), ws.data_ptr(), None) == 0

        shipped = summary(timed(lambda: key.transform(omega, out=out, workspace=ws), k), k)
        plain = summary(timed(v_call, k, v_read, v_enable), k)
        torch.cuda.synchronize()
        assert torch.equal(out, out_v), "the two builds disagree"
        V.h2r_ctx_destroy(ctx)
        print("  %-10s ctx: shipped (non-adjacent form where a wave shares its twiddle, 2-bit windows elsewhere) %9.3f ms; per-lane double-and-add %9.3f ms; ratio %.3f; outputs equal"
              % ("Montgomery" if montgomery else "canonical", shipped[2], plain[2], plain[2] / shipped[2]))
        print("    shipped stage ms:  " + " ".join("%.3f" % t for t in shipped[0]))
        print("    per-lane stage ms: " + " ".join("%.3f" % t for t in plain[0]))
    print(flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("MEASURED: every time below (HIP events stamped by the dispatch itself, medians over the timed calls; a call's time = the sum of its launches).")
    print("COUNTED: point operations = doublings + complete additions of the butterflies and of the n^-1 pass, from the twiddles' digits.  No clock is read.")
    print(torch.cuda.get_device_name(0))
    block = M.structured_bases(BLOCK, 0x1234567890abcdef, 0xfedcba987654321)
    for m in (False, True):
        run(m, block)
    baseline(block)
