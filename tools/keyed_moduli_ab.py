"""Keyed moduli: same-box A/B of the parent commit's library against this tree's (profiles/keyed_moduli_ab.txt).

  python tools/keyed_moduli_ab.py --build-parent [REV]   # the parent's sources (git archive REV, default HEAD) built into
                                                        # halo2_rsa_amd/lib/variants/parent.so; no GPU needed
  python tools/keyed_moduli_ab.py --run [--reps 10]     # on the GPU: parent / branch alternately, every run a fresh child process
                                                        # under its own `timeout`; the table goes to stdout and to --out
  python tools/keyed_moduli_ab.py --resources [PARENT_TREE]   # VGPRs / scratch / occupancy of every chain and step build (hipcc
                                                        # -Rpass-analysis=kernel-resource-usage; no GPU needed)

Workloads (e = 65537, modpow_public_key with records and the in-field witness): RSA-1024 x 1,024 and x 2,048 per call and RSA-2048 x
1,024 per call pipelined (depth 3, two side streams, trace regions from the placement-aware arena), RSA-2048 x 256 as one plain call.
Each with per-element moduli (both libraries) and, on the branch, keyed with 1, 16 and `batch` keys.  The worker talks to the library
through ctypes alone, so that the parent's library -- which lacks the new exports -- loads.  Criteria (the issue's):
  (a) branch per-element  <= parent per-element median + parent spread (max - min of its runs)
  (b) branch keyed (any number of keys) <= parent per-element median + parent spread
  (c) RSA-1024 x 1,024 pipelined and RSA-2048 x 256 plain, 1 and 16 keys: branch keyed < parent per-element median - parent spread
"""
import argparse
import ctypes
import json
import os
import random
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARENT_LIB = os.path.join(ROOT, "halo2_rsa_amd", "lib", "variants", "parent.so")
BRANCH_LIB = os.path.join(ROOT, "halo2_rsa_amd", "lib", "libh2r.so")
WORKLOADS = [("rsa1024 x 1024 pipelined", 1024, 1024, True), ("rsa1024 x 2048 pipelined", 1024, 2048, True),
             ("rsa2048 x 1024 pipelined", 2048, 1024, True), ("rsa2048 x 256 plain", 2048, 256, False)]
GAIN = ("rsa1024 x 1024 pipelined", "rsa2048 x 256 plain")
E_LE = (65537).to_bytes(3, "little")
OP_IS_IN_FIELD = 10


# ---- the worker: one library, every workload --------------------------------------------------------------------------------------
def _limbs(values, L):
    import numpy as np
    out = np.zeros((len(values), L), dtype=np.uint64)
    for r, v in enumerate(values):
        for i in range(L):
            out[r, i] = (v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF
    return out.view(np.int64)


def worker(lib_path, steps, warmup, clock_calls):
    import numpy as np
    import torch
    from halo2_rsa_amd._lib import H2RKeyedModuli, H2RParams, H2RPowLayout
    L_ = ctypes.CDLL(lib_path)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L_.h2r_workspace_bytes.restype = u64
    L_.h2r_workspace_bytes.argtypes = [vp, u64, u32]
    L_.h2r_arena_region.restype = vp
    L_.h2r_arena_region.argtypes = [vp, u32]
    L_.h2r_arena_create.argtypes = [vp, u64, u64, u32, u64, u32, u32, vp, ctypes.POINTER(vp)]
    L_.h2r_arena_destroy.argtypes = [vp]
    L_.h2r_arena_destroy.restype = None
    L_.h2r_pipeline_create_ex.argtypes = [vp, u32, u32, ctypes.POINTER(vp)]
    L_.h2r_pipeline_destroy.argtypes = [vp]
    L_.h2r_pipeline_destroy.restype = None
    L_.h2r_pipeline_join.argtypes = [vp, vp]
    sig = [vp, vp, vp, ctypes.c_char_p, ctypes.c_size_t, u64, u32, vp, vp, vp, vp, vp, vp]
    L_.h2r_pipeline_modpow_public_key.argtypes = sig
    L_.h2r_modpow_public_key_batch.argtypes = sig
    L_.h2r_fresh_op_layout.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32)]
    L_.h2r_ctx_create.argtypes = [ctypes.POINTER(H2RParams), ctypes.POINTER(vp)]
    L_.h2r_ctx_destroy.argtypes = [vp]
    L_.h2r_ctx_destroy.restype = None
    L_.h2r_pow_fixed_layout.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(H2RPowLayout)]
    keyed_lib = hasattr(L_, "h2r_key_table_build")
    if keyed_lib:
        L_.h2r_key_table_bytes.restype = u64
        L_.h2r_key_table_bytes.argtypes = [vp, u64]
        L_.h2r_key_table_build.argtypes = [vp, vp, u64, vp, vp, vp]

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError("%s: h2r status %d" % (what, rc))
    dev = "cuda:0"
    result = {"lib": os.path.basename(lib_path), "keyed_lib": keyed_lib, "ms": {}, "table_build_us": {}}
    for name, bits, B, piped in WORKLOADS:
        L = bits // 64
        ctx = vp()
        p = H2RParams(64, bits, 0, 0)
        ok(L_.h2r_ctx_create(ctypes.byref(p), ctypes.byref(ctx)), "h2r_ctx_create")
        pl = H2RPowLayout()
        ok(L_.h2r_pow_fixed_layout(ctx, E_LE, len(E_LE), ctypes.byref(pl)), "h2r_pow_fixed_layout")
        ies = u64()
        ok(L_.h2r_fresh_op_layout(ctx, OP_IS_IN_FIELD, ctypes.byref(ies), None, None), "h2r_fresh_op_layout")
        rng = random.Random(bits * 7 + B)
        keys = [rng.getrandbits(bits) | (1 << (bits - 1)) | 1 for _ in range(B)]
        n_sets = 3 if piped else 1
        arena = vp()
        if piped:
            ok(L_.h2r_arena_create(ctx, pl.elem_stride, pl.off_records, pl.num_mul_mods, B, n_sets, 8, None, ctypes.byref(arena)), "h2r_arena_create")
            traces = [L_.h2r_arena_region(arena, i) for i in range(n_sets)]
            keep = None
        else:
            keep = [torch.empty(B * pl.elem_stride, dtype=torch.uint8, device=dev) for _ in range(n_sets)]
            traces = [t.data_ptr() for t in keep]
        ws_bytes = int(L_.h2r_workspace_bytes(ctx, B, pl.num_mul_mods))
        sets = [dict(trace=traces[i], ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev), inf=torch.zeros(B * ies.value, dtype=torch.uint8, device=dev),
                     out=torch.empty((B, L), dtype=torch.int64, device=dev), status=torch.zeros(B, dtype=torch.uint8, device=dev)) for i in range(n_sets)]
        pipe = vp()
        if piped:
            ok(L_.h2r_pipeline_create_ex(ctx, 3, 2, ctypes.byref(pipe)), "h2r_pipeline_create_ex")
        variants = [("per-element", None)] + ([("keyed %d" % nk if nk != B else "keyed batch", nk) for nk in (1, 16, B)] if keyed_lib else [])
        for vname, nk in variants:
            if nk is None:
                idx = list(range(B))
            else:
                idx = [i % nk for i in range(B)]
            xs = [rng.randrange(keys[k]) for k in idx]
            x_dev = torch.from_numpy(_limbs(xs, L)).to(dev)
            hold = []
            if nk is None:
                n_dev = torch.from_numpy(_limbs([keys[k] for k in idx], L)).to(dev)
                n_arg, flags = n_dev.data_ptr(), 0
            else:
                kd = torch.from_numpy(_limbs(keys[:nk], L)).to(dev)
                tab = torch.empty(int(L_.h2r_key_table_bytes(ctx, nk)), dtype=torch.uint8, device=dev)
                ok(L_.h2r_key_table_build(ctx, kd.data_ptr(), nk, tab.data_ptr(), None, None), "h2r_key_table_build")
                idx_dev = torch.tensor(idx, dtype=torch.int32, device=dev)
                km = H2RKeyedModuli(ctypes.sizeof(H2RKeyedModuli), 0, nk, tab.data_ptr(), idx_dev.data_ptr())
                hold = [kd, tab, idx_dev, km]
                n_arg, flags = ctypes.addressof(km), 2
            torch.cuda.synchronize()

            def call(k):
                s = sets[k % n_sets]
                args = (x_dev.data_ptr(), n_arg, E_LE, len(E_LE), B, flags, s["trace"], s["inf"].data_ptr(), s["out"].data_ptr(), s["status"].data_ptr(),
                        s["ws"].data_ptr(), None)
                if piped:
                    ok(L_.h2r_pipeline_modpow_public_key(pipe, *args), "h2r_pipeline_modpow_public_key")
                else:
                    ok(L_.h2r_modpow_public_key_batch(ctx, *args), "h2r_modpow_public_key_batch")
            if piped:
                for k in range(clock_calls + warmup):      # (the clocks ramp over the first few dozen calls of a cold process)
                    call(k)
                ok(L_.h2r_pipeline_join(pipe, None), "h2r_pipeline_join")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(steps):
                    call(k)
                ok(L_.h2r_pipeline_join(pipe, None), "h2r_pipeline_join")
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3 / steps
            else:
                for k in range(clock_calls // 4 + warmup):
                    call(k)
                torch.cuda.synchronize()
                ts = []
                for k in range(steps):
                    t0 = time.perf_counter()
                    call(k)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                ms = statistics.median(ts)
            bad = int((sets[0]["status"] != 0).sum())
            if bad:
                raise RuntimeError("%s / %s: %d elements with a status" % (name, vname, bad))
            result["ms"]["%s | %s" % (name, vname)] = round(ms, 5)
            del hold
        if keyed_lib and bits == 2048 and B == 1024:   # the table's own cost: 1, 16, 1,024 RSA-2048 keys
            kd = torch.from_numpy(_limbs(keys[:1024], L)).to(dev)
            for nk in (1, 16, 1024):
                tab = torch.empty(int(L_.h2r_key_table_bytes(ctx, nk)), dtype=torch.uint8, device=dev)
                ts = []
                for _ in range(12):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    ok(L_.h2r_key_table_build(ctx, kd.data_ptr(), nk, tab.data_ptr(), None, None), "h2r_key_table_build")
                    b.record()
                    torch.cuda.synchronize()
                    ts.append(a.elapsed_time(b) * 1e3)
                result["table_build_us"][str(nk)] = round(statistics.median(ts[2:]), 2)
        if piped:
            L_.h2r_pipeline_destroy(pipe)
            torch.cuda.synchronize()
            L_.h2r_arena_destroy(arena)
        L_.h2r_ctx_destroy(ctx)
    print("AB_RESULT " + json.dumps(result), flush=True)


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def run(reps, steps, warmup, clock_calls, out_path, step_timeout):
    for lib in (PARENT_LIB, BRANCH_LIB):
        if not os.path.exists(lib):
            sys.exit("missing %s (see --build-parent / build the tree first)" % lib)
    runs = {"parent": [], "branch": []}
    for rep in range(reps):
        for who, lib in (("parent", PARENT_LIB), ("branch", BRANCH_LIB)):
            cmd = ["timeout", "-k", "10", str(step_timeout), sys.executable, os.path.abspath(__file__), "--worker", lib, "--steps", str(steps),
                   "--warmup", str(warmup), "--clock-calls", str(clock_calls)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            m = re.search(r"^AB_RESULT (.*)$", r.stdout, re.M)
            if r.returncode != 0 or not m:   # a GPU step that failed: nothing more is started
                sys.exit("rep %d %s: exit status %d\n%s\n%s" % (rep, who, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            runs[who].append(json.loads(m.group(1)))
            print("rep %d %s done" % (rep + 1, who), flush=True)
    lines = report(runs, reps, steps, warmup, clock_calls)
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def report(runs, reps, steps, warmup, clock_calls):
    med = statistics.median
    out = ["Keyed moduli: same-box A/B against the parent commit (tools/keyed_moduli_ab.py --run)",
           "parent / branch alternately, %d runs each, every run a fresh child process; per run: %d untimed clock warm-up calls, %d warm-up calls," % (reps, clock_calls, warmup),
           "%d timed calls (pipelined: wall time of the train incl. the join / calls; plain: median of the single calls' wall times).  ms per call." % steps, ""]
    verdicts = []
    for name, bits, B, piped in WORKLOADS:
        pk = "%s | per-element" % name
        pv = [r["ms"][pk] for r in runs["parent"]]
        pm, spread = med(pv), max(pv) - min(pv)
        out.append("%s   (%.2f M assigns/s at the parent's median)" % (name, B / pm / 1e3))
        out.append("  parent per-element   median %.4f   min %.4f  max %.4f  spread %.4f   runs %s" % (pm, min(pv), max(pv), spread, " ".join("%.4f" % v for v in pv)))
        for vname in ["per-element", "keyed 1", "keyed 16", "keyed batch"]:
            bv = [r["ms"]["%s | %s" % (name, vname)] for r in runs["branch"]]
            bm = med(bv)
            tags = []
            crit = "(a)" if vname == "per-element" else "(b)"
            okk = bm <= pm + spread
            tags.append("%s %s" % (crit, "PASS" if okk else "FAIL"))
            verdicts.append(okk)
            if name in GAIN and vname in ("keyed 1", "keyed 16"):
                g = bm < pm - spread
                tags.append("(c) %s" % ("PASS" if g else "FAIL"))
                verdicts.append(g)
            out.append("  branch %-13s median %.4f   min %.4f  max %.4f  (branch - parent = %+.4f ms, %+.1f %%)   %s   runs %s" % (
                vname, bm, min(bv), max(bv), bm - pm, 100 * (bm - pm) / pm, "  ".join(tags), " ".join("%.4f" % v for v in bv)))
        out.append("")
    tb = [r["table_build_us"] for r in runs["branch"] if r["table_build_us"]]
    if tb:
        out.append("h2r_key_table_build, RSA-2048 keys (event time around the launch, median of 10 per run; median / max over the runs), us:")
        for nk in ("1", "16", "1024"):
            v = [t[nk] for t in tb]
            out.append("  %5s keys   %.1f / %.1f" % (nk, med(v), max(v)))
        out.append("")
    out.append("ALL CRITERIA MET" if all(verdicts) else "CRITERIA NOT MET: see the FAIL lines above")
    return out


# ---- builds that need no GPU ----------------------------------------------------------------------------------------------------
def build_parent(rev):
    import tempfile
    tmp = tempfile.mkdtemp(prefix="h2r_parent_")
    ar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, "halo2_rsa_amd", "include"], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", tmp], stdin=ar.stdout)
    if ar.wait() != 0:
        sys.exit("git archive %s failed" % rev)
    os.makedirs(os.path.dirname(PARENT_LIB), exist_ok=True)
    subprocess.check_call([sys.executable, "-c", "from halo2_rsa_amd import _build; print(_build.build_lib(out=%r)); print(_build.build_lib.last)" % PARENT_LIB], cwd=tmp)
    print(tmp)


def resources(parent_tree):
    import tempfile
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "--offload-device-only",
             "-Rpass-analysis=kernel-resource-usage", "-c"]
    tmp = tempfile.mkdtemp(prefix="h2r_res_")

    def compile_unit(tree, u):
        src = os.path.join(tree, "halo2_rsa_amd", "csrc", u + ".hip")
        if not os.path.exists(src):
            return ""
        out = os.path.join(tmp, "%s.%s.out" % (u, "p" if tree != ROOT else "b"))
        return subprocess.run(["hipcc"] + flags + ["-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "halo2_rsa_amd", "csrc"), "-o", out, src],
                              capture_output=True, text=True).stderr

    def parse(text):
        d, cur, names = {}, None, {}
        for line in text.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                d[cur] = {}
                continue
            m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
            if m and cur:
                d[cur][m.group(1).split()[0]] = int(m.group(2))
        if d:
            dem = subprocess.run(["c++filt"] + list(d), capture_output=True, text=True).stdout.splitlines()
            names = {k: re.sub(r"^void h2r::", "", n).split("(")[0] for k, n in zip(d, dem)}
        return {names[k]: v for k, v in d.items()}
    import concurrent.futures
    units = ["h2r_tu_chain", "h2r_tu_step", "h2r_tu_chain_keyed", "h2r_tu_step_keyed"]
    jobs = [(ROOT, u) for u in units] + ([(parent_tree, u) for u in units] if parent_tree else [])
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        texts = list(ex.map(lambda j: compile_unit(*j), jobs))
    br, pa = {}, {}
    for (tree, _u), t in zip(jobs, texts):
        (br if tree == ROOT else pa).update(parse(t))
    fmt = lambda v: "%3d VGPRs  %3d B scratch  occupancy %d" % (v["VGPRs"], v["ScratchSize"], v["Occupancy"]) if v else "-"
    print("%-52s %-44s %s" % ("kernel (last template argument on the branch: KEYED)", "parent", "branch"))
    for k in sorted(br):
        if not k.startswith(("chain_kernel", "chain_wave", "chain_dual", "step_", "key_table", "recip")):
            continue
        # a branch build without keys is the parent's build of the same name less the trailing KEYED = false
        pk = k[:-len(", false>")] + ">" if k.endswith(", false>") and k.startswith(("chain_kernel", "chain_wave", "step_")) else k
        pv = pa.get(pk)
        print("%-52s %-44s %s%s" % (k, fmt(pv), fmt(br[k]), "" if pv is None or pv == br[k] else "   <- differs"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", metavar="LIB")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--build-parent", nargs="?", const="HEAD", metavar="REV")
    ap.add_argument("--resources", nargs="?", const="", metavar="PARENT_TREE")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clock-calls", type=int, default=96)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a child process may take")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.steps, a.warmup, a.clock_calls)
    elif a.build_parent:
        build_parent(a.build_parent)
    elif a.resources is not None:
        resources(a.resources)
    elif a.run:
        run(a.reps, a.steps, a.warmup, a.clock_calls, a.out, a.step_timeout)
    else:
        ap.print_help()
