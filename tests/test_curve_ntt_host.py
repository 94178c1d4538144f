"""CPU-side checks of the Lagrange-key export (h2r_curve_ntt_workspace_bytes, h2r_curve_ntt's refusals, h2r_curve_eval ops 6 and 7; DESIGN.md
section 2k): every refusal next to a valid twin in the documented order, workspace_bytes zero exactly for what needs no ctx to refuse, the
two scalar multiplications of the butterflies -- run on the host by h2r_curve_eval in a host-only ctx -- against the plain model
(tests/msm_ref.py), and the library's export list against the header's.  No device work: a valid call on a host-only ctx ends in
H2R_E_UNSUPPORTED, its last check."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import curve_ntt_ref as C
import msm_ref as M
from pyref import FIELD_MODULI
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
BASE = 0x100000       # never dereferenced: the checks are host arithmetic on the addresses
R, R256 = M.R_ORDER, 1 << 256
OP_UNIFORM, OP_WINDOW = 6, 7


def host_ctx(field="bn254_fr", montgomery=False):
    ctx = ctypes.c_void_p()
    p = H2RParams(64, 256, _lib.FIELDS[field], -1)
    if montgomery:
        rep = _lib.H2RAdviceRepr()
        rep.struct_size, rep.flags = ctypes.sizeof(rep), _lib.H2R_ADVICE_MONTGOMERY
        assert lib().h2r_ctx_create_ex(ctypes.byref(p), ctypes.byref(rep), ctypes.byref(ctx)) == 0
    else:
        assert lib().h2r_ctx_create(ctypes.byref(p), ctypes.byref(ctx)) == 0
    return ctx


def config(log_n=10, flags=_lib.H2R_CURVE_NTT_INVERSE, reserved=0, struct_size=None, omega=None, modulus=R, montgomery=False):
    cfg = _lib.H2RCurveNttConfig()
    cfg.struct_size = ctypes.sizeof(cfg) if struct_size is None else struct_size
    cfg.log_n, cfg.flags, cfg.reserved = log_n, flags, reserved
    if omega is None:
        omega = C.NR.omega_of(modulus, log_n) if 0 < log_n <= 24 else 1
        if montgomery:
            omega = omega * R256 % modulus
    for i in range(4):
        cfg.omega[i] = (omega >> (64 * i)) & (2 ** 64 - 1)
    return cfg


def layout(cfg):
    """Disjoint, aligned device ranges for a call: (in, out, workspace)."""
    pts = 64 << min(cfg.log_n, 24)
    return BASE, BASE + pts + 256, BASE + 2 * (pts + 256)


def call(ctx, cfg, inp, out, ws):
    return lib().h2r_curve_ntt(ctx, ctypes.byref(cfg) if cfg is not None else None, inp, out, ws, None)


def test_workspace_bytes_is_zero_exactly_for_what_the_call_refuses_without_a_ctx():
    ctx = host_ctx()
    for log_n in (1, 2, 10, 17, 24):
        for flags in (0, _lib.H2R_CURVE_NTT_INVERSE):
            cfg = config(log_n, flags)
            need = lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(cfg))
            assert need >= (96 << log_n) + (16 << log_n), (log_n, need)                  # the projective points and the twiddles
            assert call(ctx, cfg, *layout(cfg)) == _lib.H2R_E_UNSUPPORTED                # valid up to the device
    for bad, want in ((config(0), _lib.H2R_E_SHAPE), (config(25), _lib.H2R_E_SHAPE), (config(reserved=1), _lib.H2R_E_SHAPE),
                      (config(flags=2), _lib.H2R_E_UNSUPPORTED), (config(flags=3), _lib.H2R_E_UNSUPPORTED),
                      (config(struct_size=40), _lib.H2R_E_UNSUPPORTED), (config(struct_size=56), _lib.H2R_E_UNSUPPORTED)):
        assert lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(bad)) == 0
        assert call(ctx, bad, *layout(bad)) == want
    assert lib().h2r_curve_ntt_workspace_bytes(None) == 0
    # omega needs the ctx's p: the size query cannot refuse it
    assert lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(config(omega=R))) > 0
    lib().h2r_ctx_destroy(ctx)


@pytest.mark.parametrize("montgomery", [False, True], ids=["canonical", "montgomery"])
def test_refusals_next_to_a_valid_twin(montgomery):
    """The valid twin reaches the last check (a host-only ctx: H2R_E_UNSUPPORTED); each refusal changes one thing."""
    ctx = host_ctx(montgomery=montgomery)
    NULL, SHAPE, UNSUP = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED
    cfg = config(montgomery=montgomery)
    inp, out, ws = layout(cfg)
    wsb = lib().h2r_curve_ntt_workspace_bytes(ctypes.byref(cfg))
    pts = 64 << cfg.log_n
    assert call(ctx, cfg, inp, out, ws) == UNSUP                              # the twin: everything but the device is right
    assert call(ctx, config(flags=0, montgomery=montgomery), inp, out, ws) == UNSUP
    # NULL pointers come first
    assert call(None, cfg, inp, out, ws) == NULL
    assert call(ctx, None, inp, out, ws) == NULL
    assert call(ctx, cfg, None, out, ws) == NULL
    assert call(ctx, cfg, inp, None, ws) == NULL
    assert call(ctx, cfg, inp, out, None) == NULL
    assert call(ctx, config(struct_size=8), None, out, ws) == NULL
    # struct_size and flags before the shapes
    assert call(ctx, config(0, struct_size=44), inp, out, ws) == UNSUP
    assert call(ctx, config(0, flags=4), inp, out, ws) == UNSUP
    # shapes: log_n, reserved, omega
    for bad in (config(0), config(25), config(reserved=9)):
        assert call(ctx, bad, *layout(bad)) == SHAPE
    big = config(24, montgomery=montgomery)
    assert call(ctx, big, *layout(big)) == UNSUP                              # (the largest legal size is not a shape error)
    assert call(ctx, config(omega=R), inp, out, ws) == SHAPE                  # omega >= p
    assert call(ctx, config(omega=(1 << 256) - 1), inp, out, ws) == SHAPE
    one = R256 % R if montgomery else 1
    assert call(ctx, config(omega=one), inp, out, ws) == SHAPE                # omega^(n/2) != -1: 1 ...
    assert call(ctx, config(omega=0), inp, out, ws) == SHAPE
    w11 = C.omega_of(11) * (R256 if montgomery else 1) % R
    assert call(ctx, config(omega=w11), inp, out, ws) == SHAPE                # ... a root of a larger order ...
    w9 = C.omega_of(9) * (R256 if montgomery else 1) % R
    assert call(ctx, config(omega=w9), inp, out, ws) == SHAPE                 # ... and of a smaller one
    assert call(ctx, config(11, omega=w11), *layout(config(11))) == UNSUP
    # the other representation's omega is another number
    other = C.omega_of(10) * (1 if montgomery else R256) % R
    assert call(ctx, config(omega=other), inp, out, ws) == SHAPE
    # alignment
    assert call(ctx, cfg, inp + 8, out, ws) == SHAPE
    assert call(ctx, cfg, inp, out + 8, ws) == SHAPE
    assert call(ctx, cfg, inp, out, ws + 8) == SHAPE
    assert call(ctx, cfg, inp + 16, out + 16, ws + 16) == UNSUP
    # overlaps: in / out, in / workspace, out / workspace, by their last 16 bytes and whole
    assert call(ctx, cfg, inp, inp, ws) == SHAPE
    assert call(ctx, cfg, inp, inp + pts - 16, ws) == SHAPE
    assert call(ctx, cfg, inp + pts - 16, out + 2 * pts, inp + 4 * pts + 4096) == UNSUP
    assert call(ctx, cfg, out + pts - 16, out, ws) == SHAPE
    assert call(ctx, cfg, inp, out, inp + pts - 16) == SHAPE
    assert call(ctx, cfg, ws + wsb - 16, out, ws) == SHAPE
    assert call(ctx, cfg, inp, ws + wsb - 16, ws) == SHAPE
    assert call(ctx, cfg, inp, out, out + pts - 16) == SHAPE
    assert call(ctx, cfg, inp, inp + pts, inp + 2 * pts) == UNSUP             # adjacent is not overlapping
    assert call(ctx, cfg, ws + wsb, out, ws) == UNSUP
    lib().h2r_ctx_destroy(ctx)
    # a field without a curve: after the shape checks, before the host-only ctx (which every ctx here is)
    for field in ("pasta_fp", "pasta_fq"):                                    # (bn254_fq has no 2^10-th root of unity to offer)
        other_ctx = host_ctx(field, montgomery)
        good = config(modulus=FIELD_MODULI[field], montgomery=montgomery)
        assert call(other_ctx, good, inp, out, ws) == UNSUP
        assert call(other_ctx, good, inp + 8, out, ws) == SHAPE              # ... after the shape checks
        assert call(other_ctx, good, inp, inp, ws) == SHAPE
        lib().h2r_ctx_destroy(other_ctx)


def _arr(vals):
    return (ctypes.c_uint64 * (4 * len(vals)))(*[w for v in vals for w in M.words(v)])


def _proj(p, rng):
    lam = rng.randrange(1, M.Q)
    return [0, lam, 0] if p == M.IDENT else [p[0] * lam % M.Q, p[1] * lam % M.Q, lam]


def _mul(ctx, op, k, P):
    out = (ctypes.c_uint64 * 12)()
    assert lib().h2r_curve_eval(ctx, op, _arr(P), _arr([k]), out) == 0
    vals = [sum(int(out[4 * i + j]) << (64 * j) for j in range(4)) for i in range(3)]
    assert all(v < M.Q for v in vals)
    return M.proj_to_affine(*vals)


@pytest.fixture(scope="module")
def ctx():
    c = host_ctx()
    yield c
    lib().h2r_ctx_destroy(c)


@pytest.mark.parametrize("op", [OP_UNIFORM, OP_WINDOW], ids=["uniform", "window2"])
def test_the_butterflies_scalar_multiplication_on_edge_scalars(ctx, op):
    rng = random.Random("curve_ntt/host/edge/%d" % op)
    for p in M.mul_g_batch([1, 2, rng.randrange(1, R)]):
        P, O = _proj(p, rng), _proj(M.IDENT, rng)
        for k in (0, 1, 2, 3, R - 1, R, R + 1, (1 << 256) - 1, 1 << 255, 1 << 254, 0x5555 << 240, 0xAAAA << 240, 0xFFFF):
            assert _mul(ctx, op, k, P) == M.mul(k % R, p), k
            assert _mul(ctx, op, k, O) == M.IDENT, k                           # the identity as P
    out = (ctypes.c_uint64 * 12)()
    assert lib().h2r_curve_eval(ctx, op, _arr(_proj(M.G, rng)), _arr([0]), out) == 0
    assert not any(out[8:12]), "0 * P is Z = 0"


@pytest.mark.parametrize("op", [OP_UNIFORM, OP_WINDOW], ids=["uniform", "window2"])
def test_the_butterflies_scalar_multiplication_on_random_pairs(ctx, op):
    rng = random.Random("curve_ntt/host/random/%d" % op)
    pts = M.mul_g_batch([rng.randrange(1, R) for _ in range(12)])
    for i, p in enumerate(pts):
        k = rng.getrandbits(256) if i % 2 else rng.randrange(R)
        assert _mul(ctx, op, k, _proj(p, rng)) == M.mul(k % R, p)
    # the twiddles themselves: powers of the domain's roots
    for log_n in (2, 7, 17):
        w = C.omega_of(log_n)
        k = pow(w, rng.randrange(1, 1 << (log_n - 1)), R)
        assert _mul(ctx, op, k, _proj(pts[0], rng)) == M.mul(k, pts[0])


def test_the_new_ops_refusals(ctx):
    out = (ctypes.c_uint64 * 12)()
    rng = random.Random(1)
    P = _arr(_proj(M.G, rng))
    for op in (OP_UNIFORM, OP_WINDOW):
        assert lib().h2r_curve_eval(ctx, op, P, None, out) == _lib.H2R_E_NULL
        assert lib().h2r_curve_eval(ctx, op, None, _arr([1]), out) == _lib.H2R_E_NULL
        assert lib().h2r_curve_eval(ctx, op, _arr([M.Q, 2, 1]), _arr([1]), out) == _lib.H2R_E_SHAPE
        other = host_ctx("bn254_fq")
        assert lib().h2r_curve_eval(other, op, P, _arr([1]), out) == _lib.H2R_E_UNSUPPORTED
        lib().h2r_ctx_destroy(other)
    assert lib().h2r_curve_eval(ctx, 8, P, _arr([1]), out) == _lib.H2R_E_SHAPE


def test_the_export_list_equals_the_headers():
    hdr = open(os.path.join(ROOT, "include", "h2r.h")).read()
    declared = sorted(set(re.findall(r"\b(h2r_[a-z0-9_]+)\s*\(", hdr)))
    assert "h2r_curve_ntt" in declared and "h2r_curve_ntt_workspace_bytes" in declared
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == declared == sorted(_lib.EXPORTS), sorted(set(exported) ^ set(declared))
    assert lib().h2r_abi_version() == 5
