"""CPU-side checks of the commitments' exports (h2r_msm_plan, h2r_msm_workspace_bytes, h2r_msm_columns' refusals, h2r_curve_eval; DESIGN.md
section 2i): every refusal next to a valid twin, plan / workspace consistency, and the curve formulas the kernels inline -- run on the
host by h2r_curve_eval in a host-only ctx -- against the plain model (tests/msm_ref.py) on random points and on every exceptional pair.
No device work: a valid call on a host-only ctx ends in H2R_E_UNSUPPORTED, its last check."""
import ctypes
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_ref as M
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib

BASE = 0x10000        # never dereferenced: the checks are host arithmetic on the addresses


def host_ctx(field="bn254_fr"):
    ctx = ctypes.c_void_p()
    p = H2RParams(64, 256, _lib.FIELDS[field], -1)
    assert lib().h2r_ctx_create(ctypes.byref(p), ctypes.byref(ctx)) == 0
    return ctx


def config(n=1000, num_cols=2, reserved=0, struct_size=None):
    cfg = _lib.H2RMsmConfig()
    cfg.struct_size = ctypes.sizeof(cfg) if struct_size is None else struct_size
    cfg.n, cfg.num_cols, cfg.reserved = n, num_cols, reserved
    return cfg


def layout(cfg, batch, col_stride=None):
    """Disjoint, aligned device ranges for a call: (descriptors, bases, out, workspace)."""
    col = 32 * cfg.n
    stride = col if col_stride is None else col_stride
    cols = (_lib.H2RMsmColumn * max(cfg.num_cols, 1))()
    at = BASE
    for c in range(min(cfg.num_cols, len(cols))):
        cols[c].base, cols[c].elem_stride = at, stride
        at += max(batch, 1) * max(stride, col) + 256
    bases = at
    at += 64 * cfg.n + 256
    out = at
    at += max(batch, 1) * max(cfg.num_cols, 1) * 64 + 256
    return cols, bases, out, at


def call(ctx, cfg, cols, bases, out, ws, batch=2, status=None):
    return lib().h2r_msm_columns(ctx, ctypes.byref(cfg) if cfg is not None else None, cols, bases, batch, out, status, ws, None)


def test_plan_and_workspace_agree_and_refused_configurations_answer_zero():
    info = _lib.H2RMsmInfo()
    for n in (1, 2, 1000, 1 << 17, (1 << 17) + 1, 1 << 24):
        for num_cols, batch in ((1, 1), (30, 8), (64, 65535)):
            cfg = config(n, num_cols)
            got = lib().h2r_msm_plan(ctypes.byref(cfg), batch, ctypes.byref(info))
            assert got == info.workspace_bytes == lib().h2r_msm_workspace_bytes(ctypes.byref(cfg), batch) and got > 0
            assert (info.window_bits, info.num_windows) == (8, 32) and info.window_bits * info.num_windows == 256
            assert 256 <= info.slice_points <= 65536
            assert info.num_slices == -(-n // info.slice_points)
            assert got >= batch * num_cols * info.num_windows * info.num_slices * 96
    cfg = config(1000, 3)
    assert lib().h2r_msm_plan(ctypes.byref(cfg), 0, ctypes.byref(info)) > 0            # batch 0 is a legal call
    for bad, batch in ((config(0, 1), 1), (config((1 << 24) + 1, 1), 1), (config(10, 0), 1), (config(10, 65), 1), (config(10, 1, reserved=1), 1),
                       (config(10, 1, struct_size=12), 1), (config(10, 1), 65536)):
        info.slice_points = 12345
        assert lib().h2r_msm_plan(ctypes.byref(bad), batch, ctypes.byref(info)) == 0 and info.slice_points == 12345
        assert lib().h2r_msm_workspace_bytes(ctypes.byref(bad), batch) == 0
    assert lib().h2r_msm_plan(None, 1, ctypes.byref(info)) == 0 and lib().h2r_msm_plan(ctypes.byref(cfg), 1, None) == 0
    assert lib().h2r_msm_workspace_bytes(None, 1) == 0


def test_refusals_next_to_a_valid_twin():
    """The valid twin reaches the last check (a host-only ctx: H2R_E_UNSUPPORTED); each refusal changes one thing."""
    ctx = host_ctx()
    NULL, SHAPE, UNSUP = _lib.H2R_E_NULL, _lib.H2R_E_SHAPE, _lib.H2R_E_UNSUPPORTED
    cfg = config()
    cols, bases, out, ws = layout(cfg, 2)
    assert call(ctx, cfg, cols, bases, out, ws) == UNSUP                      # the twin: everything but the device is right
    # NULL required pointers (status is optional)
    assert call(None, cfg, cols, bases, out, ws) == NULL
    assert call(ctx, None, cols, bases, out, ws) == NULL
    assert call(ctx, cfg, None, bases, out, ws) == NULL
    assert call(ctx, cfg, cols, None, out, ws) == NULL
    assert call(ctx, cfg, cols, bases, None, ws) == NULL
    assert call(ctx, cfg, cols, bases, out, None) == NULL
    c2, *_ = layout(cfg, 2)
    c2[1].base = None
    assert call(ctx, cfg, c2, bases, out, ws) == NULL
    # shapes
    for bad in (config(0), config((1 << 24) + 1), config(num_cols=0), config(num_cols=65), config(reserved=7)):
        bc, bb, bo, bw = layout(bad, 2)
        assert call(ctx, bad, bc, bb, bo, bw) == SHAPE, (bad.n, bad.num_cols, bad.reserved)
    big = config(1 << 24, 64)
    bc, bb, bo, bw = layout(big, 2)
    assert call(ctx, big, bc, bb, bo, bw) == UNSUP                            # (the largest legal shape is not a shape error)
    # alignment: a column base, a stride, the bases, out, the workspace
    c2, *_ = layout(cfg, 2)
    c2[0].base += 8
    assert call(ctx, cfg, c2, bases, out, ws) == SHAPE
    c2, *_ = layout(cfg, 2)
    c2[1].elem_stride += 8
    assert call(ctx, cfg, c2, bases, out, ws) == SHAPE
    assert call(ctx, cfg, cols, bases + 8, out, ws) == SHAPE
    assert call(ctx, cfg, cols, bases, out + 8, ws) == SHAPE
    assert call(ctx, cfg, cols, bases, out, ws + 8) == SHAPE
    # a nonzero stride smaller than the column; zero is one copy for the batch
    c2, *_ = layout(cfg, 2)
    c2[0].elem_stride = 32 * cfg.n - 16
    assert call(ctx, cfg, c2, bases, out, ws) == SHAPE
    c2[0].elem_stride = 0
    assert call(ctx, cfg, c2, bases, out, ws) == UNSUP
    # overlaps: out / workspace with a column (its second circuit's copy included), the bases, each other
    wsb = lib().h2r_msm_workspace_bytes(ctypes.byref(cfg), 2)
    col = 32 * cfg.n
    assert call(ctx, cfg, cols, bases, cols[0].base + 2 * col - 64, ws) == SHAPE          # the last bytes of circuit 1's column 0
    assert call(ctx, cfg, cols, bases, cols[1].base, ws) == SHAPE
    assert call(ctx, cfg, cols, bases, out, cols[1].base - wsb + 16) == SHAPE              # the workspace's last bytes reach column 1
    assert call(ctx, cfg, cols, bases, bases + 64 * cfg.n - 64, ws) == SHAPE
    assert call(ctx, cfg, cols, bases, out, bases - wsb + 16) == SHAPE
    assert call(ctx, cfg, cols, bases, out, out + 2 * cfg.num_cols * 64 - 16) == SHAPE
    assert call(ctx, cfg, cols, bases, ws + 16, ws) == SHAPE
    assert call(ctx, cfg, cols, bases, out, out + 2 * cfg.num_cols * 64) == UNSUP          # adjacent is not overlapping
    # unsupported: another struct_size (before everything else), too many circuits, a field without a curve, the host-only ctx last
    assert call(ctx, config(struct_size=20), cols, bases, out, ws) == UNSUP
    assert call(ctx, config(0, struct_size=20), cols, bases, out, ws) == UNSUP
    c3, b3, o3, w3 = layout(cfg, 65536)
    assert call(ctx, cfg, c3, b3, o3, w3, batch=65536) == UNSUP
    for field in ("bn254_fq", "pasta_fp", "pasta_fq"):
        other = host_ctx(field)
        assert call(other, cfg, cols, bases, out, ws) == UNSUP
        assert call(other, config(0), cols, bases, out, ws) == SHAPE                      # ... after the shape checks
        lib().h2r_ctx_destroy(other)
    assert call(ctx, cfg, cols, bases, out, ws, batch=0) == UNSUP                          # batch 0 still needs a device ctx
    lib().h2r_ctx_destroy(ctx)


def _arr(vals):
    return (ctypes.c_uint64 * (4 * len(vals)))(*[w for v in vals for w in M.words(v)])


def _ints(a, k):
    return [sum(int(a[4 * i + j]) << (64 * j) for j in range(4)) for i in range(k)]


def _proj(p, rng=None):
    """An affine point as a projective triple, scaled by a random Z where a generator is given."""
    if p == M.IDENT:
        lam = rng.randrange(1, M.Q) if rng else 1
        return [0, lam, 0]
    lam = rng.randrange(1, M.Q) if rng else 1
    return [p[0] * lam % M.Q, p[1] * lam % M.Q, lam]


class Curve:
    def __init__(self, ctx):
        self.ctx = ctx

    def op(self, op, a, b=None, n_out=3):
        out = (ctypes.c_uint64 * (4 * n_out))()
        rc = lib().h2r_curve_eval(self.ctx, op, _arr(a), _arr(b) if b is not None else None, out)
        assert rc == 0, (op, rc)
        vals = _ints(out, n_out)
        assert all(v < M.Q for v in vals)
        return vals

    def add(self, p, q):
        return M.proj_to_affine(*self.op(0, p, q))

    def mixed(self, p, q_aff):
        return M.proj_to_affine(*self.op(1, p, list(q_aff)))

    def double(self, p):
        return M.proj_to_affine(*self.op(2, p))

    def affine(self, p):
        return tuple(self.op(3, p, n_out=2))

    def mul(self, k, p):
        return M.proj_to_affine(*self.op(4, p, [k]))


@pytest.fixture(scope="module")
def curve():
    ctx = host_ctx()
    yield Curve(ctx)
    lib().h2r_ctx_destroy(ctx)


def test_curve_formulas_on_random_points(curve):
    rng = random.Random("msm/host/random")
    pts = M.mul_g_batch([rng.randrange(1, M.R_ORDER) for _ in range(24)])
    for i, p in enumerate(pts):
        q = pts[(5 * i + 1) % len(pts)]
        want = M.add(p, q)
        assert curve.add(_proj(p, rng), _proj(q, rng)) == want
        assert curve.mixed(_proj(p, rng), q) == want
        assert curve.double(_proj(p, rng)) == M.add(p, p)
        assert curve.affine(_proj(p, rng)) == p
        k = rng.getrandbits(256)
        assert curve.mul(k, _proj(p, rng)) == M.mul(k % M.R_ORDER, p)


def test_curve_formulas_on_every_exceptional_pair(curve):
    rng = random.Random("msm/host/exceptional")
    for p in M.mul_g_batch([1, 2, rng.randrange(1, M.R_ORDER)]):
        P, N, O = _proj(p, rng), _proj(M.neg(p), rng), _proj(M.IDENT, rng)
        assert curve.add(P, _proj(p, rng)) == M.add(p, p)                      # P + P
        assert curve.add(P, P) == M.add(p, p)
        assert curve.mixed(P, p) == M.add(p, p)
        assert curve.add(P, N) == M.IDENT                                      # P + (-P)
        assert curve.mixed(P, M.neg(p)) == M.IDENT
        assert curve.op(0, P, N)[2] == 0                                       # ... is Z = 0, and to-affine sends it to (0, 0)
        assert curve.affine(curve.op(0, P, N)) == M.IDENT
        assert curve.add(O, P) == p and curve.add(P, O) == p                   # the identity on either side
        assert curve.add(O, _proj(M.IDENT, rng)) == M.IDENT
        assert curve.mixed(O, p) == p
        assert curve.mixed(P, M.IDENT) == p and curve.mixed(O, M.IDENT) == M.IDENT   # mixed add of (0, 0): skipped
        assert curve.double(O) == M.IDENT                                      # doubling the identity
        assert curve.affine(O) == M.IDENT
        for k in (0, 1, M.R_ORDER - 1, M.R_ORDER, (1 << 256) - 1, 255, 256, 1 << 248):
            assert curve.mul(k, P) == M.mul(k % M.R_ORDER, p), k
        assert curve.mul(rng.getrandbits(256), O) == M.IDENT


def test_curve_eval_refusals(curve):
    out = (ctypes.c_uint64 * 12)()
    P = _arr(_proj(M.G))
    assert lib().h2r_curve_eval(None, 0, P, P, out) == _lib.H2R_E_NULL
    assert lib().h2r_curve_eval(curve.ctx, 0, P, None, out) == _lib.H2R_E_NULL
    assert lib().h2r_curve_eval(curve.ctx, 2, None, None, out) == _lib.H2R_E_NULL
    assert lib().h2r_curve_eval(curve.ctx, 2, P, None, None) == _lib.H2R_E_NULL
    assert lib().h2r_curve_eval(curve.ctx, 2, P, None, out) == _lib.H2R_OK
    assert lib().h2r_curve_eval(curve.ctx, 5, P, P, out) == _lib.H2R_E_SHAPE
    assert lib().h2r_curve_eval(curve.ctx, 2, _arr([M.Q, 2, 1]), None, out) == _lib.H2R_E_SHAPE       # canonical coordinates only
    assert lib().h2r_curve_eval(curve.ctx, 1, P, _arr([1, M.Q]), out) == _lib.H2R_E_SHAPE
    for field in ("bn254_fq", "pasta_fp", "pasta_fq"):
        other = host_ctx(field)
        assert lib().h2r_curve_eval(other, 2, P, None, out) == _lib.H2R_E_UNSUPPORTED
        lib().h2r_ctx_destroy(other)
