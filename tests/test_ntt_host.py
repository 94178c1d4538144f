"""Host-side checks of the evaluation domain's exports (h2r_ntt_workspace_bytes, h2r_ntt_columns): argument checking only, no device work.
A host-only ctx is refused with H2R_E_UNSUPPORTED only after its arguments were found well-formed, so every H2R_E_NULL, H2R_E_SHAPE and
H2R_E_UNSUPPORTED cause shows without a device, each next to a valid twin that differs in that one field and reaches the host-only refusal."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import ntt_ref as NR
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib
from pyref import FIELD_MODULI

FIELD_IDS = {"bn254_fr": 0, "bn254_fq": 1, "pasta_fp": 2, "pasta_fq": 3}
R256 = 1 << 256
K = 6
COL = (1 << K) * 32
OK = _lib.H2R_E_UNSUPPORTED      # what a well-formed call meets on a host-only ctx


def host_ctx(field="bn254_fr", flags=0):
    ctx = ctypes.c_void_p()
    p = H2RParams(64, 256, FIELD_IDS[field], -1)
    rp = _lib.H2RAdviceRepr(ctypes.sizeof(_lib.H2RAdviceRepr), flags, 0)
    assert lib().h2r_ctx_create_ex(ctypes.byref(p), ctypes.byref(rp), ctypes.byref(ctx)) == 0
    return ctx


def fe(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)])


def config(field="bn254_fr", log_in=K, log_out=K, flags=0, omega=None, shift=1, struct_size=None):
    cfg = _lib.H2RNttConfig()
    cfg.struct_size = ctypes.sizeof(cfg) if struct_size is None else struct_size
    cfg.log_n_in, cfg.log_n_out, cfg.flags = log_in, log_out, flags
    cfg.omega = fe(NR.omega_of(FIELD_MODULI[field], log_out) if omega is None else omega)
    cfg.shift = fe(shift)
    return cfg


BUF = (ctypes.c_uint64 * 64)()          # ctypes aligns the array to 8 bytes only: the calls below take a 16-byte aligned address inside it
ALIGNED = (ctypes.addressof(BUF) + 15) & ~15
FAR = ALIGNED + (1 << 40)               # never dereferenced: no device work happens on a host-only ctx


def call(ctx, cfg, **kw):
    """The export with well-formed arguments (2 elements x 3 columns, [element][column] on both sides), overridden by name."""
    a = dict(src=ALIGNED, in_es=3 * COL, in_cs=COL, dst=FAR, out_es=3 * COL, out_cs=COL, num_cols=3, batch=2, ws=ALIGNED)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib().h2r_ntt_columns(ctx, ctypes.byref(cfg) if cfg is not None else None, a["src"], a["in_es"], a["in_cs"], a["dst"], a["out_es"],
                                 a["out_cs"], a["num_cols"], a["batch"], a["ws"], None)


@pytest.fixture
def ctx():
    c = host_ctx()
    yield c
    lib().h2r_ctx_destroy(c)


def test_valid_calls_reach_the_host_only_refusal(ctx):
    assert call(ctx, config()) == OK
    assert call(ctx, config(flags=_lib.H2R_NTT_INVERSE)) == OK
    assert call(ctx, config(log_in=K - 2), in_es=3 * COL // 4, in_cs=COL // 4) == OK              # fewer coefficients than points
    assert call(ctx, config(log_in=0), in_es=96, in_cs=32) == OK                                    # one coefficient
    assert call(ctx, config(shift=FIELD_MODULI["bn254_fr"] - 1)) == OK
    assert call(ctx, config(log_in=24, log_out=24), in_es=3 << 29, in_cs=1 << 29, out_es=3 << 29, out_cs=1 << 29, dst=ALIGNED + (1 << 50)) == OK
    assert call(ctx, config(), batch=0) == OK                                                       # (batch = 0 is H2R_OK on a device ctx: no launch)


def test_null_pointers(ctx):
    cfg = config()
    assert call(None, cfg) == _lib.H2R_E_NULL
    assert call(ctx, None) == _lib.H2R_E_NULL
    for hole in ("src", "dst", "ws"):
        assert call(ctx, cfg, **{hole: None}) == _lib.H2R_E_NULL, hole
    assert lib().h2r_ntt_workspace_bytes(None) == 0


def test_unsupported_causes(ctx):
    size = ctypes.sizeof(_lib.H2RNttConfig)
    for cfg in (config(struct_size=size + 8), config(struct_size=0), config(flags=2), config(flags=_lib.H2R_NTT_INVERSE | 0x80000000)):
        assert call(ctx, cfg) == _lib.H2R_E_UNSUPPORTED
        assert call(ctx, cfg, num_cols=0) == _lib.H2R_E_UNSUPPORTED      # not the host-only refusal: it comes before the shape checks
        assert lib().h2r_ntt_workspace_bytes(ctypes.byref(cfg)) == 0


P_FR = FIELD_MODULI["bn254_fr"]
SHAPE_CAUSES = [   # (what, config overrides, call overrides)
    ("log_n_out = 0", dict(log_in=0, log_out=0, omega=1), dict(in_es=96, in_cs=32, out_es=96, out_cs=32)),
    ("log_n_out > 24", dict(log_in=25, log_out=25, omega=NR.omega_of(P_FR, 25)), dict(in_es=3 << 30, in_cs=1 << 30, out_es=3 << 30, out_cs=1 << 30, dst=ALIGNED + (1 << 50))),
    ("log_n_in > log_n_out", dict(log_in=K + 1), dict(in_es=6 * COL, in_cs=2 * COL)),
    ("inverse with log_n_in != log_n_out", dict(log_in=K - 1, flags=_lib.H2R_NTT_INVERSE), dict()),
    ("num_cols = 0", dict(), dict(num_cols=0)),
    ("omega = p", dict(omega=P_FR), dict()),
    ("omega > p", dict(omega=P_FR + NR.omega_of(P_FR, K)), dict()),
    ("shift = p", dict(shift=P_FR), dict()),
    ("shift = 0", dict(shift=0), dict()),
    ("omega = 1", dict(omega=1), dict()),
    ("omega = -1 at k > 1", dict(omega=P_FR - 1), dict()),
    ("omega of order 2^(k-1)", dict(omega=NR.omega_of(P_FR, K - 1)), dict()),
    ("omega of order 2^(k+1)", dict(omega=NR.omega_of(P_FR, K + 1)), dict()),
    ("omega not a root of unity", dict(omega=5), dict()),
    ("in not aligned", dict(), dict(src=ALIGNED + 8)),
    ("in_elem_stride not aligned", dict(), dict(in_es=3 * COL + 8)),
    ("in_col_stride not aligned", dict(), dict(in_cs=COL + 4, in_es=4 * COL)),
    ("out not aligned", dict(), dict(dst=FAR + 8)),
    ("out_elem_stride not aligned", dict(), dict(out_es=3 * COL + 8)),
    ("out_col_stride not aligned", dict(), dict(out_cs=COL + 8, out_es=4 * COL)),
    ("in_col_stride smaller than the column", dict(), dict(in_cs=COL - 16)),
    ("in_elem_stride smaller than the column", dict(), dict(in_es=COL - 16, in_cs=2 * COL)),
    ("out_col_stride smaller than the column", dict(), dict(out_cs=COL - 32)),
    ("out_elem_stride smaller than the column", dict(), dict(out_es=COL - 16, out_cs=2 * COL)),
    ("in_elem_stride does not cover the columns", dict(), dict(in_es=2 * COL)),
    ("out_elem_stride does not cover the columns", dict(), dict(out_es=3 * COL - 16)),
    ("[column][element] with a column stride that does not cover the batch", dict(), dict(out_es=COL, out_cs=2 * COL - 16)),
    ("out starts inside in", dict(), dict(dst=ALIGNED + 6 * COL - 16)),
    ("in starts inside out", dict(), dict(src=FAR + 6 * COL - 16)),
    ("in == out", dict(), dict(dst=ALIGNED)),
    ("out inside a gap of in", dict(), dict(in_es=8 * COL, dst=ALIGNED + 4 * COL)),
]


@pytest.mark.parametrize("what,cfg_kw,call_kw", SHAPE_CAUSES, ids=[c[0] for c in SHAPE_CAUSES])
def test_shape_causes(ctx, what, cfg_kw, call_kw):
    assert call(ctx, config(**cfg_kw), **call_kw) == _lib.H2R_E_SHAPE


def test_valid_twins_of_the_shape_causes(ctx):
    """What lies just inside each bound above comes through the argument checks."""
    assert call(ctx, config(log_in=0, log_out=1), in_es=96, in_cs=32, out_es=192, out_cs=64) == OK
    assert call(ctx, config(log_in=K - 1, flags=0), in_es=3 * COL // 2, in_cs=COL // 2) == OK
    assert call(ctx, config(), num_cols=1) == OK
    assert call(ctx, config(omega=P_FR - NR.omega_of(P_FR, K))) == OK                              # -omega: also primitive
    assert call(ctx, config(shift=P_FR - 1)) == OK
    assert call(ctx, config(), in_cs=COL + 16, in_es=3 * COL + 32) == OK
    assert call(ctx, config(), out_cs=COL + 16, out_es=3 * COL + 32) == OK
    assert call(ctx, config(), in_es=COL, in_cs=2 * COL) == OK                                     # [column][element]
    assert call(ctx, config(), out_es=COL, out_cs=2 * COL) == OK
    assert call(ctx, config(), out_es=COL + 16, out_cs=2 * COL + 16) == OK
    assert call(ctx, config(), dst=ALIGNED + 6 * COL) == OK                                        # out begins where in ends
    assert call(ctx, config(), src=FAR + 6 * COL) == OK
    assert call(ctx, config(), batch=0, dst=ALIGNED) == OK                                         # no elements: nothing overlaps


@pytest.mark.parametrize("flags", [0, _lib.H2R_ADVICE_MONTGOMERY], ids=["canonical", "montgomery"])
def test_omega_and_shift_are_in_the_ctx_representation(flags):
    c = host_ctx(flags=flags)
    w = NR.omega_of(P_FR, K)
    conv = (lambda v: v * R256 % P_FR) if flags else (lambda v: v)
    other = (lambda v: v) if flags else (lambda v: v * R256 % P_FR)
    assert call(c, config(omega=conv(w), shift=conv(7))) == OK
    assert call(c, config(omega=other(w), shift=conv(7))) == _lib.H2R_E_SHAPE                      # the same root in the other representation is no root here
    lib().h2r_ctx_destroy(c)


def test_fields():
    for field in NR.FIELDS_WITH_DOMAINS:
        c = host_ctx(field)
        assert call(c, config(field)) == OK, field
        assert call(c, config(field, omega=NR.omega_of(FIELD_MODULI[field], K - 1))) == _lib.H2R_E_SHAPE, field
        lib().h2r_ctx_destroy(c)
    # bn256 Fq: p - 1 = 2 * odd, so -1 generates the only domain there is
    pq = FIELD_MODULI["bn254_fq"]
    c = host_ctx("bn254_fq")
    assert call(c, config("bn254_fq", log_in=1, log_out=1, omega=pq - 1), in_es=192, in_cs=64, out_es=192, out_cs=64) == OK
    for w in (pq - 1, 1, 2, 3, 5, pow(3, (pq - 1) // 2, pq), pow(7, (pq - 1) // 6, pq), 0x1234567 ** 7 % pq):
        assert call(c, config("bn254_fq", log_in=2, log_out=2, omega=w), in_es=384, in_cs=128, out_es=384, out_cs=128) == _lib.H2R_E_SHAPE, w
    lib().h2r_ctx_destroy(c)


def test_workspace_bytes():
    ws = lib().h2r_ntt_workspace_bytes
    sizes = {ws(ctypes.byref(config(log_in=k, log_out=k))) for k in (1, 6, 10, 11, 20, 24)}
    assert 0 not in sizes and max(sizes) < 1 << 20                                                  # tables, not columns
    assert ws(ctypes.byref(config(log_in=3, log_out=24, shift=5))) > 0
    assert ws(ctypes.byref(config(flags=_lib.H2R_NTT_INVERSE))) > 0
    # 0 exactly for what the call refuses whatever the ctx
    for bad in (dict(log_in=0, log_out=0, omega=1), dict(log_in=25, log_out=25, omega=1), dict(log_in=K + 1), dict(log_in=K - 1, flags=_lib.H2R_NTT_INVERSE),
                dict(shift=0), dict(flags=4), dict(struct_size=8)):
        assert ws(ctypes.byref(config(**bad))) == 0, bad
    # omega and shift are compared with the ctx's p by the call: the host function has no ctx
    assert ws(ctypes.byref(config(omega=1))) > 0 and ws(ctypes.byref(config(shift=P_FR))) > 0
