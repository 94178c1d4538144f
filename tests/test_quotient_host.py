"""Host-side checks of the vanishing argument's exports (h2r_quotient_sets, h2r_quotient_columns): argument checking only, no device work.
A host-only ctx is refused with H2R_E_UNSUPPORTED only after its arguments were found well-formed, so every H2R_E_NULL, H2R_E_SHAPE and
H2R_E_UNSUPPORTED cause shows without a device, each next to a valid twin that differs in that one field and reaches the host-only refusal."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import ntt_ref as NR
import permutation_ref as PR
from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib
from pyref import FIELD_MODULI

FIELD_IDS = {"bn254_fr": 0, "bn254_fq": 1, "pasta_fp": 2, "pasta_fq": 3}
R256 = 1 << 256
K, EK = 4, 6
COL = (1 << EK) * 32
OK = _lib.H2R_E_UNSUPPORTED      # what a well-formed call meets on a host-only ctx
P_FR = FIELD_MODULI["bn254_fr"]


def host_ctx(field="bn254_fr", flags=0):
    ctx = ctypes.c_void_p()
    p = H2RParams(64, 256, FIELD_IDS[field], -1)
    rp = _lib.H2RAdviceRepr(ctypes.sizeof(_lib.H2RAdviceRepr), flags, 0)
    assert lib().h2r_ctx_create_ex(ctypes.byref(p), ctypes.byref(rp), ctypes.byref(ctx)) == 0
    return ctx


def fe(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)])


def config(field="bn254_fr", log_n=K, log_ext=EK, bf=5, omega_ext=None, zeta=None, delta=None, num_fixed=15, gate_fixed=range(9), column_src=(0, 1, 2, 3, 4, 5),
           chunk_len=2, n_extra=1, lookup_mask=31, lookup_advice=(0, 1, 2, 3, 0), lookup_tag=(11, 11, 11, 11, 13), lookup_enable=(12, 12, 12, 12, 14),
           table_tag=9, table_value=10, struct_size=None, num_columns=None):
    P = FIELD_MODULI[field]
    cfg = _lib.H2RQuotientConfig()
    cfg.struct_size = ctypes.sizeof(cfg) if struct_size is None else struct_size
    cfg.log_n, cfg.log_ext, cfg.blinding_factors = log_n, log_ext, bf
    cfg.omega_ext = fe(NR.omega_of(P, min(log_ext, 28)) if omega_ext is None else omega_ext)
    cfg.zeta = fe(NR.cube_root_of_unity(P) if zeta is None else zeta)
    cfg.delta = fe(PR.domain(P, 1)[1] if delta is None else delta)
    cfg.num_fixed, cfg.chunk_len, cfg.n_extra, cfg.lookup_mask = num_fixed, chunk_len, n_extra, lookup_mask
    cfg.num_columns = len(column_src) if num_columns is None else num_columns
    for i, v in enumerate(gate_fixed):
        cfg.gate_fixed[i] = v
    for i, v in enumerate(column_src):
        cfg.column_src[i] = v
    for k in range(5):
        cfg.lookup_advice[k], cfg.lookup_tag[k], cfg.lookup_enable[k] = lookup_advice[k], lookup_tag[k], lookup_enable[k]
    cfg.table_tag, cfg.table_value = table_tag, table_value
    return cfg


BUF = (ctypes.c_uint64 * 64)()          # ctypes aligns the array to 8 bytes only: the calls below take a 16-byte aligned address inside it
ALIGNED = (ctypes.addressof(BUF) + 15) & ~15
GB = 1 << 30                            # the groups lie a gigabyte apart: never dereferenced, no device work happens on a host-only ctx
BATCH = 2
GROUP_COLS = dict(advice=5, extra=1, perm_z=3, lookup_a_perm=5, lookup_s_perm=5, lookup_z=5, fixed=15, sigma=6, l=3)
H_AT = ALIGNED + 16 * GB


def inputs(col=COL, **kw):
    """Well-formed inputs ([circuit][column] in every per-circuit group), a group's fields overridden as name=(base, elem_stride, col_stride) with
    None = as it was, or a challenge pointer as name=address."""
    inp = _lib.H2RQuotientInputs()
    for i, name in enumerate(_lib.H2RQuotientInputs.GROUPS):
        g = getattr(inp, name)
        g.base, g.elem_stride, g.col_stride = ALIGNED + (i + 1) * GB, GROUP_COLS[name] * col, col
        if name in kw:
            for field, v in zip(("base", "elem_stride", "col_stride"), kw.pop(name)):
                if v is not None:
                    setattr(g, field, None if v == 0 and field == "base" else v)
    for name in _lib.H2RQuotientInputs.CHALLENGES:
        setattr(inp, name, kw.pop(name, ALIGNED))
    assert not kw, kw
    return inp


def call(ctx, cfg, inp=None, batch=BATCH, h=H_AT, h_stride=COL, status=None, null_inputs=False):
    inp = inputs() if inp is None else inp
    return lib().h2r_quotient_columns(ctx, ctypes.byref(cfg) if cfg is not None else None, None if null_inputs else ctypes.byref(inp), batch, h, h_stride,
                                      status, None)


def sets(cfg):
    a, b = ctypes.c_uint32(77), ctypes.c_uint32(77)
    return lib().h2r_quotient_sets(ctypes.byref(cfg), ctypes.byref(a), ctypes.byref(b)), a.value, b.value


@pytest.fixture
def ctx():
    c = host_ctx()
    yield c
    lib().h2r_ctx_destroy(c)


def test_valid_calls_reach_the_host_only_refusal(ctx):
    assert call(ctx, config()) == OK
    assert call(ctx, config(), status=ALIGNED) == OK
    assert call(ctx, config(lookup_mask=0)) == OK
    assert call(ctx, config(lookup_mask=0), inputs(lookup_a_perm=(0, 0, 0), lookup_s_perm=(0, 0, 0), lookup_z=(0, 0, 0))) == OK       # no argument selected: no lookup columns
    assert call(ctx, config(column_src=(0, 1, 2, 3, 4), n_extra=0), inputs(extra=(0, 0, 0))) == OK                                     # no extra column
    assert call(ctx, config(column_src=(3,), chunk_len=7, n_extra=0)) == OK                                                            # m = 1
    assert call(ctx, config(log_ext=K + 1), inputs(col=COL // 2), h_stride=COL // 2) == OK
    assert call(ctx, config(log_n=20, log_ext=24), inputs(col=32 << 24), h_stride=32 << 24, h=ALIGNED + (1 << 50)) == OK
    assert call(ctx, config(), batch=0) == OK                                                       # (batch = 0 is H2R_OK on a device ctx: no launch)
    assert call(ctx, config(), batch=65535, inp=inputs(col=COL, **{g: (None, COL, 65535 * COL) for g in _lib.H2RQuotientInputs.GROUPS[:6]}),
                h=ALIGNED + (1 << 50)) == OK                                                        # [column][circuit]


def test_null_pointers(ctx):
    cfg = config()
    assert call(None, cfg) == _lib.H2R_E_NULL
    assert call(ctx, None) == _lib.H2R_E_NULL
    assert call(ctx, cfg, null_inputs=True) == _lib.H2R_E_NULL
    assert call(ctx, cfg, h=None) == _lib.H2R_E_NULL
    for name in _lib.H2RQuotientInputs.CHALLENGES:
        assert call(ctx, cfg, inputs(**{name: None})) == _lib.H2R_E_NULL, name
    for name in _lib.H2RQuotientInputs.GROUPS:
        assert call(ctx, cfg, inputs(**{name: (0, None, None)})) == _lib.H2R_E_NULL, name
    assert call(ctx, cfg, status=None) == OK                                                        # status is optional
    assert lib().h2r_quotient_sets(None, None, None) == 0


def test_unsupported_causes(ctx):
    size = ctypes.sizeof(_lib.H2RQuotientConfig)
    for cfg in (config(struct_size=size + 8), config(struct_size=0), config(struct_size=size - 1)):
        assert call(ctx, cfg) == _lib.H2R_E_UNSUPPORTED
        assert call(ctx, cfg, h_stride=COL - 16) == _lib.H2R_E_UNSUPPORTED      # not the host-only refusal: it comes before the shape checks
        assert sets(cfg)[0] == 0
    many = inputs(**{g: (None, COL, 65536 * COL) for g in _lib.H2RQuotientInputs.GROUPS[:6]})
    assert call(ctx, config(), many, batch=65536, h=ALIGNED + (1 << 50)) == _lib.H2R_E_UNSUPPORTED   # more than 65,535 circuits (a device ctx refuses it too)


W6 = NR.omega_of(P_FR, EK)
SHAPE_CAUSES = [   # (what, config overrides, input overrides, call overrides)
    ("log_n = 0", dict(log_n=0, log_ext=2, bf=0), dict(col=128), dict(h_stride=128)),
    ("log_ext = log_n", dict(log_ext=K, omega_ext=NR.omega_of(P_FR, K)), dict(col=COL // 4), dict(h_stride=COL // 4)),
    ("log_ext < log_n", dict(log_ext=K - 1, omega_ext=NR.omega_of(P_FR, K - 1)), dict(col=COL // 8), dict(h_stride=COL // 8)),
    ("log_ext > 24", dict(log_n=21, log_ext=25), dict(col=32 << 25), dict(h_stride=32 << 25, h=ALIGNED + (1 << 50))),
    ("log_ext - log_n > 4", dict(log_n=1, log_ext=EK, bf=0), dict(), dict()),
    ("u = 0", dict(bf=15), dict(), dict()),
    ("u < 0", dict(bf=16), dict(), dict()),
    ("blinding_factors wraps", dict(bf=0xFFFFFFFF), dict(), dict()),
    ("num_fixed > 16", dict(num_fixed=17), dict(), dict()),
    ("gate_fixed beyond num_fixed", dict(gate_fixed=(0, 1, 2, 3, 4, 5, 6, 7, 15)), dict(), dict()),
    ("gate_fixed with no fixed column", dict(num_fixed=0, lookup_mask=0), dict(), dict()),
    ("lookup_tag beyond num_fixed", dict(lookup_tag=(11, 11, 15, 11, 13)), dict(), dict()),
    ("lookup_enable beyond num_fixed", dict(lookup_enable=(12, 12, 12, 12, 255)), dict(), dict()),
    ("table_tag beyond num_fixed", dict(table_tag=15), dict(), dict()),
    ("table_value beyond num_fixed", dict(table_value=16), dict(), dict()),
    ("lookup_advice beyond the five columns", dict(lookup_advice=(0, 5, 2, 3, 0)), dict(), dict()),
    ("lookup_mask beyond the five arguments", dict(lookup_mask=32), dict(), dict()),
    ("num_columns = 0", dict(column_src=(), n_extra=0), dict(), dict()),
    ("num_columns > 8", dict(num_columns=9), dict(), dict()),
    ("chunk_len = 0", dict(chunk_len=0), dict(), dict()),
    ("n_extra > 3", dict(n_extra=4), dict(), dict()),
    ("column_src beyond the extra columns", dict(column_src=(0, 1, 2, 3, 4, 6)), dict(), dict()),
    ("column_src repeated", dict(column_src=(0, 1, 2, 3, 3, 5)), dict(), dict()),
    ("omega_ext = p", dict(omega_ext=P_FR), dict(), dict()),
    ("zeta >= p", dict(zeta=P_FR + 5), dict(), dict()),
    ("delta = p", dict(delta=P_FR), dict(), dict()),
    ("zeta = 0", dict(zeta=0), dict(), dict()),
    ("omega_ext = 1", dict(omega_ext=1), dict(), dict()),
    ("omega_ext of order N / 2", dict(omega_ext=NR.omega_of(P_FR, EK - 1)), dict(), dict()),
    ("omega_ext of order 2 N", dict(omega_ext=NR.omega_of(P_FR, EK + 1)), dict(), dict()),
    ("omega_ext not a root of unity", dict(omega_ext=5), dict(), dict()),
    ("zeta^n = 1", dict(zeta=1), dict(), dict()),
    ("zeta^n in the subgroup: zeta = omega_ext", dict(zeta=W6), dict(), dict()),
    ("zeta = omega_ext * omega: the same zeta^n", dict(zeta=W6 * NR.omega_of(P_FR, K) % P_FR), dict(), dict()),
    ("h_out not aligned", dict(), dict(), dict(h=H_AT + 8)),
    ("h_elem_stride not aligned", dict(), dict(), dict(h_stride=COL + 8)),
    ("h_elem_stride smaller than the column", dict(), dict(), dict(h_stride=COL - 16)),
] + [("%s: %s" % (g, what), dict(), {g: over}, dict()) for g in _lib.H2RQuotientInputs.GROUPS for what, over in (
    ("base not aligned", (ALIGNED + (_lib.H2RQuotientInputs.GROUPS.index(g) + 1) * GB + 8, None, None)),
    ("col_stride not aligned", (None, 64 * COL, COL + 8)),
    ("col_stride smaller than the column", (None, 64 * COL, COL - 16)),
)] + [("%s: %s" % (g, what), dict(), {g: over}, dict()) for g in _lib.H2RQuotientInputs.GROUPS[:6] for what, over in (
    ("elem_stride not aligned", (None, 64 * COL + 8, None)),
    ("elem_stride smaller than the column", (None, COL - 16, 2 * COL)),
    ("elem_stride does not cover the columns", (None, GROUP_COLS[g] * COL - 16 if GROUP_COLS[g] > 1 else COL - 16, None)),
    ("[column][circuit] with a column stride that does not cover the batch", (None, COL, 2 * COL - 16)),
) if not (GROUP_COLS[g] == 1 and what.startswith("[column]"))] + [("h_out inside %s" % g, dict(), dict(), dict(h=ALIGNED + (_lib.H2RQuotientInputs.GROUPS.index(g) + 1) * GB + (GROUP_COLS[g] - 1) * COL + COL - 16))
      for g in _lib.H2RQuotientInputs.GROUPS] + [
    ("advice inside h_out", dict(), dict(advice=(H_AT + 2 * COL - 16, None, None)), dict()),
    ("h_out == fixed", dict(), dict(), dict(h=ALIGNED + 7 * GB)),
    ("h_out in a gap between the circuits of perm_z", dict(), dict(perm_z=(None, 8 * COL, None)), dict(h=ALIGNED + 3 * GB + 4 * COL)),
]


@pytest.mark.parametrize("what,cfg_kw,in_kw,call_kw", SHAPE_CAUSES, ids=[c[0] for c in SHAPE_CAUSES])
def test_shape_causes(ctx, what, cfg_kw, in_kw, call_kw):
    assert call(ctx, config(**cfg_kw), inputs(**in_kw), **call_kw) == _lib.H2R_E_SHAPE
    if cfg_kw and not (set(cfg_kw) & {"omega_ext", "zeta", "delta"}) or what.startswith("log_ext"):
        assert sets(config(**cfg_kw))[0] == 0                                                       # what needs no ctx: the host helper refuses it too


def test_valid_twins_of_the_shape_causes(ctx):
    """What lies just inside each bound above comes through the argument checks."""
    assert call(ctx, config(log_n=1, log_ext=2, bf=0), inputs(col=128), h_stride=128) == OK
    assert call(ctx, config(log_n=EK - 4, log_ext=EK, bf=1)) == OK                                  # log_ext - log_n = 4
    assert call(ctx, config(log_n=20, log_ext=24), inputs(col=32 << 24), h_stride=32 << 24, h=ALIGNED + (1 << 50)) == OK
    assert call(ctx, config(bf=14)) == OK                                                           # u = 1
    assert call(ctx, config(bf=0)) == OK
    assert call(ctx, config(num_fixed=16, gate_fixed=(0, 1, 2, 3, 4, 5, 6, 7, 15), table_value=15, lookup_enable=(12, 12, 12, 12, 15)), inputs(fixed=(None, None, None))) == OK
    assert call(ctx, config(num_fixed=9, lookup_mask=0)) == OK                                      # the lookup indices of unselected arguments are not looked at
    assert call(ctx, config(lookup_mask=0, lookup_tag=(99,) * 5, lookup_enable=(99,) * 5, lookup_advice=(9,) * 5, table_tag=99, table_value=99)) == OK
    assert call(ctx, config(lookup_mask=1 << 2, lookup_tag=(99, 99, 3, 99, 99), lookup_enable=(99, 99, 0, 99, 99), lookup_advice=(9, 9, 4, 9, 9))) == OK
    assert call(ctx, config(column_src=(7, 0, 5, 6, 1, 2, 3, 4), n_extra=3, chunk_len=1000), inputs(extra=(None, 3 * COL, None))) == OK  # eight columns, three extra, one set
    assert call(ctx, config(omega_ext=P_FR - W6)) == OK                                             # -omega: also primitive
    assert call(ctx, config(zeta=5, delta=0)) == OK                                                 # delta is only compared with p
    for g in _lib.H2RQuotientInputs.GROUPS[:6]:
        assert call(ctx, config(), inputs(**{g: (None, GROUP_COLS[g] * (COL + 16), COL + 16)})) == OK, g
        assert call(ctx, config(), inputs(**{g: (None, COL, 2 * COL)})) == OK, g                    # [column][circuit]
        assert call(ctx, config(), inputs(**{g: (None, COL + 16, 2 * COL + 16)})) == OK, g
    for g in _lib.H2RQuotientInputs.GROUPS[6:]:
        assert call(ctx, config(), inputs(**{g: (None, 8, COL + 16)})) == OK, g                     # a key group's elem_stride is ignored
    for g in _lib.H2RQuotientInputs.GROUPS:                                                         # h begins where a group ends, and ends where it begins
        at = ALIGNED + (_lib.H2RQuotientInputs.GROUPS.index(g) + 1) * GB
        assert call(ctx, config(), h=at + BATCH * GROUP_COLS[g] * COL) == OK, g
        assert call(ctx, config(), h=at - BATCH * COL) == OK, g
    assert call(ctx, config(), h=ALIGNED + 7 * GB, batch=0) == OK                                   # no circuits: nothing overlaps
    assert call(ctx, config(), h_stride=COL + 16) == OK


def test_zeta_minus_one_is_in_the_subgroup(ctx):
    assert call(ctx, config(zeta=P_FR - 1)) == _lib.H2R_E_SHAPE                                     # (-1)^n = 1 for n >= 2


@pytest.mark.parametrize("flags", [0, _lib.H2R_ADVICE_MONTGOMERY], ids=["canonical", "montgomery"])
def test_the_constants_are_in_the_ctx_representation(flags):
    c = host_ctx(flags=flags)
    conv = (lambda v: v * R256 % P_FR) if flags else (lambda v: v)
    other = (lambda v: v) if flags else (lambda v: v * R256 % P_FR)
    z = NR.cube_root_of_unity(P_FR)
    assert call(c, config(omega_ext=conv(W6), zeta=conv(z), delta=conv(7))) == OK
    assert call(c, config(omega_ext=other(W6), zeta=conv(z), delta=conv(7))) == _lib.H2R_E_SHAPE    # the same root in the other representation is no root here
    assert call(c, config(omega_ext=conv(W6), zeta=conv(1), delta=conv(7))) == _lib.H2R_E_SHAPE     # zeta = 1 in this representation
    lib().h2r_ctx_destroy(c)


def test_fields():
    for field in NR.FIELDS_WITH_DOMAINS:
        c = host_ctx(field)
        assert call(c, config(field)) == OK, field
        assert call(c, config(field, omega_ext=NR.omega_of(FIELD_MODULI[field], EK - 1))) == _lib.H2R_E_SHAPE, field
        lib().h2r_ctx_destroy(c)
    c = host_ctx("bn254_fq")                                                                        # p - 1 = 2 * odd: no domain of four points
    pq = FIELD_MODULI["bn254_fq"]
    for w in (pq - 1, 1, 2, pow(3, (pq - 1) // 2, pq)):
        assert call(c, config("bn254_fq", log_n=1, log_ext=2, bf=0, omega_ext=w, zeta=3, delta=5), inputs(col=128), h_stride=128) == _lib.H2R_E_SHAPE, w
    lib().h2r_ctx_destroy(c)


def test_sets_and_column_counts():
    assert sets(config()) == (3, 5 + 1 + 3 + 15, 15 + 6 + 3)                                        # every fixed column is used
    assert sets(config(chunk_len=1)) == (6, 5 + 1 + 6 + 15, 24)
    assert sets(config(chunk_len=3, lookup_mask=0)) == (2, 5 + 1 + 2, 9 + 6 + 3)
    assert sets(config(chunk_len=9, lookup_mask=1 << 4)) == (1, 5 + 1 + 1 + 3, 9 + 4 + 6 + 3)
    assert sets(config(column_src=(2,), n_extra=0, lookup_mask=0, gate_fixed=(0,) * 9)) == (1, 5 + 1, 1 + 1 + 3)
    assert sets(config(omega_ext=1, zeta=0, delta=P_FR))[0] == 3                                    # compared with the ctx's p by the call: the helper has no ctx
    assert sets(config(chunk_len=0)) == (0, 77, 77)                                                 # refused: the counts are left alone
