"""Host-side checks of the permutation argument's grand-product exports (h2r_permutation_sets, h2r_permutation_product_workspace_bytes,
h2r_permutation_product_columns): argument checking only, no device work.  A host-only ctx is refused with H2R_E_UNSUPPORTED only after
its arguments were found well-formed, so every H2R_E_NULL and H2R_E_SHAPE cause shows without a device."""
import ctypes

import pytest

from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib

P_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
U = 1018
COL = (U + 1) * 32


def host_ctx(w=64, L=4, flags=0, col_stride=0):
    ctx = ctypes.c_void_p()
    p = H2RParams(w, w * L, 0, -1)
    rp = _lib.H2RAdviceRepr(ctypes.sizeof(_lib.H2RAdviceRepr), flags, col_stride)
    assert lib().h2r_ctx_create_ex(ctypes.byref(p), ctypes.byref(rp), ctypes.byref(ctx)) == 0
    return ctx


def fe(v):
    return (ctypes.c_uint64 * 4)(*[(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)])


def config(src=(0, 1, 2, 3, 4, 5), chunk=2, delta=7, omega=5, n_extra=None):
    cfg = _lib.H2RPermutationConfig()
    cfg.struct_size = ctypes.sizeof(cfg)
    cfg.num_columns, cfg.chunk_len = len(src), chunk
    cfg.n_extra = max([s - 4 for s in src if s >= 5] + [0]) if n_extra is None else n_extra
    for c, s in enumerate(src[:8]):
        cfg.column_src[c] = s
    cfg.delta, cfg.omega = fe(delta), fe(omega)
    return cfg


BUF = (ctypes.c_uint64 * 64)()          # ctypes aligns the array to 8 bytes only: the calls below take a 16-byte aligned address inside it
ALIGNED = (ctypes.addressof(BUF) + 15) & ~15


def call(ctx, cfg, **kw):
    """The export with well-formed arguments (never dereferenced: no device work happens on a host-only ctx), overridden by name."""
    a = dict(image=ALIGNED, image_stride=8 * 160, rows=8, first_row=0, batch=2, extra=ALIGNED, extra_elem_stride=U * 32, extra_col_stride=U * 32,
             sigma=ALIGNED, sigma_col_stride=U * 32, beta=ALIGNED, gamma=ALIGNED, usable=U, z=ALIGNED, z_elem_stride=3 * COL, z_col_stride=COL,
             status=None, ws=ALIGNED)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return lib().h2r_permutation_product_columns(ctx, ctypes.byref(cfg) if cfg is not None else None, a["image"], a["image_stride"], a["rows"],
                                                 a["first_row"], a["batch"], a["extra"], a["extra_elem_stride"], a["extra_col_stride"], a["sigma"],
                                                 a["sigma_col_stride"], a["beta"], a["gamma"], a["usable"], a["z"], a["z_elem_stride"],
                                                 a["z_col_stride"], a["status"], a["ws"], None)


@pytest.fixture
def ctx():
    c = host_ctx()
    yield c
    lib().h2r_ctx_destroy(c)


def test_host_only_ctx_refuses_device_work(ctx):
    assert call(ctx, config()) == _lib.H2R_E_UNSUPPORTED
    assert call(ctx, config(src=(0, 1, 2, 3, 4), chunk=2), extra=None) == _lib.H2R_E_UNSUPPORTED      # no extra column: extra may be NULL
    assert call(ctx, config(), batch=65536, z_elem_stride=3 * COL) == _lib.H2R_E_UNSUPPORTED
    cfg = config()
    cfg.struct_size += 8
    assert call(ctx, cfg) == _lib.H2R_E_UNSUPPORTED and lib().h2r_permutation_sets(ctypes.byref(cfg)) == 0


def test_null_pointers(ctx):
    cfg = config()
    assert call(None, cfg) == _lib.H2R_E_NULL
    assert call(ctx, None) == _lib.H2R_E_NULL
    for hole in ("image", "extra", "sigma", "beta", "gamma", "z", "ws"):
        assert call(ctx, cfg, **{hole: None}) == _lib.H2R_E_NULL, hole
    assert call(ctx, cfg, status=None) == _lib.H2R_E_UNSUPPORTED                                       # status is optional


SHAPE_CAUSES = [
    ("usable_rows = 0", dict(), dict(usable=0, rows=0)),
    ("usable_rows > 2^28", dict(), dict(usable=(1 << 28) + 1, sigma_col_stride=1 << 34, z_col_stride=1 << 34, z_elem_stride=1 << 36)),
    ("first_row + rows > usable_rows", dict(), dict(first_row=U - 7)),
    ("m = 0", dict(src=()), dict()),
    ("m > 8", dict(src=(0, 1, 2, 3, 4, 5, 6, 7, 0)), dict()),
    ("chunk_len = 0", dict(chunk=0), dict()),
    ("column_src out of range", dict(src=(0, 1, 6), n_extra=1), dict()),
    ("column_src beyond n_extra", dict(src=(0, 1, 5), n_extra=0), dict()),
    ("n_extra > 3", dict(src=(0, 8)), dict()),
    ("column_src repeated", dict(src=(0, 1, 2, 1)), dict()),
    ("extra column repeated", dict(src=(0, 5, 5)), dict()),
    ("delta = p", dict(delta=P_FR), dict()),
    ("omega >= p", dict(omega=P_FR + 1), dict()),
    ("image not aligned", dict(), dict(image=ALIGNED + 8)),
    ("image_stride not aligned", dict(), dict(image_stride=8 * 160 + 8)),
    ("extra not aligned", dict(), dict(extra=ALIGNED + 8)),
    ("extra_elem_stride not aligned", dict(), dict(extra_elem_stride=U * 32 + 8)),
    ("extra_col_stride not aligned", dict(), dict(extra_col_stride=U * 32 + 4)),
    ("sigma not aligned", dict(), dict(sigma=ALIGNED + 4)),
    ("sigma_col_stride not aligned", dict(), dict(sigma_col_stride=U * 32 + 8)),
    ("sigma_col_stride < u * 32", dict(), dict(sigma_col_stride=U * 32 - 32)),
    ("z not aligned", dict(), dict(z=ALIGNED + 8)),
    ("z_elem_stride not aligned", dict(), dict(z_elem_stride=3 * COL + 8)),
    ("z_col_stride too small", dict(), dict(z_col_stride=COL - 32)),
    ("z_col_stride not a multiple of 32", dict(), dict(z_col_stride=COL + 16, z_elem_stride=3 * (COL + 16))),
    ("z_elem_stride does not cover S columns", dict(), dict(z_elem_stride=2 * COL)),
    ("[set][element] with a column stride that does not cover the batch", dict(), dict(z_elem_stride=COL, z_col_stride=COL + 32)),
    ("image stride below the rows", dict(), dict(image_stride=7 * 160)),
]


@pytest.mark.parametrize("what,cfg_kw,call_kw", SHAPE_CAUSES, ids=[c[0] for c in SHAPE_CAUSES])
def test_shape_causes(ctx, what, cfg_kw, call_kw):
    assert call(ctx, config(**cfg_kw), **call_kw) == _lib.H2R_E_SHAPE


def test_accepted_arrangements(ctx):
    """What lies just inside the bounds above comes through the argument checks (and then meets the host-only ctx)."""
    ok = _lib.H2R_E_UNSUPPORTED
    assert call(ctx, config(), first_row=U - 8) == ok
    assert call(ctx, config(), z_elem_stride=COL, z_col_stride=2 * COL) == ok                 # [set][element]
    assert call(ctx, config(), z_col_stride=1 << 15, z_elem_stride=3 << 15) == ok             # 2^k * 32 per column
    assert call(ctx, config(delta=P_FR - 1, omega=P_FR - 1)) == ok
    assert call(ctx, config(src=(7, 0, 6, 5, 4, 3, 2, 1), chunk=9)) == ok
    assert call(ctx, config(), usable=1 << 28, sigma_col_stride=1 << 33, z_col_stride=1 << 34, z_elem_stride=1 << 36) == ok
    planar = host_ctx(flags=_lib.H2R_ADVICE_COLUMNS, col_stride=1 << 15)
    assert call(planar, config(), image_stride=5 << 15) == ok
    assert call(planar, config(), image_stride=4 << 15) == _lib.H2R_E_SHAPE                   # the element stride does not cover five columns
    lib().h2r_ctx_destroy(planar)


def test_no_elements_leaves_the_z_layout_unseen(ctx):
    """batch = 0: Z's strides need not hold a column apart from each other (only z_col_stride's own bounds apply), and the call goes on
    to meet the host-only ctx.  The shared column-block test would refuse these strides: the export asks it only when there are elements."""
    ok = _lib.H2R_E_UNSUPPORTED
    assert call(ctx, config(), batch=0, z_elem_stride=0) == ok
    assert call(ctx, config(), batch=0, z_elem_stride=COL - 32) == ok
    assert call(ctx, config(), batch=0, z_elem_stride=2 * COL) == ok                          # (refused with elements: SHAPE_CAUSES)
    assert call(ctx, config(), batch=0, z_elem_stride=0, z_col_stride=COL - 32) == _lib.H2R_E_SHAPE
    assert call(ctx, config(), batch=0, z_elem_stride=0, z_col_stride=COL + 16) == _lib.H2R_E_SHAPE
    assert call(ctx, config(), batch=1, z_elem_stride=0) == _lib.H2R_E_SHAPE                  # one element: the strides count


def test_huge_z_strides_are_judged_without_wrapping(ctx):
    """Three sets at strides of 2^63: two elements' columns collide (element 1's set 0 IS element 0's set 1), but 2 * 2^63 + column is
    `column` in 64 bits, which an element stride of 2^63 covers.  The layout test is 128-bit now and refuses what the 64-bit one let
    through to the host-only ctx's H2R_E_UNSUPPORTED."""
    three = config(src=(0, 1, 2), chunk=1)
    assert call(ctx, three, z_elem_stride=1 << 63, z_col_stride=1 << 63) == _lib.H2R_E_SHAPE
    assert call(ctx, three, batch=1, z_elem_stride=1 << 63, z_col_stride=1 << 63) == _lib.H2R_E_UNSUPPORTED   # one element: [set][element] holds
    assert call(ctx, three, z_elem_stride=COL, z_col_stride=1 << 63) == _lib.H2R_E_UNSUPPORTED                 # [set][element], truly


def test_sets():
    sets = lib().h2r_permutation_sets
    for (m, chunk), want in {(5, 2): 3, (6, 2): 3, (6, 6): 1, (6, 7): 1, (3, 1): 3, (8, 3): 3, (1, 1): 1}.items():
        assert sets(ctypes.byref(config(src=tuple(range(m)), chunk=chunk))) == want, (m, chunk)
    assert sets(None) == 0
    assert sets(ctypes.byref(config(chunk=0))) == 0 and sets(ctypes.byref(config(src=()))) == 0
    assert sets(ctypes.byref(config(src=(0, 0)))) == 0 and sets(ctypes.byref(config(src=(0, 9)))) == 0


def test_workspace_bytes():
    ws = lib().h2r_permutation_product_workspace_bytes
    cfg = ctypes.byref(config())
    assert ws(cfg, 131066, 0) == 0 and ws(cfg, 0, 0) == 0 and ws(None, 131066, 4) == 0
    assert ws(ctypes.byref(config(chunk=0)), 131066, 4) == 0
    rows = [1, 1018, 1024, 1025, 4090, 131066, (1 << 20) - 6]
    elems = [1, 2, 3, 256, 65535]
    for u in rows:
        sizes = [ws(cfg, u, e) for e in elems]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and sizes[0] > 0, u
    for e in elems:
        sizes = [ws(cfg, u, e) for u in rows]
        assert sizes == sorted(sizes), e
    assert ws(ctypes.byref(config(chunk=1)), 131066, 256) > ws(cfg, 131066, 256) > ws(ctypes.byref(config(chunk=6)), 131066, 256)
    assert ws(ctypes.byref(config(chunk=1)), 131066, 256) < 16 << 20      # two products per tile of a set
