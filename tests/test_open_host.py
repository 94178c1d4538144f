"""Host-side checks of the openings' exports (h2r_open_queries, h2r_open_workspace_bytes, h2r_open_eval_columns, h2r_open_witness_columns,
h2r_fold_columns): argument checking only, no device work.  A host-only ctx is refused with H2R_E_UNSUPPORTED only after its arguments were
found well-formed, so every H2R_E_NULL, H2R_E_SHAPE and H2R_E_UNSUPPORTED cause shows without a device, each next to a valid twin that
differs in that one field and reaches the host-only refusal."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from halo2_rsa_amd import _lib
from halo2_rsa_amd._lib import H2RParams, lib

N = 1000                                # coefficients: no power of two, no multiple of the tile
COL = N * 32
OK = _lib.H2R_E_UNSUPPORTED             # what a well-formed call meets on a host-only ctx
BUF = (ctypes.c_uint64 * 64)()          # ctypes aligns the array to 8 bytes only: the calls below take a 16-byte aligned address inside it
ALIGNED = (ctypes.addressof(BUF) + 15) & ~15
GB = 1 << 30                            # the columns lie a gigabyte apart: never dereferenced, no device work happens on a host-only ctx
BATCH = 3
MASKS = (0b0011, 0b0001, 0b1011, 0b0010, 0b0001)         # point 2 of four has no column
W_AT = ALIGNED + 100 * GB            # behind every column, 64 of them included
WS_BYTES = 256 + BATCH * (64 + 32 * 8 * 1)               # h2r_open_workspace_bytes of the default call: 8 queries, one tile


@pytest.fixture
def ctx():
    c = ctypes.c_void_p()
    p = H2RParams(64, 256, 0, -1)
    assert lib().h2r_ctx_create(ctypes.byref(p), ctypes.byref(c)) == 0
    yield c
    lib().h2r_ctx_destroy(c)


def config(n=N, num_cols=len(MASKS), num_points=4, struct_size=None):
    cfg = _lib.H2ROpenConfig()
    cfg.struct_size = ctypes.sizeof(cfg) if struct_size is None else struct_size
    cfg.n_coeffs, cfg.num_cols, cfg.num_points = n, num_cols, num_points
    return cfg


def columns(masks=MASKS, col=COL, **over):
    """Well-formed descriptors: column c per circuit at its own gigabyte, the last one a key column (elem_stride 0); `over` = {index: (base,
    elem_stride, mask, reserved)} with None = as it was."""
    desc = (_lib.H2ROpenColumn * max(len(masks), 1))()
    for c, m in enumerate(masks):
        desc[c].base, desc[c].elem_stride, desc[c].point_mask = ALIGNED + (c + 1) * GB, 0 if c == len(masks) - 1 else col, m
    for c, fields in over.items():
        for name, v in zip(("base", "elem_stride", "point_mask", "reserved"), fields):
            if v is not None:
                setattr(desc[int(c)], name, None if name == "base" and v == 0 else v)
    return desc


def ev(ctx, cfg=None, cols=None, points=ALIGNED, batch=BATCH, evals=ALIGNED, status=None, ws=ALIGNED):
    cfg = config() if cfg is None else cfg
    return lib().h2r_open_eval_columns(ctx, ctypes.byref(cfg) if cfg else None, columns() if cols is None else cols, points, batch, evals, status, ws, None)


def wit(ctx, cfg=None, cols=None, points=ALIGNED, v=ALIGNED, batch=BATCH, w=W_AT, w_es=4 * COL, w_ps=COL, be=ALIGNED, status=None, ws=ALIGNED, col=COL):
    cfg = config() if cfg is None else cfg
    return lib().h2r_open_witness_columns(ctx, ctypes.byref(cfg) if cfg else None, columns() if cols is None else cols, points, v, batch, w, w_es, w_ps,
                                          be, status, ws, None)


def fold(ctx, inp=ALIGNED + GB, in_es=4 * COL, in_cs=COL, num_cols=4, n=N, s=ALIGNED, batch=BATCH, out=W_AT, out_es=COL, status=None):
    return lib().h2r_fold_columns(ctx, inp, in_es, in_cs, num_cols, n, s, batch, out, out_es, status, None)


def both(ctx, want, **kw):
    assert ev(ctx, **kw) == want and wit(ctx, **kw) == want


def test_valid_calls_reach_the_host_only_refusal(ctx):
    both(ctx, OK)
    both(ctx, OK, status=ALIGNED)
    both(ctx, OK, batch=0)                                              # (batch = 0 is H2R_OK on a device ctx: no launch)
    both(ctx, OK, batch=65535, cols=columns(col=COL), cfg=config())
    assert wit(ctx, be=None) == OK                                      # batch_evals is optional
    both(ctx, OK, cfg=config(n=1), cols=columns(col=32))
    assert ev(ctx, cfg=config(n=1 << 24), cols=columns(col=32 << 24)) == OK
    assert wit(ctx, cfg=config(n=1 << 24), cols=columns(col=32 << 24), w=ALIGNED + (1 << 50), w_es=4 * (32 << 24), w_ps=32 << 24) == OK
    both(ctx, OK, cfg=config(num_cols=1, num_points=1), cols=columns(masks=(1,)))
    both(ctx, OK, cfg=config(num_cols=64), cols=columns(masks=(0b1111,) * 64))
    assert wit(ctx, w_es=COL, w_ps=BATCH * COL) == OK                   # [point][circuit]
    assert wit(ctx, w_es=4 * (COL + 16), w_ps=COL + 16) == OK
    assert fold(ctx) == OK and fold(ctx, status=ALIGNED) == OK and fold(ctx, batch=0) == OK
    assert fold(ctx, num_cols=1) == OK and fold(ctx, num_cols=64, in_es=64 * COL) == OK
    assert fold(ctx, in_es=COL, in_cs=BATCH * COL) == OK                # [column][circuit]
    assert fold(ctx, n=1 << 24, in_es=4 * (32 << 24), in_cs=32 << 24, out=ALIGNED + (1 << 50), out_es=32 << 24) == OK


def test_null_pointers(ctx):
    for kw in (dict(points=None), dict(ws=None)):
        both(ctx, _lib.H2R_E_NULL, **kw)
    both(ctx, _lib.H2R_E_NULL, cols=columns(**{"2": (0, None, None, None)}))
    assert ev(ctx, evals=None) == _lib.H2R_E_NULL
    assert wit(ctx, v=None) == _lib.H2R_E_NULL and wit(ctx, w=None) == _lib.H2R_E_NULL
    cfg, cols = config(), columns()
    assert lib().h2r_open_eval_columns(None, ctypes.byref(cfg), cols, ALIGNED, BATCH, ALIGNED, None, ALIGNED, None) == _lib.H2R_E_NULL
    assert lib().h2r_open_eval_columns(ctx, None, cols, ALIGNED, BATCH, ALIGNED, None, ALIGNED, None) == _lib.H2R_E_NULL
    assert lib().h2r_open_eval_columns(ctx, ctypes.byref(cfg), None, ALIGNED, BATCH, ALIGNED, None, ALIGNED, None) == _lib.H2R_E_NULL
    assert lib().h2r_open_witness_columns(None, ctypes.byref(cfg), cols, ALIGNED, ALIGNED, BATCH, W_AT, 4 * COL, COL, None, None, ALIGNED, None) == _lib.H2R_E_NULL
    assert lib().h2r_open_witness_columns(ctx, None, cols, ALIGNED, ALIGNED, BATCH, W_AT, 4 * COL, COL, None, None, ALIGNED, None) == _lib.H2R_E_NULL
    assert lib().h2r_open_witness_columns(ctx, ctypes.byref(cfg), None, ALIGNED, ALIGNED, BATCH, W_AT, 4 * COL, COL, None, None, ALIGNED, None) == _lib.H2R_E_NULL
    assert fold(ctx, inp=None) == _lib.H2R_E_NULL and fold(ctx, s=None) == _lib.H2R_E_NULL and fold(ctx, out=None) == _lib.H2R_E_NULL
    assert lib().h2r_fold_columns(None, ALIGNED + GB, 4 * COL, COL, 4, N, ALIGNED, BATCH, W_AT, COL, None, None) == _lib.H2R_E_NULL
    assert lib().h2r_open_queries(None, cols, None) == 0 and lib().h2r_open_queries(ctypes.byref(cfg), None, None) == 0
    assert lib().h2r_open_workspace_bytes(None, cols, 1) == 0 and lib().h2r_open_workspace_bytes(ctypes.byref(cfg), None, 1) == 0


def test_unsupported_causes(ctx):
    size = ctypes.sizeof(_lib.H2ROpenConfig)
    assert size == 16 and ctypes.sizeof(_lib.H2ROpenColumn) == 24
    for bad in (size + 8, 0, size - 1):
        cfg = config(struct_size=bad)
        both(ctx, _lib.H2R_E_UNSUPPORTED, cfg=cfg)
        both(ctx, _lib.H2R_E_UNSUPPORTED, cfg=cfg, cols=columns(**{"0": (None, None, 0, None)}))   # not the host-only refusal: it comes before the shape checks
        assert lib().h2r_open_queries(ctypes.byref(cfg), columns(), None) == 0
    both(ctx, _lib.H2R_E_UNSUPPORTED, batch=65536)                      # more than 65,535 circuits (a device ctx refuses it too)
    assert wit(ctx, batch=65536, w=ALIGNED + (1 << 50)) == _lib.H2R_E_UNSUPPORTED
    assert fold(ctx, batch=65536, out=ALIGNED + (1 << 50)) == _lib.H2R_E_UNSUPPORTED
    assert lib().h2r_open_workspace_bytes(ctypes.byref(config()), columns(), 65536) == 0


SHAPE_CAUSES = [   # (what, config overrides, columns overrides (masks / col / per-column), witness-call overrides or None when both calls refuse)
    ("n_coeffs = 0", dict(n=0), dict(), None),
    ("n_coeffs > 2^24", dict(n=(1 << 24) + 1), dict(col=32 * ((1 << 24) + 1)), None),
    ("num_cols = 0", dict(num_cols=0), dict(), None),
    ("num_cols > 64", dict(num_cols=65), dict(masks=(1,) * 65), None),
    ("num_points = 0", dict(num_points=0), dict(), None),
    ("num_points > 4", dict(num_points=5), dict(), None),
    ("a mask of 0", dict(), {"1": (None, None, 0, None)}, None),
    ("a mask with a bit beyond num_points", dict(num_points=3), dict(masks=(0b0011, 0b0001, 0b1011, 0b0010, 0b0001)), None),
    ("a mask with bit 31", dict(), {"0": (None, None, 0x80000001, None)}, None),
    ("reserved != 0", dict(), {"3": (None, None, None, 1)}, None),
    ("a base that is not aligned", dict(), {"0": (ALIGNED + GB + 8, None, None, None)}, None),
    ("an elem_stride that is not aligned", dict(), {"0": (None, COL + 8, None, None)}, None),
    ("an elem_stride smaller than the column", dict(), {"1": (None, COL - 16, None, None)}, None),
]
WITNESS_SHAPE_CAUSES = [
    ("w_out not aligned", dict(w=W_AT + 8)),
    ("w_elem_stride not aligned", dict(w_es=4 * COL + 8)),
    ("w_point_stride not aligned", dict(w_ps=COL + 8, w_es=8 * COL)),
    ("w_point_stride smaller than the column", dict(w_ps=COL - 16)),
    ("w_elem_stride smaller than the column", dict(w_es=COL - 16, w_ps=BATCH * COL)),
    ("w_elem_stride does not cover the points", dict(w_es=4 * COL - 16)),
    ("[point][circuit] with a point stride that does not cover the batch", dict(w_es=COL, w_ps=BATCH * COL - 16)),
    ("W begins inside column 0", dict(w=ALIGNED + GB + BATCH * COL - 16)),
    ("W ends inside column 2", dict(w=ALIGNED + 3 * GB - BATCH * 4 * COL + 16)),
    ("W == the key column", dict(w=ALIGNED + 5 * GB)),
    ("W inside the key column's one copy", dict(w=ALIGNED + 5 * GB + COL - 16)),
    # the small inputs and the workspace: points [batch][4][4] uint64, v [batch][4], batch_evals [batch][4][4]
    ("W == the points", dict(points=W_AT)),
    ("the points end inside W", dict(points=W_AT - BATCH * 128 + 16)),
    ("v inside W", dict(v=W_AT + COL)),
    ("W ends inside v", dict(v=W_AT + BATCH * 4 * COL - 16)),
    ("batch_evals inside W", dict(be=W_AT + 2 * COL + 16)),
    ("the workspace begins inside W", dict(ws=W_AT + BATCH * 4 * COL - 16)),
    ("the workspace ends inside W", dict(ws=W_AT - WS_BYTES + 16)),
]


@pytest.mark.parametrize("what,cfg_kw,col_kw,_", SHAPE_CAUSES, ids=[c[0] for c in SHAPE_CAUSES])
def test_shape_causes(ctx, what, cfg_kw, col_kw, _):
    cfg, cols = config(**cfg_kw), columns(**col_kw)
    both(ctx, _lib.H2R_E_SHAPE, cfg=cfg, cols=cols)
    if not any(w in what for w in ("base", "elem_stride")):             # what needs no pointer: the host helpers refuse it too
        assert lib().h2r_open_queries(ctypes.byref(cfg), cols, None) == 0
        assert lib().h2r_open_workspace_bytes(ctypes.byref(cfg), cols, BATCH) == 0


@pytest.mark.parametrize("what,kw", WITNESS_SHAPE_CAUSES, ids=[c[0] for c in WITNESS_SHAPE_CAUSES])
def test_witness_shape_causes(ctx, what, kw):
    assert wit(ctx, **kw) == _lib.H2R_E_SHAPE


def test_valid_twins_of_the_shape_causes(ctx):
    """What lies just inside each bound above comes through the argument checks."""
    both(ctx, OK, cfg=config(num_points=4), cols=columns(masks=(0b1111, 0b1000, 0b0100, 0b0010, 0b0001)))
    both(ctx, OK, cfg=config(num_points=3), cols=columns(masks=(0b0011, 0b0001, 0b0111, 0b0010, 0b0100)))
    both(ctx, OK, cols=columns(**{"0": (None, COL + 16, None, None)}))
    both(ctx, OK, cols=columns(**{"0": (None, 0, None, None)}))          # any column may be a key column
    both(ctx, OK, cols=columns(**{"1": (ALIGNED + GB, None, None, None)}))   # two descriptors may name one column (inputs may overlap each other)
    assert wit(ctx, w=ALIGNED + GB + BATCH * COL) == OK                 # W begins where column 0 ends
    assert wit(ctx, w=ALIGNED + 3 * GB - BATCH * 4 * COL) == OK         # ... and ends where column 2 begins
    assert wit(ctx, w=ALIGNED + 5 * GB + COL) == OK                     # behind the key column's one copy
    assert wit(ctx, w=ALIGNED + GB, batch=0) == OK                      # no circuits: nothing overlaps
    assert wit(ctx, points=W_AT - BATCH * 128) == OK and wit(ctx, points=W_AT + BATCH * 4 * COL) == OK      # the small inputs end where W begins, begin where it ends
    assert wit(ctx, v=W_AT - BATCH * 32) == OK and wit(ctx, v=W_AT + BATCH * 4 * COL) == OK
    assert wit(ctx, be=W_AT - BATCH * 128) == OK and wit(ctx, be=W_AT + BATCH * 4 * COL) == OK
    assert wit(ctx, ws=W_AT - WS_BYTES) == OK and wit(ctx, ws=W_AT + BATCH * 4 * COL) == OK
    assert ev(ctx, points=ALIGNED, evals=ALIGNED, ws=ALIGNED) == OK     # the evaluations write no column: nothing of theirs is compared


FOLD_SHAPE_CAUSES = [
    ("n_coeffs = 0", dict(n=0)),
    ("n_coeffs > 2^24", dict(n=(1 << 24) + 1, in_es=1 << 40, in_cs=1 << 32, out=ALIGNED + (1 << 50), out_es=1 << 32)),
    ("num_cols = 0", dict(num_cols=0)),
    ("num_cols > 64", dict(num_cols=65, in_es=65 * COL)),
    ("in not aligned", dict(inp=ALIGNED + GB + 8)),
    ("in_elem_stride not aligned", dict(in_es=4 * COL + 8)),
    ("in_col_stride not aligned", dict(in_cs=COL + 8, in_es=8 * COL)),
    ("out not aligned", dict(out=W_AT + 8)),
    ("out_elem_stride not aligned", dict(out_es=COL + 8)),
    ("in_col_stride smaller than the column", dict(in_cs=COL - 16)),
    ("in_elem_stride does not cover the columns", dict(in_es=4 * COL - 16)),
    ("out_elem_stride smaller than the column", dict(out_es=COL - 16)),
    ("out inside the input", dict(out=ALIGNED + GB + BATCH * 4 * COL - 16)),
    ("out == in", dict(out=ALIGNED + GB)),
    ("the input begins inside out", dict(out=ALIGNED + GB - BATCH * COL + 16)),
]


@pytest.mark.parametrize("what,kw", FOLD_SHAPE_CAUSES, ids=[c[0] for c in FOLD_SHAPE_CAUSES])
def test_fold_shape_causes(ctx, what, kw):
    assert fold(ctx, **kw) == _lib.H2R_E_SHAPE


def test_fold_valid_twins(ctx):
    assert fold(ctx, out=ALIGNED + GB + BATCH * 4 * COL) == OK           # out begins where the input ends
    assert fold(ctx, out=ALIGNED + GB - BATCH * COL) == OK               # ... and ends where it begins
    assert fold(ctx, in_es=4 * (COL + 16), in_cs=COL + 16, out_es=COL + 16) == OK
    assert fold(ctx, out=ALIGNED + GB, batch=0) == OK


def test_queries_and_workspace_bytes():
    def q(masks, num_points):
        cfg, pp = config(num_cols=len(masks), num_points=num_points), (ctypes.c_uint32 * 4)(77, 77, 77, 77)
        return lib().h2r_open_queries(ctypes.byref(cfg), columns(masks=masks), pp), list(pp)

    assert q(MASKS, 4) == (8, [4, 3, 0, 1])
    assert q((1,), 1) == (1, [1, 0, 0, 0])
    assert q((0b1111,) * 64, 4) == (256, [64, 64, 64, 64])
    assert q((0b10, 0b10), 2) == (2, [0, 2, 0, 0])
    assert q((0b10, 0b100), 2) == (0, [77, 77, 77, 77])                  # refused: the counts are left alone
    cfg = config()
    assert lib().h2r_open_queries(ctypes.byref(cfg), columns(), None) == 8   # per_point is optional

    def ws(n, masks, num_points, batch):
        cfg = config(n=n, num_cols=len(masks), num_points=num_points)
        return lib().h2r_open_workspace_bytes(ctypes.byref(cfg), columns(masks=masks), batch)

    # 256 bytes of alignment slack, then per circuit a 64-byte header and 32 bytes per (slot, tile of 1,024 coefficients); slots = the larger
    # of Q (the evaluations') and num_points (the witness's), so that one size serves either call
    assert ws(N, MASKS, 4, BATCH) == 256 + BATCH * (64 + 32 * 8 * 1) == WS_BYTES
    assert ws(1025, MASKS, 4, 1) == 256 + (64 + 32 * 8 * 2)
    assert ws(1 << 17, (1,), 4, 2) == 256 + 2 * (64 + 32 * 4 * 128)
    assert ws(1 << 24, (0b1111,) * 64, 4, 65535) == 256 + 65535 * (64 + 32 * 256 * (1 << 14))
    assert ws(N, MASKS, 4, 0) == 256
