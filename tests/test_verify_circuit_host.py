"""CPU: the closed verify_pkcs1v15_signature circuit -- row counts, row kinds and the copy map (host-only exports) -- against the reference's
circuit sizes (tests/test_reference_circuit_sizes.py) and the plain walk of tests/circuit_copy_ref.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circuit_copy_ref as CR  # noqa: E402
import test_reference_circuit_sizes as sizes  # noqa: E402
from halo2_rsa_amd import _lib  # noqa: E402
from halo2_rsa_amd._lib import lib  # noqa: E402

ROW_RANGE_LIMB, ROW_ASSERT_ONE = 32, 17            # include/h2r.h H2R_ROW_*
COPY_SRC = {0xFFFFFF01: "A", 0xFFFFFF02: "B", 0xFFFFFF03: "N"}
OP_IS_IN_FIELD, ASSERT_ONE = sizes.OPS["IS_IN_FIELD"], sizes.ASSERT_ONE


def e_bytes(e):
    return e.to_bytes((e.bit_length() + 7) // 8, "little")


def fixed_layout(ctx, e):
    vl, eb = _lib.H2RVerifyLayout(), e_bytes(e)
    assert lib().h2r_verify_layout_fixed(ctx, eb, len(eb), ctypes.byref(vl)) == 0
    return vl


def pairs_of(call):
    """the two-call protocol of the copy-map exports: cap = 0 asks for the count"""
    n = int(call(None, 0))
    assert n > 0
    buf = (_lib.H2RCopy * n)()
    assert int(call(buf, n)) == n
    short = (_lib.H2RCopy * 3)()
    assert int(call(short, 3)) == n                # a short buffer is filled up to cap, the count is still the whole map's
    assert [(c.row, c.col, c.src_row, c.src_col) for c in short] == [(c.row, c.col, c.src_row, c.src_col) for c in buf[:3]]
    return [(c.row, c.col, c.src_row, c.src_col) for c in buf]


def circuit(ctx, e):
    L = lib()
    vl, eb = fixed_layout(ctx, e), e_bytes(e)
    sec = (ctypes.c_uint64 * 3)()
    rows = int(L.h2r_verify_circuit_rows(ctx, ctypes.byref(vl), sec))
    pairs = pairs_of(lambda out, cap: L.h2r_verify_circuit_copy_map(ctx, ctypes.byref(vl), eb, len(eb), out, cap))
    return vl, rows, [int(v) for v in sec], pairs


@pytest.mark.parametrize("bits", [512, 1024, 2048])
def test_row_counts_are_the_reference_circuits(bits):
    ctx = sizes.host_ctx(64, bits)
    vl, rows, sec, _ = circuit(ctx, 65537)
    sec4 = (ctypes.c_uint64 * 4)()
    elem = int(lib().h2r_verify_advice_rows(ctx, ctypes.byref(vl), sec4))
    nl = bits // 64
    assert sec == [4 * nl + 8, elem, 1] and rows == sum(sec)
    assert rows == sizes.rsa_signature_circuit(bits)
    if bits == 2048:
        assert rows == 77356
    lib().h2r_ctx_destroy(ctx)


@pytest.mark.parametrize("bits,e", [(512, 3), (1024, 65537)])
def test_row_kinds(bits, e):
    ctx = sizes.host_ctx(64, bits)
    vl, rows, sec, _ = circuit(ctx, e)
    kinds = np.full(rows + 1, 0xEE, dtype=np.uint8)
    assert lib().h2r_verify_circuit_row_kinds(ctx, ctypes.byref(vl), kinds.ctypes.data) == 0
    assert kinds[rows] == 0xEE                                              # nothing behind the last row
    P, E = sec[0], sec[1]
    assert list(kinds[:P]) == [ROW_RANGE_LIMB, ROW_RANGE_LIMB + 1] * (P // 2)
    elem = np.zeros(E, dtype=np.uint8)
    assert lib().h2r_verify_row_kinds(ctx, ctypes.byref(vl), elem.ctypes.data) == 0
    assert np.array_equal(kinds[P:P + E], elem)
    assert kinds[P + E] == ROW_ASSERT_ONE
    lib().h2r_ctx_destroy(ctx)


@pytest.mark.parametrize("nl,e", [(8, 3), (8, 65537), (16, 65537), (32, 65537)])
def test_copy_map_is_the_models(nl, e):
    L = lib()
    ctx = sizes.host_ctx(64, 64 * nl)
    vl, rows, sec, pairs = circuit(ctx, e)
    sec4 = (ctypes.c_uint64 * 4)()
    L.h2r_verify_advice_rows(ctx, ctypes.byref(vl), sec4)
    pow_rows, rec_rows, T = int(sec4[2]), int(L.h2r_advice_rows(ctx)), int(vl.pow.num_mul_mods)
    m_rows, m_pairs, pow_first, cells = CR.signature_circuit(nl, pow_rows, rec_rows, T)
    assert m_rows == rows and pow_first == sec[0] + int(sec4[0]) + int(sec4[1])
    in_pow = lambda p: pow_first <= p[0] < pow_first + pow_rows
    # in-field + encoded-message + frame: the model's pairs, as a set
    outside = [p for p in pairs if not in_pow(p)]
    assert len(set(outside)) == len(outside) and len(set(m_pairs)) == len(m_pairs)
    assert set(outside) == set(m_pairs)
    # the pow rows: h2r_pow_copy_map at that offset, x = the signature cells, n = the modulus cells
    eb = e_bytes(e)
    pw = pairs_of(lambda out, cap: L.h2r_pow_copy_map(ctx, ctypes.byref(vl.pow), eb, len(eb), pow_first, out, cap))
    resolve = {"A": cells["sig"], "N": cells["n"]}
    want = [(r, c) + (resolve[COPY_SRC[sr]][sc] if sr in COPY_SRC else (sr, sc)) for (r, c, sr, sc) in pw]
    assert any(sr in COPY_SRC for (_, _, sr, _) in pw)
    assert set(p for p in pairs if in_pow(p)) == set(want) and len(want) == len(pairs) - len(outside)
    # closed: every source is a cell of the image; no destination is named twice
    assert all(sr < rows and sc < 5 and r < rows and c < 5 for (r, c, sr, sc) in pairs)
    assert max(sr for (_, _, sr, _) in pairs) < 0xFFFFFF00
    dst = [(r, c) for (r, c, _, _) in pairs]
    assert len(set(dst)) == len(dst)
    # the ties the parent's map did not have: the signature and the modulus are sources of both the in-field and the pow rows, the hashed
    # cells and the last record's r limbs of the encoded-message rows, the seed of the first `and`, the last AND of the last row
    em_first = pow_first + pow_rows
    by_src = {}
    for (r, c, sr, sc) in pairs:
        by_src.setdefault((sr, sc), []).append(r)
    for cell in cells["sig"] + cells["n"]:
        assert any(r < pow_first for r in by_src[cell]) and any(pow_first <= r < em_first for r in by_src[cell])
    for cell in cells["hashed"]:
        assert all(em_first <= r for r in by_src[cell])
    assert (rows - 1, 0, rows - 2, 2) in set(pairs) and any(em_first <= r for r in by_src[(sec[0], 0)])
    L.h2r_ctx_destroy(ctx)


@pytest.mark.parametrize("w,bits", [(64, 512), (64, 2048), (32, 512)])
def test_fresh_op_copy_map(w, bits):
    """assert_in_field alone against the model (operands stay H2R_COPY_SRC_A / _B); every op the builder knows has a map whose pairs stay
    inside its rows, shift with row_offset and name no destination twice."""
    L = lib()
    ctx = sizes.host_ctx(w, bits)
    nl = bits // w
    got = pairs_of(lambda out, cap: L.h2r_fresh_op_copy_map(ctx, OP_IS_IN_FIELD, ASSERT_ONE, 0, out, cap))
    m_rows, m_pairs = CR.in_field_pairs(nl)
    assert m_rows == L.h2r_fresh_op_advice_rows(ctx, OP_IS_IN_FIELD, ASSERT_ONE)
    named = set((r, c, COPY_SRC.get(sr, sr), sc) for (r, c, sr, sc) in got)
    assert named == set(m_pairs) and len(got) == len(m_pairs)
    for name, op in sizes.OPS.items():
        rows = L.h2r_fresh_op_advice_rows(ctx, op, 0)
        p0 = pairs_of(lambda out, cap: L.h2r_fresh_op_copy_map(ctx, op, 0, 0, out, cap))
        p7 = pairs_of(lambda out, cap: L.h2r_fresh_op_copy_map(ctx, op, 0, 1000, out, cap))
        assert p7 == [(r + 1000, c, sr if sr in COPY_SRC else sr + 1000, sc) for (r, c, sr, sc) in p0], name
        assert all(r < rows and c < 5 and (sr in COPY_SRC and sc < nl or sr < r and sc < 5) for (r, c, sr, sc) in p0), name
        assert len(set((r, c) for (r, c, _, _) in p0)) == len(p0), name
        if name in ("ADD_MOD", "SUB_MOD"):
            assert any(sr == 0xFFFFFF03 for (_, _, sr, _) in p0), name
    assert L.h2r_fresh_op_copy_map(ctx, 99, 0, 0, None, 0) == 0
    assert L.h2r_fresh_op_copy_map(ctx, sizes.OPS["ADD"], ASSERT_ONE, 0, None, 0) == 0    # no bit to assert: as the emitter
    L.h2r_ctx_destroy(ctx)


def test_refusals():
    L = lib()
    eb = e_bytes(65537)
    sec = (ctypes.c_uint64 * 3)()
    kinds = np.zeros(1 << 17, dtype=np.uint8)
    # a Var layout: h2r_pow_copy_map is fixed-exponent too
    ctx = sizes.host_ctx(64, 1024)
    var = _lib.H2RVerifyLayout()
    assert L.h2r_verify_layout_var(ctx, 1, 5, ctypes.byref(var)) == 0
    assert L.h2r_verify_circuit_rows(ctx, ctypes.byref(var), sec) == 0
    assert L.h2r_verify_circuit_row_kinds(ctx, ctypes.byref(var), kinds.ctypes.data) == _lib.H2R_E_UNSUPPORTED
    assert L.h2r_verify_circuit_copy_map(ctx, ctypes.byref(var), eb, len(eb), None, 0) == 0
    assert L.h2r_verify_circuit_emit_frame(ctx, ctypes.byref(var), kinds.ctypes.data, kinds.ctypes.data, kinds.ctypes.data, kinds.ctypes.data,
                                           0, 1, None, kinds.ctypes.data, 1 << 17, None) == _lib.H2R_E_UNSUPPORTED   # (and a host ctx has no device)
    # an exponent that is not the layout's
    vl = fixed_layout(ctx, 65537)
    assert L.h2r_verify_circuit_copy_map(ctx, ctypes.byref(vl), e_bytes(3), 1, None, 0) == 0
    assert L.h2r_verify_circuit_rows(None, ctypes.byref(vl), sec) == 0
    assert L.h2r_verify_circuit_row_kinds(ctx, ctypes.byref(vl), None) == _lib.H2R_E_NULL
    L.h2r_ctx_destroy(ctx)
    # L < 8: the encoded message has no room (RSAChip's check reads limbs 0 .. 7) -- no layout, and a borrowed one is refused too
    ctx8, ctx = sizes.host_ctx(64, 512), sizes.host_ctx(64, 256)
    vl = fixed_layout(ctx8, 65537)
    assert L.h2r_verify_circuit_rows(ctx8, ctypes.byref(vl), sec) > 0
    assert L.h2r_verify_layout_fixed(ctx, eb, len(eb), ctypes.byref(_lib.H2RVerifyLayout())) == _lib.H2R_E_SHAPE
    assert L.h2r_verify_circuit_rows(ctx, ctypes.byref(vl), sec) == 0
    assert L.h2r_verify_circuit_row_kinds(ctx, ctypes.byref(vl), kinds.ctypes.data) == _lib.H2R_E_UNSUPPORTED
    assert L.h2r_verify_circuit_copy_map(ctx, ctypes.byref(vl), eb, len(eb), None, 0) == 0
    L.h2r_ctx_destroy(ctx)
    L.h2r_ctx_destroy(ctx8)
