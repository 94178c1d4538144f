"""The marshalling layer of the ctypes wrappers (halo2_rsa_amd/_marshal.py) on CPU tensors: words and back, challenges, the column-block
test, a group's strides, the stride of an image, nullable pointers, and the allocate-or-unpack step with its choice of empty or zeros."""
import ctypes

import numpy as np
import pytest
import torch

from halo2_rsa_amd import _lib, _marshal as M

M64 = 2 ** 64 - 1
EDGES = [0, 1, 2 ** 64 - 1, 2 ** 64, 2 ** 255, 2 ** 256 - 1, (0x8000000000000001 << 128) | (0xFFFFFFFFFFFFFFFE << 64) | 0x8000000000000000]


@pytest.mark.parametrize("v", EDGES)
def test_words_round_trip(v):
    w = M.words(v)
    assert len(w) == 4 and all(0 <= x <= M64 for x in w) and w == [(v >> (64 * k)) % 2 ** 64 for k in range(4)]
    assert M.from_words(w) == v
    field = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    M.set_words(field, v)
    assert list(field) == w and M.from_words(field) == v
    cfg = _lib.H2RNttConfig()
    M.set_words(cfg.omega, v)       # a struct's array field is a view of the struct: the words land in it
    assert list(cfg.omega) == w and list(cfg.shift) == [0] * 4
    # a word with its top bit set is negative in the int64 view a device tensor holds; from_words reads it back unsigned
    row = torch.from_numpy(np.array(w, dtype=np.uint64).view(np.int64))
    assert M.from_words(row) == v
    assert M.words(np.uint64(v & M64)) == [v & M64, 0, 0, 0]


def test_challenges_of_a_list_and_a_nested_list():
    flat = M.challenges(EDGES[:3], "cpu", 3)
    assert flat.dtype == torch.int64 and tuple(flat.shape) == (3, 4)
    assert [M.from_words(r) for r in flat] == EDGES[:3]
    assert tuple(M.challenges(tuple(EDGES), "cpu").shape) == (len(EDGES), 4)
    points = [EDGES[0:3], EDGES[3:6]]
    nested = M.challenges(points, "cpu")
    assert nested.dtype == torch.int64 and tuple(nested.shape) == (2, 3, 4)
    assert [[M.from_words(w) for w in row] for row in nested] == points
    assert nested[1, 2].tolist() == [-1, -1, -1, -1]       # 2^256 - 1: the uint64 -> int64 view
    with pytest.raises(AssertionError):
        M.challenges(EDGES[:3], "cpu", 2)
    with pytest.raises(AssertionError):
        M.challenges(points, "cpu", 2)                     # a batch names a per-circuit list, not a nested one


def test_column_predicate():
    n, b, c = 8, 2, 3
    for t in (torch.zeros((n, 32), dtype=torch.uint8), torch.zeros((b, n, 32), dtype=torch.uint8), torch.zeros((b, c, n, 32), dtype=torch.uint8)):
        assert M.is_columns(t) and M.is_columns(t, rows=n, dims=(2, 3, 4), batch=b)
    t3 = torch.zeros((b, n, 32), dtype=torch.uint8)
    assert M.is_columns(torch.zeros((2 * b, n, 32), dtype=torch.uint8)[::2], rows=n, batch=b)      # any leading stride
    assert M.is_columns(torch.zeros((c, b, n, 32), dtype=torch.uint8).transpose(0, 1), dims=(4,), batch=b)
    assert not M.is_columns(t3.view(torch.int8))                                                    # wrong dtype
    assert not M.is_columns(torch.zeros((b, n, 31), dtype=torch.uint8))                             # last dimension 31
    assert not M.is_columns(torch.zeros((b, 32, n), dtype=torch.uint8).transpose(1, 2))             # a transposed view
    wide = torch.zeros((b, n, 64), dtype=torch.uint8)[..., :32]
    assert not M.is_columns(wide)                                                                   # a row stride of 64
    assert M.is_columns(wide, strides=False) and not M.is_columns(wide.view(torch.int8), strides=False)
    assert not M.is_columns(t3, rows=n + 1)                                                         # a wrong row count
    assert not M.is_columns(t3, batch=b + 1)                                                        # a wrong batch
    assert not M.is_columns(t3, dims=(2, 4)) and not M.is_columns(torch.zeros(32, dtype=torch.uint8))


def test_column_group_strides():
    n = 8
    pc = torch.zeros((2, 3, n, 32), dtype=torch.uint8)
    assert M.column_group(pc, True) == (pc.data_ptr(), 3 * n * 32, n * 32)
    cm = torch.zeros((3, 2, n, 32), dtype=torch.uint8).transpose(0, 1)        # [column][circuit] in memory
    assert M.column_group(cm, True) == (cm.data_ptr(), n * 32, 2 * n * 32)
    key = torch.zeros((5, 2 * n, 32), dtype=torch.uint8)[:, :n]
    assert M.column_group(key, False) == (key.data_ptr(), 0, 2 * n * 32)
    one = torch.zeros((4, n, 32), dtype=torch.uint8)[::2]
    assert M.column_group(one, True) == (one.data_ptr(), 2 * n * 32, n * 32)   # [batch, n, 32]: one column per circuit
    assert M.column_group(one[0], False) == (one.data_ptr(), 0, n * 32)        # [n, 32]: a key's single column


def test_image_stride_ptr_ref_workspace_kinds():
    assert M.image_stride(torch.zeros((3, 320), dtype=torch.uint8), 3) == 320
    assert M.image_stride(torch.zeros(960, dtype=torch.uint8), 3) == 320
    assert M.image_stride(torch.zeros(0, dtype=torch.uint8), 0) == 0 and M.image_stride(torch.zeros(960, dtype=torch.uint8), 0) == 960
    t = torch.zeros(4, dtype=torch.uint8)
    assert M.ptr(None) is None and M.ptr(t) == t.data_ptr()
    assert M.ref(None) is None and M.ref(_lib.H2RLayout()) is not None
    assert M.workspace(0, "cpu").numel() == 16 and M.workspace(40, "cpu").numel() == 40 and M.workspace(0, "cpu", floor=0).numel() == 0
    assert M.workspace(40, "cpu").dtype == torch.uint8
    kd = torch.arange(4, dtype=torch.uint8)
    assert M.kinds_tensor(kd, "cpu") is kd
    assert M.kinds_tensor(np.arange(4), "cpu").dtype == torch.uint8 and M.kinds_tensor([3, 1], "cpu").tolist() == [3, 1]


def test_outputs_hand_back_or_allocate():
    mine = (torch.full((2, 3), 7, dtype=torch.uint8), None)
    assert M.outputs(mine, "cpu", (torch.zeros, torch.uint8, (9,)), status=2) is mine and mine[0].tolist() == [[7] * 3] * 2
    one = torch.full((4,), 7, dtype=torch.int64)
    assert M.outputs(one, "cpu", (torch.zeros, torch.int64, (4,))) is one and one.tolist() == [7] * 4
    # open_witness: W and the remainders are documented as zeros where no column queries a point; the status starts at zero
    W, be, status = M.outputs(None, "cpu", (torch.zeros, torch.uint8, (2, 3, 8, 32)), (torch.zeros, torch.int64, (2, 3, 4)), status=2)
    assert (W.dtype, tuple(W.shape)) == (torch.uint8, (2, 3, 8, 32)) and (be.dtype, tuple(be.shape)) == (torch.int64, (2, 3, 4))
    assert (status.dtype, tuple(status.shape)) == (torch.uint8, (2,)) and not W.any() and not be.any() and not status.any()
    # a product call: Z is written whole (empty), the status must still be zeros
    z, status = M.outputs(None, "cpu", (torch.empty, torch.uint8, (2, 5, 7, 32)), status=2)
    assert (z.dtype, tuple(z.shape)) == (torch.uint8, (2, 5, 7, 32)) and status.tolist() == [0, 0]
    single = M.outputs(None, "cpu", (torch.zeros, torch.int64, (2, 1, 2, 4)))
    assert isinstance(single, torch.Tensor) and tuple(single.shape) == (2, 1, 2, 4) and not single.any()
    made = []
    M.outputs(None, "cpu", (lambda shape, **kw: made.append("empty") or torch.empty(shape, **kw), torch.uint8, (1,)),
              (lambda shape, **kw: made.append("zeros") or torch.zeros(shape, **kw), torch.uint8, (1,)))
    assert made == ["empty", "zeros"]                      # each spec's own factory makes its tensor


def test_hold_keeps_one_slot_per_method():
    class Obj:
        pass
    o, a, b = Obj(), torch.zeros(1), torch.zeros(2)
    M.hold(o, "hist_advice", a)
    M.hold(o, "permuted_columns", b, None)
    assert o._held == {"hist_advice": (a,), "permuted_columns": (b, None)}
    M.hold(o, "hist_advice", b)
    assert o._held["hist_advice"] == (b,) and o._held["permuted_columns"] == (b, None)
