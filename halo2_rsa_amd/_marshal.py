"""What a ctypes wrapper of a device export does between its arguments and the call (the Python half).  Shared by
`prover` and `big_integer`; nothing here calls the library."""
import ctypes

import numpy as np
import torch


def words(v):
    """The four little-endian 64-bit words of int(v)."""
    v = int(v)
    return [(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]


def from_words(w) -> int:
    """The integer of four little-endian 64-bit words (a list, a ctypes uint64[4], a row of an int64 tensor)."""
    return sum((int(w[k]) & (2 ** 64 - 1)) << (64 * k) for k in range(4))


def set_words(field, v):
    """field (a ctypes uint64[4]: a constant of a configuration struct) = words(v)."""
    field[:] = words(v)


def challenges(values, dev, batch=None) -> torch.Tensor:
    """int64 [values' shape..., 4] on `dev`: the words of a per-circuit list of integers (batch: how many it must hold), or of the
    nested [batch][num_points] list of opening points.  An int64 tensor already on a device ([batch, 4] or [batch, num_points, 4]: what
    prover.Transcript draws) passes through where it lies; a strided view of one is made contiguous there."""
    if isinstance(values, torch.Tensor) and values.is_cuda and values.dtype == torch.int64:
        assert values.dim() in (2, 3) and values.shape[-1] == 4
        assert batch is None or tuple(values.shape) == (batch, 4)
        return values if values.is_contiguous() else values.contiguous()

    def nest(v):
        return [nest(x) for x in v] if isinstance(v, (list, tuple, range)) or getattr(v, "ndim", 0) else words(v)
    w = np.array(nest(values), dtype=np.uint64)
    assert batch is None or w.shape == (batch, 4)
    return torch.from_numpy(w.view(np.int64)).to(dev)


def kinds_tensor(kinds, dev) -> torch.Tensor:
    """uint8 row kinds on the device: a tensor is used as it is, anything numpy takes is copied there."""
    return kinds if isinstance(kinds, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(kinds, dtype=np.uint8)).to(dev)


def is_columns(t, rows=None, dims=None, batch=None, strides=True) -> bool:
    """Whether t is a block of 32-byte columns: uint8 [..., rows, 32] whose last two dimensions are contiguous.  rows: its row count;
    dims: the numbers of dimensions it may have; batch: shape[0] unless it is a bare [rows, 32] column, which every circuit shares;
    strides=False leaves the two strides out (for a method that refuses the shape first and asserts the strides after)."""
    if t.dtype != torch.uint8 or t.dim() < 2 or t.shape[-1] != 32 or (strides and (t.stride(-1) != 1 or t.stride(-2) != 32)):
        return False
    return (rows is None or t.shape[-2] == rows) and (dims is None or t.dim() in dims) and (batch is None or t.dim() == 2 or t.shape[0] == batch)


def column_group(t, per_circuit: bool):
    """(base, elem_stride, col_stride) of a column group [circuits][columns][rows][32].  A key's group (per_circuit=False) has no circuits
    dimension and element stride 0; a group without a columns dimension is one column."""
    has_columns = t.dim() - (1 if per_circuit else 0) > 2
    return t.data_ptr(), t.stride(0) if per_circuit else 0, t.stride(-3) if has_columns else t.shape[-2] * 32


def outputs(out, dev, *specs, status=None):
    """The caller's `out`, handed back untouched, or new tensors on `dev`: one per spec = (torch.empty or torch.zeros, dtype, shape),
    then for status=batch the call's own zeroed uint8 [batch] status.  A tuple, or the tensor itself where there is one."""
    if out is not None:
        return out
    specs += ((torch.zeros, torch.uint8, (status,)),) if status is not None else ()
    new = tuple(make(shape, dtype=dtype, device=dev) for make, dtype, shape in specs)
    return new if len(new) > 1 else new[0]


def workspace(nbytes, dev, floor: int = 16) -> torch.Tensor:
    """uint8 [max(nbytes, floor)] on `dev`: a call's scratch memory (with the floor its pointer is never null)."""
    return torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=dev)


def ptr(t):
    """t.data_ptr(), or None (a null pointer) for None."""
    return None if t is None else t.data_ptr()


def ref(struct):
    """ctypes.byref(struct), or None (a null pointer) for None."""
    return None if struct is None else ctypes.byref(struct)


def image_stride(image, batch: int) -> int:
    """Bytes between the images of two elements: the row of a [batch, bytes] tensor, an equal share of a flat buffer."""
    return image.shape[1] if image.dim() > 1 else image.numel() // max(batch, 1)


def hold(obj, method: str, *tensors):
    """Keeps a call's temporaries and operands alive with `obj` until its next call of `method`: until the stream has run the kernels."""
    obj.__dict__.setdefault("_held", {})[method] = tensors
