"""The argument rules of the Python front end, each in one place: what `Interpolator`, `Fields` and the `interpn_*`
helpers require of coordinate tensors, results, strides and streams, and how they hand them to the C ABI.

Messages differ between callers on purpose (they are part of the behaviour): where they do, the caller passes its words.
torch is imported only by the functions that work on tensors."""

from __future__ import annotations

import ctypes
from ctypes import c_uint64, c_void_p

import numpy as np

from . import _lib


def torch_dtype(dtype):
    """The torch dtype of tensors for a handle of numpy `dtype`."""
    import torch

    return torch.float64 if dtype == np.float64 else torch.float32


def resolve_stream(stream, device: int):
    """`stream` (None: torch's current stream on `device`; a torch Stream; a raw hipStream_t integer) as `(raw, owner)`.
    `owner` is the Stream object, which whoever enqueues on `raw` keeps alive (a raw handle whose torch Stream was
    collected would dangle), or None for a caller's integer."""
    if stream is None:
        import torch

        stream = torch.cuda.current_stream(device)
    if hasattr(stream, "cuda_stream"):
        return stream.cuda_stream, stream
    return int(stream), None


def ptr_array(addresses):
    """A `void*[]` of the addresses (integers or ctypes pointers), never of zero length."""
    addresses = list(addresses)
    return (c_void_p * max(len(addresses), 1))(*addresses)


def void_pp(ptrs):
    """The `T*[]` that `raw._slice_of_slices` made, as the `void**` the handle entry points take: the same memory."""
    return ctypes.cast(ptrs, ctypes.POINTER(c_void_p))


def eval_flags(no_alloc: bool) -> int:
    """`flags` of the device entry points."""
    return _lib.EVAL_NO_ALLOC if no_alloc else 0


def dim_mismatch(via_lib: bool = False) -> AssertionError:
    """The reference's "Dimension mismatch": spelled out by some callers, taken from the library's table by others."""
    return AssertionError(_lib.strerror(_lib.ERR_DIM_MISMATCH) if via_lib else "Dimension mismatch")


def same_device(what: str, tensor, dev: int, noun: str, none_is_current: bool = False) -> None:
    """Kernels run under the handle's device with the grid resident there: a tensor on another GPU would be read across
    devices on a stream of the wrong device.  A tensor that does not say which GPU it is on passes, or with
    `none_is_current` counts as being on torch's current device."""
    idx = tensor.device.index
    if idx is None and none_is_current:
        import torch

        idx = torch.cuda.current_device()
    if idx is not None and idx != dev:
        raise ValueError(f"{what} is on cuda:{idx} but this {noun} lives on cuda:{dev}")


def coord_tensors(name: str, tensors, want, dev: int, noun: str, none_is_current: bool = False, same_length: bool = True,
                  via_lib: bool = False) -> int:
    """`tensors` (the argument `name`, a list) must be contiguous 1-D CUDA tensors of dtype `want` on device `dev` and, with
    `same_length`, equally long; returns the length of the first (0 for none)."""
    for i, t in enumerate(tensors):
        if not (hasattr(t, "is_cuda") and t.is_cuda and t.is_contiguous() and t.dim() == 1 and t.dtype == want):
            raise TypeError(f"{name}[{i}]: expected a contiguous 1-D {want} CUDA tensor")
        if t.device.index != dev:  # the common case costs one comparison; the rest is `same_device`'s to decide
            same_device(f"{name}[{i}]", t, dev, noun, none_is_current)
    n = tensors[0].numel() if tensors else 0
    if same_length:
        for t in tensors:
            if t.numel() != n:
                raise dim_mismatch(via_lib)
    return n


def out_tensor(out, n: int, want, dev: int, via_lib: bool = False):
    """The 1-D result of an `Interpolator`: a caller's contiguous CUDA tensor of `n` elements on `dev`, or a new one."""
    if out is None:
        import torch

        return torch.empty(n, dtype=want, device=torch.device("cuda", dev))
    if not (out.is_cuda and out.is_contiguous() and out.dim() == 1 and out.dtype == want):
        raise TypeError(f"out: expected a contiguous 1-D {want} CUDA tensor")
    if out.numel() != n:
        raise dim_mismatch(via_lib)
    same_device("out", out, dev, "interpolator", True)
    return out


def check_ndarray(name: str, a, dtype: np.dtype) -> None:
    """`a` (the argument `name`) must be a numpy array of `dtype`; the first two checks of `raw._check_arr`."""
    if not isinstance(a, np.ndarray):
        raise TypeError(f"argument '{name}': expected a numpy array, got {type(a).__name__}")
    if a.dtype != dtype:
        raise TypeError(f"argument '{name}': expected dtype {dtype.name}, got {a.dtype.name}")


def elem_strides(a: np.ndarray):
    """The strides of a numpy array in elements; -1 where one is not a whole number of elements."""
    item = a.itemsize
    return [st // item if st % item == 0 else -1 for st in a.strides]


def row_stride(name: str, n: int, width: int, strides, exc, unit_msg: str, stride_msg: str, check_empty: bool = True) -> int:
    """The row stride, in elements, that an `(n, width)` array with `strides` (in elements) hands to the library: unit stride
    along a row, and rows a whole number of elements >= `width` apart.  Raises `exc` with `unit_msg` / `stride_msg`, the
    caller's words with `{name}` and `{width}` filled in; without `check_empty` an array of no rows may have any layout."""
    if width > 1 and (n or check_empty) and strides[1] != 1:
        raise exc(unit_msg.format(name=name, width=width))
    if n > 1:
        if strides[0] < width:
            raise exc(stride_msg.format(name=name, width=width))
        return int(strides[0])
    return width


def point_rows(name: str, pts, nd: int):
    """The rows of point-major `pts`, a numpy array or a torch tensor of shape `(..., nd)` whose type and dtype the caller
    has checked: `(rows, n, stride, lead)`.  A 2-D array with unit stride along a row and rows a whole number of elements
    >= `nd` apart (`buf[:, :3]` of an `(n, 4)` block) is taken as it is; anything else is copied once."""
    shape = tuple(int(v) for v in pts.shape)
    if len(shape) < 1 or shape[-1] != nd:
        raise ValueError(f"{name}: expected shape (..., {nd}), got {shape}")
    host = isinstance(pts, np.ndarray)
    strides = elem_strides(pts) if host else [int(v) for v in pts.stride()]
    if len(shape) == 2 and (nd == 1 or strides[1] == 1) and (shape[0] <= 1 or strides[0] >= nd):
        rows = pts
    else:
        rows = np.ascontiguousarray(pts).reshape(-1, nd) if host else pts.contiguous().reshape(-1, nd)
        strides = [nd, 1]
    n = int(rows.shape[0])
    return rows, n, (strides[0] if n > 1 else nd), shape[:-1]


def point_results(name: str, a, lead, tail, n: int) -> int:
    """The row stride, in elements, of the point-major result block `a` (the argument `name`; a numpy array or a torch tensor
    whose type and dtype the caller has checked) of shape `lead + tail`: a contiguous block, or with one leading axis a view
    whose rows are contiguous runs of prod(tail) elements a whole number of elements >= that apart — a row's other elements
    stay untouched."""
    shape = tuple(int(v) for v in a.shape)
    want = tuple(lead) + tuple(tail)
    if shape != want:
        raise ValueError(f"{name}: expected shape {want}, got {shape}")
    width = int(np.prod(tail, dtype=np.int64))
    host = isinstance(a, np.ndarray)
    strides = elem_strides(a) if host else [int(v) for v in a.stride()]
    if len(lead) != 1:
        if not (a.flags.c_contiguous if host else a.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous block, or one leading axis and contiguous rows")
        return width
    if n:
        run = 1
        for extent, st in zip(reversed(tail), reversed(strides[1:])):  # the row itself: C order, unit inner stride
            if extent > 1 and st != run:
                raise ValueError(f"{name}: every row must be contiguous (unit stride along the last axis)")
            run *= extent
    if n > 1:
        if strides[0] < width:
            raise ValueError(f"{name}: the row stride must be a whole number of elements, at least {width}")
        return strides[0]
    return width


def first_bad_error(status: int, index: int) -> AssertionError:
    """The error of a status that carries a first failing index (`_lib.UNREPRESENTABLE`)."""
    err = AssertionError(_lib.strerror(status))
    err.first_bad_index = index
    return err


def raise_for_indexed_status(status: int, bad: c_uint64) -> None:
    """`_lib.raise_for_status` for entry points that report the first failing index through `bad`."""
    if status in _lib.UNREPRESENTABLE:
        raise first_bad_error(status, bad.value)
    _lib.raise_for_status(status)


def finish_streams(finish, handle, raws, pending: dict) -> None:
    """Wait for the streams `raws` of `handle` with the library's `finish` and drop them from `pending`; raise the first
    other error, else the smallest first failing index any of them reports."""
    first_bad, bad_status, status = None, _lib.ERR_UNREPRESENTABLE, _lib.OK
    for raw in raws:
        bad = c_uint64(0)
        st = finish(handle, c_void_p(int(raw)), ctypes.byref(bad))
        pending.pop(raw, None)
        if st in _lib.UNREPRESENTABLE:
            bad_status = st
            first_bad = bad.value if first_bad is None else min(first_bad, bad.value)
        elif st != _lib.OK and status == _lib.OK:
            status = st
    _lib.raise_for_status(status)
    if first_bad is not None:
        raise first_bad_error(bad_status, first_bad)
