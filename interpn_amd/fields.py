"""Field sets: K value grids ("fields") on one grid, evaluated at the same points in one pass
(`interpn_hip_fields_*` of include/interpn_hip.h) — equation-of-state tables, vector fields, colour
channels, scipy's RegularGridInterpolator with trailing value dimensions.

`Fields` is the persistent form (the counterpart of `Interpolator`), `interpn_fields()` the one-call
form (the counterpart of `interpn()`), `interpn_fields_grad()` the one-call form with the Jacobian.  Row f of every result is bit-identical to what the single
interpolator of field f returns.  On a lattice (one coordinate vector per axis): `Fields.eval_lattice*` /
`interpn_fields_lattice()` for the values, `Fields.eval_lattice_grad*` / `interpn_fields_lattice_grad()` with the Jacobian.
"""

from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_uint64, c_void_p

import numpy as np

from . import _args, _lib, _setup
from ._setup import is_tensor as _is_tensor
from .handle import Interpolator
from .raw import _check_arr, _dims, _slice_of_slices


def _field_axis(field_axis) -> int:
    if field_axis not in (0, -1):
        raise ValueError("field_axis: expected 0 (fields first) or -1 (fields last)")
    return _lib.FIELDS_LATTICE_FIELD_MAJOR if field_axis == 0 else _lib.FIELDS_LATTICE_FIELDS_LAST


def _lattice_out_stride(shape, strides, k, m, layout, contiguous) -> int:
    """The element stride a lattice result of `shape` / `strides` (in elements) hands to the library, for K fields on a
    lattice of axis lengths `m`; ValueError for a wrong shape or a layout the kernels cannot write."""
    count = int(np.prod(m, dtype=object)) if m else 0
    shape, m = tuple(int(v) for v in shape), tuple(m)
    if layout == _lib.FIELDS_LATTICE_FIELD_MAJOR:
        if shape != (k,) + m and shape != (k, count):
            raise ValueError(f"out: expected shape {(k,) + m}, got {shape}")
        if count == 0:
            return 0
        inner, want = strides[1:], 1  # each field's block in C order
        for n, st in zip(reversed(shape[1:]), reversed(inner)):
            if n > 1 and st != want:
                raise ValueError("out: each field's block must be contiguous")
            want *= n
        if k > 1 and strides[0] < count:
            raise ValueError(f"out: the stride from field to field must be at least {count} elements")
        return int(strides[0]) if k > 1 else count
    if shape == m + (k,) and contiguous:
        return k
    if len(shape) == 2 and shape == (count, k):
        if count and k > 1 and strides[1] != 1:
            raise ValueError("out: every row must be contiguous (unit stride along the last axis)")
        if count > 1 and strides[0] < k:
            raise ValueError(f"out: the row stride must be at least {k} elements")
        return int(strides[0]) if count > 1 else k
    if shape != m + (k,):
        raise ValueError(f"out: expected shape {m + (k,)}, got {shape}")
    raise ValueError(f"out: expected a C-contiguous array, or a 2-D ({count}, >= {k}) view with contiguous rows")


def _lattice_jac_stride(shape, strides, k, nd, m, layout, contiguous) -> int:
    """`_lattice_out_stride` for the Jacobian of K fields in N dimensions on a lattice of axis lengths `m`: field-major
    `(K, N, *m)` or `(K, N, prod(m))` with every (f, d) block contiguous and ONE stride between the K * N blocks;
    fields-last `(*m, K, N)` C-contiguous, or a `(prod(m), K, N)` view whose rows of K * N elements are contiguous."""
    count = int(np.prod(m, dtype=object)) if m else 0
    shape, m = tuple(int(v) for v in shape), tuple(m)
    if layout == _lib.FIELDS_LATTICE_FIELD_MAJOR:
        if shape != (k, nd) + m and shape != (k, nd, count):
            raise ValueError(f"jac: expected shape {(k, nd) + m}, got {shape}")
        if count == 0:
            return 0
        want = 1  # each (f, d) block in C order
        for n, st in zip(reversed(shape[2:]), reversed(strides[2:])):
            if n > 1 and st != want:
                raise ValueError("jac: each component's block must be contiguous")
            want *= n
        row = int(strides[1]) if nd > 1 else (int(strides[0]) if k > 1 else count)
        if row < count or (k > 1 and nd > 1 and strides[0] != nd * row):
            raise ValueError(f"jac: one uniform stride of at least {count} elements between the K * N blocks "
                             "(stride(0) == N * stride(1))")
        return row
    if shape == m + (k, nd) and contiguous:
        return k * nd
    if len(shape) == 3 and shape == (count, k, nd):
        if count and ((nd > 1 and strides[2] != 1) or (k > 1 and strides[1] != nd)):
            raise ValueError("jac: every row of K * N elements must be contiguous")
        if count > 1 and strides[0] < k * nd:
            raise ValueError(f"jac: the row stride must be at least {k * nd} elements")
        return int(strides[0]) if count > 1 else k * nd
    if shape != m + (k, nd):
        raise ValueError(f"jac: expected shape {m + (k, nd)}, got {shape}")
    raise ValueError(f"jac: expected a C-contiguous array, or a 3-D ({count}, {k}, {nd}) view with contiguous rows")


_ROWS_UNIT = "out: every row must be contiguous (unit stride along the last axis)"  # point-major (n, K) results


def _value_row_stride(n: int, strides) -> int:
    """The element stride between the K rows of a (K, n) result with `strides` (in elements; -1: not a whole number of
    elements): rows contiguous, any row stride >= n."""
    if n == 0:
        return 0
    if strides[1] != 1 or strides[0] < n:
        raise ValueError("out: rows must be contiguous")
    return int(strides[0])


def _grad_row_stride(shape, strides) -> int:
    """The one element stride between the K * N rows of a (K, N, n) gradient block of `shape` / `strides` (in elements; -1:
    not a whole number of elements); ValueError for a layout the kernels cannot write."""
    k, nd, n = (int(v) for v in shape)
    if n == 0 or k * nd == 0:
        return 0
    if n > 1 and strides[2] != 1:
        raise ValueError("grad: the last axis must be contiguous (unit stride)")
    row = int(strides[1]) if nd > 1 else (int(strides[0]) if k > 1 else n)
    if row < n or (k > 1 and nd > 1 and strides[0] != nd * row):
        raise ValueError(f"grad: one uniform stride of at least {n} elements between the K * N rows (stride(0) == N * stride(1))")
    return row


def _field_major(vals, nper, dtype):
    """`vals` as (address, nvals, nfields, field_stride, mem kind, keepalive): an array or tensor of shape
    (K, *dims) or (K, prod(dims)), or a sequence of K arrays / tensors of prod(dims) values each."""
    if isinstance(vals, (list, tuple)):
        if not vals:
            raise ValueError("argument 'vals': expected at least one field")
        if all(_is_tensor(v) for v in vals):
            import torch

            vals = torch.stack([v.reshape(-1) for v in vals])
        else:
            vals = np.stack([np.asarray(v).ravel() for v in vals])
    if isinstance(vals, np.ndarray):
        if vals.ndim < 2:
            raise ValueError("argument 'vals': expected shape (K, *dims) or (K, prod(dims))")
        if vals.dtype != dtype:
            raise TypeError(f"argument 'vals': expected dtype {np.dtype(dtype).name}, got {vals.dtype.name}")
        k = vals.shape[0]
        v = np.ascontiguousarray(vals).reshape(k, -1)
        if v.shape[1] != nper:
            raise ValueError(f"argument 'vals': expected {nper} values per field, got {v.shape[1]}")
        return v.ctypes.data_as(c_void_p), v.size, k, v.shape[1], _lib.MEM_HOST, v
    if _is_tensor(vals):
        if vals.dim() < 2:
            raise ValueError("argument 'vals': expected shape (K, *dims) or (K, prod(dims))")
        want = "torch.float64" if dtype == np.float64 else "torch.float32"
        if str(vals.dtype) != want:
            raise TypeError(f"argument 'vals': expected {want}, got {vals.dtype}")
        k = vals.shape[0]
        v = vals.contiguous().reshape(k, -1)
        if v.shape[1] != nper:
            raise ValueError(f"argument 'vals': expected {nper} values per field, got {v.shape[1]}")
        mem = _lib.MEM_DEVICE if v.is_cuda else _lib.MEM_HOST
        return c_void_p(v.data_ptr()), v.numel(), k, v.shape[1], mem, v
    raise TypeError("argument 'vals': expected a numpy array, a torch tensor or a sequence of them")


class Fields:
    """K fields on one grid, resident on the device.  `last_path` is "fused" (one pass of
    `interpn::k_linear_fields`: multilinear, N = 2, 3) or "per_field" (K evaluations through K ordinary
    interpolators: every other method and N, and sets without the fused table)."""

    def __init__(self, handle: int, dtype, ndims: int, nfields: int, keepalive=None):
        self._h = c_void_p(handle)
        self.dtype = np.dtype(dtype)
        self._ndims = ndims
        self.nfields = nfields
        self._keepalive = keepalive
        self._pending_streams = {}
        self.last_path = None
        self.last_points_path = None

    # -- construction ---------------------------------------------------------------------
    @classmethod
    def regular(cls, method: str, dims, starts, steps, vals, linearize_extrapolation: bool = False, device: int = -1,
                dtype=None, fma=None) -> "Fields":
        dtype = np.dtype(dtype or starts.dtype)
        sfx = "f64" if dtype == np.float64 else "f32"
        ct = c_double if dtype == np.float64 else c_float
        d, nd = _dims(dims)
        starts = _check_arr("starts", starts, dtype)
        steps = _check_arr("steps", steps, dtype)
        nper = int(np.prod([int(v) for v in dims], dtype=object)) if nd else 1
        vptr, nvals, k, stride, mem, keep = _field_major(vals, nper, dtype)
        h = c_void_p()
        st = getattr(_lib.load(), f"interpn_hip_create_fields_regular_{sfx}")(
            Interpolator._method_arg(method, fma), d, nd, starts.ctypes.data_as(POINTER(ct)), starts.size,
            steps.ctypes.data_as(POINTER(ct)), steps.size, vptr, nvals, k, stride, mem, int(bool(linearize_extrapolation)),
            int(device), ctypes.byref(h))
        _lib.raise_for_status(st)
        return cls(h.value, dtype, nd, k, keep if mem == _lib.MEM_DEVICE else None)

    @classmethod
    def rectilinear(cls, method: str, grids, vals, linearize_extrapolation: bool = False, device: int = -1, dtype=None,
                    fma=None) -> "Fields":
        dtype = np.dtype(dtype or grids[0].dtype)
        sfx = "f64" if dtype == np.float64 else "f32"
        gptr, glen, ng, _keep_grids = _slice_of_slices("grids", grids, dtype)
        nper = int(np.prod([int(g.size) for g in grids], dtype=object)) if ng else 1
        vptr, nvals, k, stride, mem, keep = _field_major(vals, nper, dtype)
        h = c_void_p()
        st = getattr(_lib.load(), f"interpn_hip_create_fields_rectilinear_{sfx}")(
            Interpolator._method_arg(method, fma), gptr, glen, ng, vptr, nvals, k, stride, mem,
            int(bool(linearize_extrapolation)), int(device), ctypes.byref(h))
        _lib.raise_for_status(st)
        return cls(h.value, dtype, ng, k, keep if mem == _lib.MEM_DEVICE else None)

    # -- what the set says about itself ---------------------------------------------------
    def ndims(self) -> int:
        return self._ndims

    def device(self) -> int:
        return _lib.load().interpn_hip_fields_device(self._h)

    def set_option(self, name: str, value: int) -> None:
        """"fused" (-1 automatic, 0 never, 1 wherever the set has the table); other names go to the K interpolators."""
        _lib.raise_for_status(_lib.load().interpn_hip_fields_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = ctypes.c_longlong(0)
        _lib.raise_for_status(_lib.load().interpn_hip_fields_get_option(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def kernel_name(self) -> str:
        buf = ctypes.create_string_buffer(256)
        _lib.raise_for_status(_lib.load().interpn_hip_fields_kernel_name(self._h, buf, len(buf)))
        return buf.value.decode()

    def _took(self) -> str:
        self.last_path = "fused" if self.get_option("last_path") == _lib.FIELDS_PATH_FUSED else "per_field"
        return self.last_path

    def _tensor_values(self, out, n: int, want, dev: int):
        """`(out, row stride)` of the (K, n) values of the device forms: a caller's tensor checked, or a new one."""
        k = self.nfields
        if out is None:
            import torch

            out = torch.empty((k, n), dtype=want, device=torch.device("cuda", dev))
        elif not (out.is_cuda and out.dim() == 2 and out.dtype == want and tuple(out.shape) == (k, n)):
            raise TypeError(f"out: expected a ({k}, {n}) {want} CUDA tensor")
        return out, _value_row_stride(n, out.stride())

    # -- evaluation -----------------------------------------------------------------------
    def eval_host(self, obs, out=None) -> np.ndarray:
        """Every field at host points (synchronous): a (K, n) array.  `out` may be a (K, n) array whose rows are
        contiguous (a row stride beyond n is fine: a view of a wider array)."""
        optr, olen, nobs, _keep = _slice_of_slices("obs", obs, self.dtype)
        n = int(olen[0]) if nobs else 0
        if out is None:
            out = np.zeros((self.nfields, n), dtype=self.dtype)
        if not isinstance(out, np.ndarray) or out.dtype != self.dtype or out.shape != (self.nfields, n):
            raise ValueError(f"out: expected a ({self.nfields}, {n}) array of {self.dtype.name}")
        stride = _value_row_stride(n, _args.elem_strides(out))
        if not out.flags.writeable:
            raise ValueError("out: array is read-only")
        vp = _args.void_pp(optr)
        st = _lib.load().interpn_hip_fields_eval_host(self._h, vp, olen, nobs, c_void_p(out.ctypes.data), stride, n)
        self._took()
        _lib.raise_for_status(st)
        return out

    def eval_device_ptrs(self, obs_ptrs, out_ptr: int, out_stride: int, npoints: int, stream: int = 0,
                         no_alloc: bool = False) -> str:
        """Enqueue one evaluation on device buffers given as raw addresses; returns the path taken."""
        vp = _args.ptr_array(int(p) for p in obs_ptrs)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_fields_eval_device(self._h, vp, len(obs_ptrs), c_void_p(int(out_ptr)), int(out_stride),
                                                        int(npoints), c_void_p(int(stream)), _args.eval_flags(no_alloc),
                                                        ctypes.byref(path))
        _lib.raise_for_status(st)
        self.last_path = "fused" if path.value == _lib.FIELDS_PATH_FUSED else "per_field"
        self._pending_streams.setdefault(int(stream), None)
        return self.last_path

    def eval_tensors(self, obs, out=None, stream=None, no_alloc: bool = False):
        """Every field at points held in torch CUDA tensors (asynchronous on torch's current stream unless given):
        a (K, n) tensor.  `out` may be a (K, n) tensor with contiguous rows.  Call `finish()` to synchronise and
        surface "Unrepresentable coordinate value"."""
        want = _args.torch_dtype(self.dtype)
        obs = list(obs)
        dev = self.device()
        n = _args.coord_tensors("obs", obs, want, dev, "set")
        out, stride = self._tensor_values(out, n, want, dev)
        raw, owner = _args.resolve_stream(stream, dev)
        self.eval_device_ptrs([t.data_ptr() for t in obs], out.data_ptr(), stride, n, raw, no_alloc)
        self._pending_streams[raw] = owner
        return out

    # -- values and Jacobian: (K, n) values and (K, N, n) components in one pass --------------
    def eval_grad_host(self, obs, out=None, grad=None):
        """Every field and its gradient at host points (synchronous; `interpn_hip_fields_eval_grad_host`): `(out, grad)`,
        `out` of shape (K, n) with the bits of `eval_host`, `grad` of shape (K, N, n) whose block f has the bits of
        `Interpolator.eval_grad_host` (multicubic sets: `eval_cubic_grad_host`) of field f alone.  `out`: rows contiguous,
        any row stride >= n; `grad`: unit stride along its last axis and one uniform stride >= n between its K * N rows.
        On "Unrepresentable coordinate value" exactly the elements in front of the failing point are written, in every
        value and gradient row."""
        optr, olen, nobs, _keep = _slice_of_slices("obs", obs, self.dtype)
        n = int(olen[0]) if nobs else 0
        k, nd = self.nfields, self._ndims
        if out is None:
            out = np.zeros((k, n), dtype=self.dtype)
        if grad is None:
            grad = np.zeros((k, nd, n), dtype=self.dtype)
        if not isinstance(out, np.ndarray) or out.dtype != self.dtype or out.shape != (k, n):
            raise ValueError(f"out: expected a ({k}, {n}) array of {self.dtype.name}")
        if not isinstance(grad, np.ndarray) or grad.dtype != self.dtype or grad.shape != (k, nd, n):
            raise ValueError(f"grad: expected a ({k}, {nd}, {n}) array of {self.dtype.name}")
        stride = _value_row_stride(n, _args.elem_strides(out))
        gstride = _grad_row_stride(grad.shape, _args.elem_strides(grad))
        if not (out.flags.writeable and grad.flags.writeable):
            raise ValueError("out, grad: array is read-only")
        vp = _args.void_pp(optr)
        st = _lib.load().interpn_hip_fields_eval_grad_host(self._h, vp, olen, nobs, c_void_p(out.ctypes.data), stride,
                                                          c_void_p(grad.ctypes.data), max(gstride, n), n)
        self._took()
        _lib.raise_for_status(st)
        return out, grad

    def eval_grad_device_ptrs(self, obs_ptrs, out_ptr: int, out_stride: int, grad_ptr: int, grad_stride: int, npoints: int,
                              stream: int = 0, no_alloc: bool = False) -> str:
        """Enqueue one value-and-Jacobian evaluation on device buffers given as raw addresses; returns the path taken."""
        vp = _args.ptr_array(int(p) for p in obs_ptrs)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_fields_eval_grad_device(self._h, vp, len(obs_ptrs), c_void_p(int(out_ptr)), int(out_stride),
                                                            c_void_p(int(grad_ptr)), int(grad_stride), int(npoints),
                                                            c_void_p(int(stream)), _args.eval_flags(no_alloc), ctypes.byref(path))
        _lib.raise_for_status(st)
        self.last_path = "fused" if path.value == _lib.FIELDS_PATH_FUSED else "per_field"
        self._pending_streams.setdefault(int(stream), None)
        return self.last_path

    def eval_grad_tensors(self, obs, out=None, grad=None, stream=None, no_alloc: bool = False):
        """The same on torch CUDA tensors (asynchronous on torch's current stream unless given;
        `interpn_hip_fields_eval_grad_device`): `(out, grad)` of shapes (K, n) and (K, N, n).  Sets with the fused table
        run one launch of `interpn::k_linear_fields_grad`, which allocates nothing and can be captured into a graph;
        `last_path` says which path ran.  `out`: rows contiguous, any row stride >= n; `grad`: unit stride along its last
        axis and one uniform stride >= n between its K * N rows.  Call `finish()` to synchronise and surface
        "Unrepresentable coordinate value"."""
        want = _args.torch_dtype(self.dtype)
        obs = list(obs)
        dev = self.device()
        n = _args.coord_tensors("obs", obs, want, dev, "set")
        k, nd = self.nfields, self._ndims
        out, stride = self._tensor_values(out, n, want, dev)
        if grad is None:
            import torch

            grad = torch.empty((k, nd, n), dtype=want, device=torch.device("cuda", dev))
        elif not (grad.is_cuda and grad.dim() == 3 and grad.dtype == want and tuple(grad.shape) == (k, nd, n)):
            raise TypeError(f"grad: expected a ({k}, {nd}, {n}) {want} CUDA tensor")
        gstride = _grad_row_stride(tuple(grad.shape), grad.stride())
        raw, owner = _args.resolve_stream(stream, dev)
        self.eval_grad_device_ptrs([t.data_ptr() for t in obs], out.data_ptr(), stride, grad.data_ptr(),
                                   max(gstride, n) if n else 0, n, raw, no_alloc)
        self._pending_streams[raw] = owner
        return out, grad

    def eval_grad(self, obs, out=None, grad=None, **kwargs):
        """`eval_grad_tensors` for torch tensors, `eval_grad_host` for numpy arrays (by the type of `obs[0]`)."""
        obs = list(obs)
        if obs and _is_tensor(obs[0]):
            return self.eval_grad_tensors(obs, out, grad, **kwargs)
        if kwargs:
            raise TypeError(f"eval_grad on host arrays takes no {sorted(kwargs)}")
        return self.eval_grad_host(obs, out, grad)

    # -- point-major evaluation: (n, N) points in, (n, K) values out -------------------------
    def reserve_points(self, npoints: int, nstreams: int = 1) -> None:
        """Pre-allocate the scratch that split-path point-major evaluations of up to `npoints` points on up to `nstreams`
        concurrent streams need (`interpn_hip_fields_reserve_points`); afterwards they work with `no_alloc=True` and
        under graph capture.  The fused kernel (sets with the fused table) needs none."""
        _lib.raise_for_status(_lib.load().interpn_hip_fields_reserve_points(self._h, int(npoints), int(nstreams)))

    def _took_points(self) -> None:
        self.last_points_path = _lib.FIELDS_POINTS_PATHS.get(self.get_option("last_points_path"))
        self._took()

    def eval_points_host(self, pts, out=None) -> np.ndarray:
        """Every field at the rows of a host array of shape `(n, N)` or `(..., N)` (synchronous;
        `interpn_hip_fields_eval_points_host`): an `(n, K)` or `(..., K)` array whose element `[i, f]` has the bits of
        `eval_host(columns)[f, i]`.  A C-contiguous array, or a 2-D view whose last axis is unit-stride and whose row
        stride is a whole number of elements (`buf[:, :3]` of an `(n, 4)` array), is taken as it is; anything else is
        copied once.  `out` may have any row stride >= K with unit-stride rows; elements behind a row's first K are not
        touched.  On "Unrepresentable coordinate value" exactly the rows in front of the failing point are written."""
        _args.check_ndarray("pts", pts, self.dtype)
        nd, k, item = self._ndims, self.nfields, self.dtype.itemsize
        if pts.ndim < 1 or pts.shape[-1] != nd:
            raise ValueError(f"argument 'pts': expected shape (..., {nd}), got {tuple(pts.shape)}")
        lead = tuple(pts.shape[:-1])
        if pts.ndim == 2 and (nd == 1 or pts.strides[1] == item) and (
                pts.shape[0] <= 1 or (pts.strides[0] % item == 0 and pts.strides[0] >= nd * item)):
            rows = pts
        else:
            rows = np.ascontiguousarray(pts).reshape(-1, nd)
        n = rows.shape[0]
        stride = rows.strides[0] // item if n > 1 else nd
        if out is None:
            out = np.zeros(lead + (k,), dtype=self.dtype)
        if not isinstance(out, np.ndarray) or out.dtype != self.dtype:
            raise TypeError(f"out: expected a numpy array of {self.dtype.name}")
        if tuple(out.shape) != lead + (k,):
            raise ValueError(f"out: expected shape {lead + (k,)}, got {tuple(out.shape)}")
        if not out.flags.writeable:
            raise ValueError("out: array is read-only")
        if out.ndim == 2:
            ostride = _args.row_stride("out", n, k, _args.elem_strides(out), ValueError, _ROWS_UNIT,
                                       "out: the row stride must be a whole number of elements, at least {width}", check_empty=False)
        else:
            if not out.flags.c_contiguous:
                raise ValueError("out: expected a C-contiguous array, or a 2-D array with contiguous rows")
            ostride = k
        st = _lib.load().interpn_hip_fields_eval_points_host(self._h, c_void_p(rows.ctypes.data), stride, n, c_void_p(out.ctypes.data),
                                                            ostride)
        self._took_points()
        _lib.raise_for_status(st)
        return out

    def eval_points_tensors(self, pts, out=None, stream=None, no_alloc: bool = False):
        """The same on a torch CUDA tensor (asynchronous on torch's current stream unless given;
        `interpn_hip_fields_eval_points_device`): no `pts.T.contiguous()` in front and no transpose of the result behind.
        `pts` and `out` must not overlap.  Sets with the fused table run one kernel, which can be captured into a graph;
        `last_points_path` says which path ran; `finish()` synchronises and surfaces "Unrepresentable coordinate value"."""
        want = _args.torch_dtype(self.dtype)
        nd, k = self._ndims, self.nfields
        if not (hasattr(pts, "is_cuda") and pts.is_cuda and pts.dtype == want):
            raise TypeError(f"pts: expected a {want} CUDA tensor of shape (..., {nd})")
        if pts.dim() < 1 or pts.shape[-1] != nd:
            raise ValueError(f"pts: expected shape (..., {nd}), got {tuple(pts.shape)}")
        dev = self.device()
        _args.same_device("pts", pts, dev, "set")
        lead = tuple(pts.shape[:-1])
        if pts.dim() == 2 and (nd == 1 or pts.stride(1) == 1) and (pts.shape[0] <= 1 or pts.stride(0) >= nd):
            rows = pts
        else:
            rows = pts.contiguous().reshape(-1, nd)
        n = int(rows.shape[0])
        stride = int(rows.stride(0)) if n > 1 else nd
        if out is None:
            import torch

            out = torch.empty(lead + (k,), dtype=want, device=torch.device("cuda", dev))
        if not (hasattr(out, "is_cuda") and out.is_cuda and out.dtype == want):
            raise TypeError(f"out: expected a {want} CUDA tensor")
        if tuple(out.shape) != lead + (k,):
            raise ValueError(f"out: expected shape {lead + (k,)}, got {tuple(out.shape)}")
        _args.same_device("out", out, dev, "set")
        if out.dim() == 2:
            ostride = _args.row_stride("out", n, k, out.stride(), ValueError, _ROWS_UNIT, "out: the row stride must be at least {width}",
                                       check_empty=False)
        else:
            if not out.is_contiguous():
                raise ValueError("out: expected a contiguous tensor, or a 2-D tensor with contiguous rows")
            ostride = k
        raw, owner = _args.resolve_stream(stream, dev)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_fields_eval_points_device(self._h, c_void_p(rows.data_ptr()), stride, n, c_void_p(out.data_ptr()),
                                                              ostride, c_void_p(int(raw)), _args.eval_flags(no_alloc),
                                                              ctypes.byref(path))
        _lib.raise_for_status(st)
        if n:
            self._took_points()
        self._pending_streams[raw] = owner
        return out

    def eval_points(self, pts, out=None, **kwargs):
        """`eval_points_tensors` for a torch tensor, `eval_points_host` for a numpy array."""
        if _is_tensor(pts):
            return self.eval_points_tensors(pts, out, **kwargs)
        if kwargs:
            raise TypeError(f"eval_points on a host array takes no {sorted(kwargs)}")
        return self.eval_points_host(pts, out)

    # -- point-major values and Jacobian: (n, N) points in, (n, K) values and (n, K, N) Jacobian out ----
    def reserve_points_grad(self, npoints: int, nstreams: int = 1) -> None:
        """`reserve_points` for `eval_points_grad_*` (`interpn_hip_fields_reserve_points_grad`): a slice of the split path
        holds N + K (N + 1) arrays.  The fused kernel (sets with the fused table) needs none."""
        _lib.raise_for_status(_lib.load().interpn_hip_fields_reserve_points_grad(self._h, int(npoints), int(nstreams)))

    def eval_points_grad_host(self, pts, out=None, jac=None):
        """Every field and its gradient at the rows of a host array of shape `(n, N)` or `(..., N)` (synchronous;
        `interpn_hip_fields_eval_points_grad_host`): `(out, jac)` of shapes `(..., K)` and `(..., K, N)`; `out[i, f]` has the
        bits of `eval_points_host`, `jac[i, f, d]` those of `eval_grad_host(columns)[1][f, d, i]`.  `pts` is taken as
        `eval_points_host` takes it.  `out` and `jac` may be 2-D / 3-D views with any row stride >= K / K N and contiguous
        rows; a row's other elements are not touched.  On "Unrepresentable coordinate value" exactly the rows in front of
        the failing point are written, in both blocks."""
        _args.check_ndarray("pts", pts, self.dtype)
        nd, k = self._ndims, self.nfields
        rows, n, stride, lead = _args.point_rows("argument 'pts'", pts, nd)
        if out is None:
            out = np.zeros(lead + (k,), dtype=self.dtype)
        if jac is None:
            jac = np.zeros(lead + (k, nd), dtype=self.dtype)
        for name, a in (("out", out), ("jac", jac)):
            if not isinstance(a, np.ndarray) or a.dtype != self.dtype:
                raise TypeError(f"{name}: expected a numpy array of {self.dtype.name}")
        ostride = _args.point_results("out", out, lead, (k,), n)
        jstride = _args.point_results("jac", jac, lead, (k, nd), n)
        if not (out.flags.writeable and jac.flags.writeable):
            raise ValueError("out, jac: array is read-only")
        st = _lib.load().interpn_hip_fields_eval_points_grad_host(self._h, c_void_p(rows.ctypes.data), stride, n,
                                                                 c_void_p(out.ctypes.data), ostride, c_void_p(jac.ctypes.data), jstride)
        self._took_points()
        _lib.raise_for_status(st)
        return out, jac

    def eval_points_grad_tensors(self, pts, out=None, jac=None, stream=None, no_alloc: bool = False):
        """The same on a torch CUDA tensor (asynchronous on torch's current stream unless given;
        `interpn_hip_fields_eval_points_grad_device`): no `pts.T.contiguous()` in front and no permuted copy of the values
        or the Jacobian behind; everything stays on the device.  `pts`, `out` and `jac` must not overlap.  Sets with the
        fused table run one launch of `interpn::k_linear_fields_points_grad`, which allocates nothing and can be captured
        into a graph; `last_points_path` says which path ran; `finish()` synchronises and surfaces "Unrepresentable
        coordinate value"."""
        want = _args.torch_dtype(self.dtype)
        nd, k = self._ndims, self.nfields
        if not (hasattr(pts, "is_cuda") and pts.is_cuda and pts.dtype == want):
            raise TypeError(f"pts: expected a {want} CUDA tensor of shape (..., {nd})")
        dev = self.device()
        rows, n, stride, lead = _args.point_rows("pts", pts, nd)
        _args.same_device("pts", pts, dev, "set")
        if out is None or jac is None:
            import torch

            if out is None:
                out = torch.empty(lead + (k,), dtype=want, device=torch.device("cuda", dev))
            if jac is None:
                jac = torch.empty(lead + (k, nd), dtype=want, device=torch.device("cuda", dev))
        for name, a in (("out", out), ("jac", jac)):
            if not (hasattr(a, "is_cuda") and a.is_cuda and a.dtype == want):
                raise TypeError(f"{name}: expected a {want} CUDA tensor")
            _args.same_device(name, a, dev, "set")
        ostride = _args.point_results("out", out, lead, (k,), n)
        jstride = _args.point_results("jac", jac, lead, (k, nd), n)
        raw, owner = _args.resolve_stream(stream, dev)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_fields_eval_points_grad_device(self._h, c_void_p(rows.data_ptr()), stride, n,
                                                                   c_void_p(out.data_ptr()), ostride, c_void_p(jac.data_ptr()),
                                                                   jstride, c_void_p(int(raw)), _args.eval_flags(no_alloc),
                                                                   ctypes.byref(path))
        _lib.raise_for_status(st)
        if n:
            self._took_points()
        self._pending_streams[raw] = owner
        return out, jac

    def eval_points_grad(self, pts, out=None, jac=None, **kwargs):
        """`eval_points_grad_tensors` for a torch tensor, `eval_points_grad_host` for a numpy array."""
        if _is_tensor(pts):
            return self.eval_points_grad_tensors(pts, out, jac, **kwargs)
        if kwargs:
            raise TypeError(f"eval_points_grad on a host array takes no {sorted(kwargs)}")
        return self.eval_points_grad_host(pts, out, jac)

    # -- lattice evaluation: one coordinate vector per axis in, (K, *m) or (*m, K) values out ----
    @property
    def last_lattice_path(self):
        """"fused" (one launch of `interpn::k_lattice_fields_rows` for all fields) or "per_field" (K lattice evaluations
        through the K interpolators): what the most recent lattice evaluation did (None before any)."""
        return _lib.FIELDS_LATTICE_PATHS.get(self.get_option("last_lattice_path"))

    def reserve_lattice(self, axis_lens, nstreams: int = 1) -> None:
        """Pre-allocate the scratch of lattice evaluations with up to these axis lengths on up to `nstreams` concurrent
        streams (`interpn_hip_fields_reserve_lattice`); afterwards they work with `no_alloc=True` and under graph
        capture.  Per-field evaluations with `field_axis=-1` hold two blocks of the first field's interpolator at a time,
        of the four it can have: for them the guarantee covers two concurrent streams."""
        lens, n = _dims(axis_lens)
        _lib.raise_for_status(_lib.load().interpn_hip_fields_reserve_lattice(self._h, lens, n, int(nstreams)))

    def eval_lattice_host(self, axes, out=None, field_axis: int = 0) -> np.ndarray:
        """Every field on the lattice axes[0] x .. x axes[N-1] of host coordinate vectors (synchronous;
        `interpn_hip_fields_eval_lattice_host`): an array of shape `(K, *m)`, or `(*m, K)` with `field_axis=-1`, m =
        the vectors' lengths, whose field f has the bits of `Interpolator.eval_lattice_host` of that field alone.
        `out`, field-major: every field's block contiguous, any stride from field to field; fields-last: a C-contiguous
        array, or a 2-D `(prod(m), >= K)` view with contiguous rows.  On "Unrepresentable coordinate value" the
        AssertionError carries `first_bad_index` (C order over m) and exactly the results in front of it are written,
        for every field."""
        layout = _field_axis(field_axis)
        aptr, alen, naxes, _keep = _slice_of_slices("axes", axes, self.dtype)
        m = tuple(int(alen[i]) for i in range(naxes))
        k, item = self.nfields, self.dtype.itemsize
        if out is None:
            out = np.zeros((k,) + m if field_axis == 0 else m + (k,), dtype=self.dtype)
        _args.check_ndarray("out", out, self.dtype)
        if any(st % item for st in out.strides):
            raise ValueError("out: strides must be whole numbers of elements")
        stride = _lattice_out_stride(out.shape, [st // item for st in out.strides], k, m, layout, out.flags.c_contiguous)
        if not out.flags.writeable:
            raise ValueError("argument 'out': array is read-only")
        vp = _args.void_pp(aptr)
        bad = c_uint64(0)
        st = _lib.load().interpn_hip_fields_eval_lattice_host(self._h, vp, alen, naxes, c_void_p(out.ctypes.data), stride, layout,
                                                             ctypes.byref(bad))
        _args.raise_for_indexed_status(st, bad)
        return out

    def eval_lattice_tensors(self, axes, out=None, field_axis: int = 0, stream=None, no_alloc: bool = False):
        """The same on torch CUDA tensors (asynchronous on torch's current stream unless given;
        `interpn_hip_fields_eval_lattice_device`): `axes` are contiguous 1-D tensors of the set's dtype.  `out` must not
        overlap them.  `last_lattice_path` says which path ran; `finish()` synchronises and raises for a coordinate the
        reference cannot evaluate, with `first_bad_index` in C order over m (the same for every field)."""
        layout = _field_axis(field_axis)
        want = _args.torch_dtype(self.dtype)
        axes = list(axes)
        dev = self.device() if self._h is not None and self._h.value else -1
        _args.coord_tensors("axes", axes, want, dev, "set", same_length=False)
        m = tuple(int(t.numel()) for t in axes)
        k = self.nfields
        if out is None:
            import torch

            out = torch.empty((k,) + m if field_axis == 0 else m + (k,), dtype=want, device=torch.device("cuda", dev))
        if not (hasattr(out, "is_cuda") and out.is_cuda and out.dtype == want):
            raise TypeError(f"out: expected a {want} CUDA tensor")
        _args.same_device("out", out, dev, "set")
        stride = _lattice_out_stride(out.shape, out.stride(), k, m, layout, out.is_contiguous())
        raw, owner = _args.resolve_stream(stream, dev)
        n = len(axes)
        lens = (ctypes.c_size_t * max(n, 1))(*m)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_fields_eval_lattice_device(self._h, _args.ptr_array(t.data_ptr() for t in axes), lens, n,
                                                               c_void_p(out.data_ptr()), stride, layout, c_void_p(int(raw)),
                                                               _args.eval_flags(no_alloc), ctypes.byref(path))
        _lib.raise_for_status(st)
        self._pending_streams[raw] = owner
        return out

    def eval_lattice(self, axes, out=None, **kwargs):
        """`eval_lattice_tensors` for torch tensors, `eval_lattice_host` for numpy arrays (by the type of `axes[0]`)."""
        axes = list(axes)
        if axes and _is_tensor(axes[0]):
            return self.eval_lattice_tensors(axes, out, **kwargs)
        extra = sorted(set(kwargs) - {"field_axis"})
        if extra:
            raise TypeError(f"eval_lattice on host arrays takes no {extra}")
        return self.eval_lattice_host(axes, out, **kwargs)

    # -- lattice values and Jacobian: (K, *m) values and (K, N, *m) Jacobian, or (*m, K) and (*m, K, N) ----
    def reserve_lattice_grad(self, axis_lens, nstreams: int = 1) -> None:
        """`reserve_lattice` for `eval_lattice_grad_*` (`interpn_hip_fields_reserve_lattice_grad`): the per-field slice holds
        K (N + 1) rows.  The same limit of two concurrent streams for per-field evaluations with `field_axis=-1`."""
        lens, n = _dims(axis_lens)
        _lib.raise_for_status(_lib.load().interpn_hip_fields_reserve_lattice_grad(self._h, lens, n, int(nstreams)))

    def _lattice_grad_shapes(self, m, field_axis):
        k, nd = self.nfields, self._ndims
        return ((k,) + m, (k, nd) + m) if field_axis == 0 else (m + (k,), m + (k, nd))

    def eval_lattice_grad_host(self, axes, out=None, jac=None, field_axis: int = 0):
        """Every field and its gradient on the lattice axes[0] x .. x axes[N-1] of host coordinate vectors (synchronous;
        `interpn_hip_fields_eval_lattice_grad_host`): `(out, jac)` of shapes `(K, *m)` and `(K, N, *m)`, or `(*m, K)` and
        `(*m, K, N)` with `field_axis=-1`.  `out` has the bits of `eval_lattice_host`; `jac[f, d]` (`jac[..., f, d]`) has
        the bits of `Interpolator.eval_lattice_grad_host(axes)[1][d]` of field f alone.  `out` as for `eval_lattice_host`;
        `jac`, field-major: every (f, d) block contiguous, one stride between the K N blocks; fields-last: C-contiguous, or
        a `(prod(m), K, N)` view with contiguous rows.  On "Unrepresentable coordinate value" the AssertionError carries
        `first_bad_index` (C order over m) and exactly the results in front of it are written, in both arrays."""
        layout = _field_axis(field_axis)
        aptr, alen, naxes, _keep = _slice_of_slices("axes", axes, self.dtype)
        m = tuple(int(alen[i]) for i in range(naxes))
        k, nd, item = self.nfields, self._ndims, self.dtype.itemsize
        oshape, jshape = self._lattice_grad_shapes(m, field_axis)
        if out is None:
            out = np.zeros(oshape, dtype=self.dtype)
        if jac is None:
            jac = np.zeros(jshape, dtype=self.dtype)
        _args.check_ndarray("out", out, self.dtype)
        _args.check_ndarray("jac", jac, self.dtype)
        if any(st % item for st in out.strides + jac.strides):
            raise ValueError("out, jac: strides must be whole numbers of elements")
        stride = _lattice_out_stride(out.shape, [st // item for st in out.strides], k, m, layout, out.flags.c_contiguous)
        jstride = _lattice_jac_stride(jac.shape, [st // item for st in jac.strides], k, nd, m, layout, jac.flags.c_contiguous)
        if not (out.flags.writeable and jac.flags.writeable):
            raise ValueError("out, jac: array is read-only")
        bad = c_uint64(0)
        st = _lib.load().interpn_hip_fields_eval_lattice_grad_host(self._h, _args.void_pp(aptr), alen, naxes, c_void_p(out.ctypes.data),
                                                                  stride, c_void_p(jac.ctypes.data), jstride, layout, ctypes.byref(bad))
        _args.raise_for_indexed_status(st, bad)
        return out, jac

    def eval_lattice_grad_tensors(self, axes, out=None, jac=None, field_axis: int = 0, stream=None, no_alloc: bool = False):
        """The same on torch CUDA tensors (asynchronous on torch's current stream unless given;
        `interpn_hip_fields_eval_lattice_grad_device`): `axes` are contiguous 1-D tensors of the set's dtype; `out` and `jac`
        must not overlap them or each other.  With `field_axis=-1` the kernel writes `(*m, K)` and `(*m, K, N)` itself: no
        stack and no permuted copy behind K single-field calls.  `last_lattice_path` says which path ran; `finish()`
        synchronises and raises for a coordinate the reference cannot evaluate."""
        layout = _field_axis(field_axis)
        want = _args.torch_dtype(self.dtype)
        axes = list(axes)
        dev = self.device() if self._h is not None and self._h.value else -1
        _args.coord_tensors("axes", axes, want, dev, "set", same_length=False)
        m = tuple(int(t.numel()) for t in axes)
        k, nd = self.nfields, self._ndims
        oshape, jshape = self._lattice_grad_shapes(m, field_axis)
        if out is None or jac is None:
            import torch

            if out is None:
                out = torch.empty(oshape, dtype=want, device=torch.device("cuda", dev))
            if jac is None:
                jac = torch.empty(jshape, dtype=want, device=torch.device("cuda", dev))
        for name, a in (("out", out), ("jac", jac)):
            if not (hasattr(a, "is_cuda") and a.is_cuda and a.dtype == want):
                raise TypeError(f"{name}: expected a {want} CUDA tensor")
            _args.same_device(name, a, dev, "set")
        stride = _lattice_out_stride(out.shape, out.stride(), k, m, layout, out.is_contiguous())
        jstride = _lattice_jac_stride(jac.shape, jac.stride(), k, nd, m, layout, jac.is_contiguous())
        raw, owner = _args.resolve_stream(stream, dev)
        n = len(axes)
        lens = (ctypes.c_size_t * max(n, 1))(*m)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_fields_eval_lattice_grad_device(
            self._h, _args.ptr_array(t.data_ptr() for t in axes), lens, n, c_void_p(out.data_ptr()), stride, c_void_p(jac.data_ptr()),
            jstride, layout, c_void_p(int(raw)), _args.eval_flags(no_alloc), ctypes.byref(path))
        _lib.raise_for_status(st)
        self._pending_streams[raw] = owner
        return out, jac

    def eval_lattice_grad(self, axes, out=None, jac=None, **kwargs):
        """`eval_lattice_grad_tensors` for torch tensors, `eval_lattice_grad_host` for numpy arrays (by the type of
        `axes[0]`)."""
        axes = list(axes)
        if axes and _is_tensor(axes[0]):
            return self.eval_lattice_grad_tensors(axes, out, jac, **kwargs)
        extra = sorted(set(kwargs) - {"field_axis"})
        if extra:
            raise TypeError(f"eval_lattice_grad on host arrays takes no {extra}")
        return self.eval_lattice_grad_host(axes, out, jac, **kwargs)

    def finish(self, stream=None) -> None:
        """Wait for the evaluations enqueued since the last finish; AssertionError("Unrepresentable coordinate
        value") with `.first_bad_index` if a point could not be evaluated (the same index for every field)."""
        raws = [_args.resolve_stream(stream, None)[0]] if stream is not None else list(self._pending_streams) or [0]
        _args.finish_streams(_lib.load().interpn_hip_fields_finish, self._h, raws, self._pending_streams)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.load().interpn_hip_fields_destroy(self._h)
            self._h = c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fields_layout(dtype, dims, nfields: int):
    """(fields per 128-byte line, lines per cell, table bytes) of the fused table (`interpn_hip_fields_layout`);
    needs no device.  ValueError outside the fused kernel's coverage (N = 2, 3)."""
    d, nd = _dims(dims)
    per_line, lines, nbytes = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.raise_for_status(_lib.load().interpn_hip_fields_layout(np.dtype(dtype).itemsize, nd, d, int(nfields), ctypes.byref(per_line),
                                                                ctypes.byref(lines), ctypes.byref(nbytes)))
    return int(per_line.value), int(lines.value), int(nbytes.value)


def fields_lattice_plan(dtype, method: str, dims, axis_lens, nfields: int, field_axis: int = 0):
    """(path, group, lds_bytes, npoints): the path ("fused" / "per_field") a set of `nfields` fields takes in automatic mode
    on a lattice of `axis_lens` coordinates per axis of a grid of `dims`, the fields per pass G and the LDS bytes of the
    fused kernel's workgroup (both 0 on the per-field path), and the point count (`interpn_hip_fields_lattice_plan`; needs
    no device)."""
    layout = _field_axis(field_axis)
    d, nd = _dims(dims)
    m, nm = _dims(axis_lens)
    if nd != nm:
        raise ValueError(f"axis_lens: expected {nd} lengths, got {nm}")
    path, group, lds, npts = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    st = _lib.load().interpn_hip_fields_lattice_plan(np.dtype(dtype).itemsize, _lib.METHODS[method], nd, d, m, int(nfields), layout,
                                                     ctypes.byref(path), ctypes.byref(group), ctypes.byref(lds), ctypes.byref(npts))
    _lib.raise_for_status(st)
    return _lib.FIELDS_LATTICE_PATHS[path.value], int(group.value), int(lds.value), int(npts.value)


def interpn_fields_lattice(axes, grids, vals, *, method="linear", field_axis: int = 0, out=None,
                           linearize_extrapolation: bool = True, assume_regular: bool = False):
    """`interpn_lattice()` for K fields on one grid: every field on the lattice axes[0] x .. x axes[N-1] in one pass.  The
    rules are those of `interpn_lattice` and `interpn_fields` (inputs ravelled, dtype from `vals`, exact-spacing regularity
    test, host arrays or torch CUDA tensors as coordinate vectors).

    `vals` has shape (K, *dims) and the result (K, *m), m = the vectors' lengths; with `field_axis=-1` the channel-last
    layout: `vals` (*dims, K), result (*m, K) — an image resize when N = 2."""
    _field_axis(field_axis)
    _setup.check_method(method)
    axes = list(axes)
    dtype, grids, k, nper = _setup.grids_and_fields(grids, vals, field_axis, naxes=len(axes))
    on_device = bool(axes) and _setup.is_cuda_tensor(axes[0])
    m = tuple(int(a.numel()) if _is_tensor(a) else int(np.asarray(a).size) for a in axes)
    rshape = (k,) + m if field_axis == 0 else m + (k,)
    if out is not None and tuple(out.shape) != rshape:
        raise ValueError(f"out: expected shape {rshape}, got {tuple(out.shape)}")
    device = _setup.device_index(axes[0]) if on_device else -1
    axes = _setup.flat_coords(axes, on_device)
    vals = _setup.field_major(vals, k, nper, field_axis == -1, on_device)
    fs = _setup.create(Fields, method, grids, _setup.regular_spec(grids, dtype, assume_regular), vals, dtype, device,
                       linearize_extrapolation=linearize_extrapolation)
    try:
        if on_device:
            res = fs.eval_lattice_tensors(axes, out, field_axis=field_axis)
            fs.finish()
        else:
            res = fs.eval_lattice_host(axes, out, field_axis=field_axis)
    finally:
        fs.close()
    return res


def fields_lattice_grad_plan(dtype, method: str, dims, axis_lens, nfields: int, field_axis: int = 0):
    """`fields_lattice_plan` for a value-and-Jacobian call (`interpn_hip_fields_lattice_grad_plan`; needs no device): a
    wave of the fused kernel keeps G x L lines (multilinear L = N + 1, multicubic L = N) and, for `field_axis=-1`, a tile of
    (G (N + 1)) | 1 elements per point.  `method` "linear" or "cubic"."""
    layout = _field_axis(field_axis)
    d, nd = _dims(dims)
    m, nm = _dims(axis_lens)
    if nd != nm:
        raise ValueError(f"axis_lens: expected {nd} lengths, got {nm}")
    path, group, lds, npts = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    st = _lib.load().interpn_hip_fields_lattice_grad_plan(np.dtype(dtype).itemsize, _lib.METHODS[method], nd, d, m, int(nfields), layout,
                                                          ctypes.byref(path), ctypes.byref(group), ctypes.byref(lds), ctypes.byref(npts))
    _lib.raise_for_status(st)
    return _lib.FIELDS_LATTICE_PATHS[path.value], int(group.value), int(lds.value), int(npts.value)


def interpn_fields_lattice_grad(axes, grids, vals, *, method="linear", field_axis: int = 0, linearize_extrapolation: bool = True,
                                assume_regular: bool = False):
    """`interpn_fields_lattice()` with the Jacobian: every field and its derivative with respect to every coordinate on the
    lattice axes[0] x .. x axes[N-1], one pass (`Fields.eval_lattice_grad`).  The rules are those of `interpn_fields_lattice`;
    `method` is "linear" or "cubic" ("nearest" has no gradient: the library's "unsupported" error).

    Returns `(val, jac)`.  `vals` (K, *dims): `val` (K, *m), `jac` (K, N, *m), `jac[f, d]` the derivative of field f with
    respect to coordinate d, with the bits of `interpn_lattice_grad` of field f.  With `field_axis=-1` the channel-last
    layout, written by the kernel: `vals` (*dims, K), `val` (*m, K), `jac` (*m, K, N) — the Jacobian of a displacement field
    on a finer mesh, the per-channel gradients of a resized image."""
    _field_axis(field_axis)
    _setup.check_method(method)
    axes = list(axes)
    dtype, grids, k, nper = _setup.grids_and_fields(grids, vals, field_axis, naxes=len(axes))
    on_device = bool(axes) and _setup.is_cuda_tensor(axes[0])
    device = _setup.device_index(axes[0]) if on_device else -1
    axes = _setup.flat_coords(axes, on_device)
    vals = _setup.field_major(vals, k, nper, field_axis == -1, on_device)
    fs = _setup.create(Fields, method, grids, _setup.regular_spec(grids, dtype, assume_regular), vals, dtype, device,
                       linearize_extrapolation=linearize_extrapolation)
    try:
        if on_device:
            res = fs.eval_lattice_grad_tensors(axes, field_axis=field_axis)
            fs.finish()
        else:
            res = fs.eval_lattice_grad_host(axes, field_axis=field_axis)
    finally:
        fs.close()
    return res


def _points_of_fields(obs, grids, vals, method, field_axis):
    """What `interpn_fields` and `interpn_fields_grad` check and work out before they differ:
    `(dtype, grids, k, nper, on_device, pshape)`."""
    _field_axis(field_axis)
    _setup.check_method(method)
    dtype, grids, k, nper = _setup.grids_and_fields(grids, vals, field_axis)
    on_device = bool(len(obs)) and _setup.is_cuda_tensor(obs[0])
    pshape = tuple(obs[0].shape) if len(obs) else (0,)
    return dtype, grids, k, nper, on_device, pshape


def interpn_fields(obs, grids, vals, *, method="linear", field_axis: int = 0, out=None, linearize_extrapolation: bool = True,
                   assume_regular: bool = False, check_bounds: bool = False, bounds_atol: float = 1e-8):
    """`interpn()` for K fields on one grid: the same rules (ravelled inputs, dtype from `vals`, exact-spacing
    regularity test, host arrays or torch CUDA tensors as points), one pass over the points.

    `vals` has shape (K, *dims) and the result (K, *obs[0].shape); with `field_axis=-1` the scipy layout:
    `vals` (*dims, K), result (*obs[0].shape, K)."""
    dtype, grids, k, nper, on_device, pshape = _points_of_fields(obs, grids, vals, method, field_axis)
    rshape = (k,) + pshape if field_axis == 0 else pshape + (k,)
    if out is not None and tuple(out.shape) != rshape:
        raise ValueError(f"out: expected shape {rshape}, got {tuple(out.shape)}")
    device = _setup.device_index(obs[0]) if on_device else -1
    obs_flat = _setup.flat_coords(obs, on_device)
    vals = _setup.field_major(vals, k, nper, field_axis == -1, on_device)
    spec = _setup.regular_spec(grids, dtype, assume_regular)
    if check_bounds and not on_device:
        _setup.check_host_bounds(grids, spec, dtype, obs_flat, bounds_atol)
    fs = _setup.create(Fields, method, grids, spec, vals, dtype, device, linearize_extrapolation=linearize_extrapolation)
    try:
        if on_device:
            if check_bounds:
                _setup.check_field_device_bounds(method, grids, spec, vals, dtype, device, obs_flat, bounds_atol)
            direct = out is not None and field_axis == 0 and out.is_contiguous()
            res = fs.eval_tensors(obs_flat, out.reshape(k, -1) if direct else None)
            fs.finish()
        else:
            direct = out is not None and field_axis == 0 and out.flags.c_contiguous and out.dtype == dtype
            res = fs.eval_host(obs_flat, out.reshape(k, -1) if direct else None)
    finally:
        fs.close()
    if direct:
        return out
    res = res.reshape((k,) + pshape)
    if field_axis == -1:
        res = res.permute(*range(1, len(rshape)), 0) if on_device else np.moveaxis(res, 0, -1)
    if out is not None:
        if on_device:
            out.copy_(res)
        else:
            out[...] = res
        return out
    return res.contiguous() if on_device else np.ascontiguousarray(res)


def interpn_fields_grad(obs, grids, vals, *, method="linear", field_axis: int = 0, linearize_extrapolation: bool = True,
                        assume_regular: bool = False):
    """`interpn_fields()` with the Jacobian: every field and its derivative with respect to every coordinate at the
    observation points, one pass over the points where the set has the fused kernel (`Fields.eval_grad`).  The rules are
    those of `interpn_fields` (ravelled inputs, dtype from `vals`, exact-spacing regularity test, host arrays or torch CUDA
    tensors as points); `method` is "linear" or "cubic" ("nearest" has no gradient: the library's "unsupported" error).

    Returns `(out, jac)`.  `vals` (K, *dims): `out` (K, *obs[0].shape), `jac` (K, N, *obs[0].shape), `jac[f, d]` the
    derivative of field f with respect to coordinate d, with the bits of `interpn_grad` of field f.  With `field_axis=-1`
    the scipy layout: `vals` (*dims, K), `out` (*obs[0].shape, K), `jac` (*obs[0].shape, K, N) — permuted copies made here,
    not by the kernel."""
    dtype, grids, k, nper, on_device, pshape = _points_of_fields(obs, grids, vals, method, field_axis)
    nd = len(grids)
    device = _setup.device_index(obs[0]) if on_device else -1
    obs_flat = _setup.flat_coords(obs, on_device)
    vals = _setup.field_major(vals, k, nper, field_axis == -1, on_device)
    fs = _setup.create(Fields, method, grids, _setup.regular_spec(grids, dtype, assume_regular), vals, dtype, device,
                       linearize_extrapolation=linearize_extrapolation)
    try:
        if on_device:
            out, jac = fs.eval_grad_tensors(obs_flat)
            fs.finish()
        else:
            out, jac = fs.eval_grad_host(obs_flat)
    finally:
        fs.close()
    out = out.reshape((k,) + pshape)
    jac = jac.reshape((k, nd) + pshape)
    if field_axis == 0:
        return out, jac
    np_ = len(pshape)
    if on_device:
        return (out.permute(*range(1, np_ + 1), 0).contiguous(), jac.permute(*range(2, np_ + 2), 0, 1).contiguous())
    return (np.ascontiguousarray(np.moveaxis(out, 0, -1)), np.ascontiguousarray(np.moveaxis(np.moveaxis(jac, 0, -1), 0, -1)))


def _xi_of_fields(xi, grids, vals, method, out):
    """What `interpn_fields_points` and `interpn_fields_points_grad` check and work out before they differ:
    `(dtype, grids, nd, k, nper, on_device)`."""
    _setup.check_method(method)
    dtype = _setup.field_values_dtype(vals, "a trailing field axis")
    if not (isinstance(xi, np.ndarray) or _is_tensor(xi)):
        raise TypeError("xi: expected a numpy array or a torch tensor of shape (..., N)")
    grids = _setup.canonical_grids(grids, dtype)
    nd = len(grids)
    if len(vals.shape) != nd + 1:
        raise ValueError(f"vals: expected shape (*dims, K) for {nd} grids, got {tuple(vals.shape)}")
    if len(xi.shape) < 1 or int(xi.shape[-1]) != nd:
        raise ValueError(f"xi: expected shape (..., {nd}), got {tuple(xi.shape)}")
    nper = int(np.prod([g.size for g in grids], dtype=object))
    k = int(vals.shape[-1])
    if tuple(int(v) for v in vals.shape[:-1]) != tuple(g.size for g in grids) or k < 1:
        raise _setup.value_count_error(k, nper, grids, vals)
    on_device = _setup.is_cuda_tensor(xi)
    want = str(xi.dtype).rsplit(".", 1)[-1]
    if want != dtype.name:
        raise TypeError(f"xi: expected dtype {dtype.name} (that of vals), got {want}")
    rshape = tuple(int(v) for v in xi.shape[:-1]) + (k,)
    if out is not None and tuple(out.shape) != rshape:
        raise ValueError(f"out: expected shape {rshape}, got {tuple(out.shape)}")
    if _is_tensor(xi) and not on_device:
        raise TypeError("xi: expected a numpy array or a torch CUDA tensor")
    return dtype, grids, nd, k, nper, on_device


def interpn_fields_points(xi, grids, vals, *, method="linear", out=None, linearize_extrapolation: bool = True,
                          assume_regular: bool = False, check_bounds: bool = False, bounds_atol: float = 1e-8):
    """scipy's `interpn(points, values, xi)` with trailing value dimensions: `vals` of shape (*dims, K), `xi` of shape
    (..., N) — a numpy array or a torch CUDA tensor — and a result of shape (..., K).  The rules are those of
    `interpn_fields` (dtype from `vals`, exact-spacing regularity test); the points and the result keep their layout
    (`Fields.eval_points`), and the value table is re-laid field-major once, as part of setting the fields up."""
    dtype, grids, nd, k, nper, on_device = _xi_of_fields(xi, grids, vals, method, out)
    device = _setup.device_index(xi) if on_device else -1
    vals = _setup.field_major(vals, k, nper, True, on_device)
    spec = _setup.regular_spec(grids, dtype, assume_regular)
    if check_bounds and not on_device:
        _setup.check_host_bounds(grids, spec, dtype, [np.ascontiguousarray(xi[..., d].ravel()) for d in range(nd)], bounds_atol)
    fs = _setup.create(Fields, method, grids, spec, vals, dtype, device, linearize_extrapolation=linearize_extrapolation)
    try:
        if on_device:
            if check_bounds:
                cols = [xi[..., d].reshape(-1).contiguous() for d in range(nd)]
                _setup.check_field_device_bounds(method, grids, spec, vals, dtype, device, cols, bounds_atol)
            res = fs.eval_points_tensors(xi, out)
            fs.finish()
        else:
            res = fs.eval_points_host(xi, out)
    finally:
        fs.close()
    return res


def interpn_fields_points_grad(xi, grids, vals, *, method="linear", linearize_extrapolation: bool = True,
                               assume_regular: bool = False):
    """`interpn_fields_points()` with the Jacobian: `vals` of shape (*dims, K), `xi` of shape (..., N) — a numpy array or a
    torch CUDA tensor — and `(out, jac)` of shapes (..., K) and (..., K, N), `jac[..., f, d]` the derivative of field f with
    respect to coordinate d, with the bits of `interpn_fields_grad` on the columns.  The points and both results keep their
    layout (`Fields.eval_points_grad`): one pass where the set has the fused kernel.  `method` is "linear" or "cubic"
    ("nearest" has no gradient: the library's "unsupported" error)."""
    dtype, grids, nd, k, nper, on_device = _xi_of_fields(xi, grids, vals, method, None)
    device = _setup.device_index(xi) if on_device else -1
    vals = _setup.field_major(vals, k, nper, True, on_device)
    fs = _setup.create(Fields, method, grids, _setup.regular_spec(grids, dtype, assume_regular), vals, dtype, device,
                       linearize_extrapolation=linearize_extrapolation)
    try:
        if on_device:
            res = fs.eval_points_grad_tensors(xi)
            fs.finish()
        else:
            res = fs.eval_points_grad_host(xi)
    finally:
        fs.close()
    return res
