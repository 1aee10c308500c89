"""Field sets: K value grids ("fields") on one grid, evaluated at the same points in one pass
(`interpn_hip_fields_*` of include/interpn_hip.h) — equation-of-state tables, vector fields, colour
channels, scipy's RegularGridInterpolator with trailing value dimensions.

`Fields` is the persistent form (the counterpart of `Interpolator`), `interpn_fields()` the one-call
form (the counterpart of `interpn()`).  Row f of every result is bit-identical to what the single
interpolator of field f returns.
"""

from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_uint64, c_void_p

import numpy as np

from . import _lib
from .raw import _check_arr, _dims, _slice_of_slices


def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


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

    # -- construction ---------------------------------------------------------------------
    @classmethod
    def regular(cls, method: str, dims, starts, steps, vals, linearize_extrapolation: bool = False, device: int = -1,
                dtype=None, fma=None) -> "Fields":
        from .handle import Interpolator

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
        from .handle import Interpolator

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

    # -- evaluation -----------------------------------------------------------------------
    def eval_host(self, obs, out=None) -> np.ndarray:
        """Every field at host points (synchronous): a (K, n) array.  `out` may be a (K, n) array whose rows are
        contiguous (a row stride beyond n is fine: a view of a wider array)."""
        optr, olen, nobs, _keep = _slice_of_slices("obs", obs, self.dtype)
        n = int(olen[0]) if nobs else 0
        if out is None:
            out = np.zeros((self.nfields, n), dtype=self.dtype)
        if not isinstance(out, np.ndarray) or out.dtype != self.dtype or out.ndim != 2 or out.shape != (self.nfields, n):
            raise ValueError(f"out: expected a ({self.nfields}, {n}) array of {self.dtype.name}")
        item = self.dtype.itemsize
        if n and (out.strides[1] != item or out.strides[0] % item or out.strides[0] < n * item):
            raise ValueError("out: rows must be contiguous")
        if not out.flags.writeable:
            raise ValueError("out: array is read-only")
        vp = (c_void_p * max(nobs, 1))()
        for i in range(nobs):
            vp[i] = ctypes.cast(optr[i], c_void_p)
        stride = out.strides[0] // item if n else 0
        st = _lib.load().interpn_hip_fields_eval_host(self._h, vp, olen, nobs, c_void_p(out.ctypes.data), max(stride, n), n)
        self._took()
        _lib.raise_for_status(st)
        return out

    def eval_device_ptrs(self, obs_ptrs, out_ptr: int, out_stride: int, npoints: int, stream: int = 0,
                         no_alloc: bool = False) -> str:
        """Enqueue one evaluation on device buffers given as raw addresses; returns the path taken."""
        n = len(obs_ptrs)
        vp = (c_void_p * max(n, 1))()
        for i, p in enumerate(obs_ptrs):
            vp[i] = c_void_p(int(p))
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_fields_eval_device(self._h, vp, n, c_void_p(int(out_ptr)), int(out_stride), int(npoints),
                                                        c_void_p(int(stream)), _lib.EVAL_NO_ALLOC if no_alloc else 0,
                                                        ctypes.byref(path))
        _lib.raise_for_status(st)
        self.last_path = "fused" if path.value == _lib.FIELDS_PATH_FUSED else "per_field"
        self._pending_streams.setdefault(int(stream), None)
        return self.last_path

    def eval_tensors(self, obs, out=None, stream=None, no_alloc: bool = False):
        """Every field at points held in torch CUDA tensors (asynchronous on torch's current stream unless given):
        a (K, n) tensor.  `out` may be a (K, n) tensor with contiguous rows.  Call `finish()` to synchronise and
        surface "Unrepresentable coordinate value"."""
        import torch

        want = torch.float64 if self.dtype == np.float64 else torch.float32
        obs = list(obs)
        dev = self.device()
        for i, t in enumerate(obs):
            if not (t.is_cuda and t.is_contiguous() and t.dim() == 1 and t.dtype == want):
                raise TypeError(f"obs[{i}]: expected a contiguous 1-D {want} CUDA tensor")
            if t.device.index not in (None, dev):
                raise ValueError(f"obs[{i}] is on {t.device} but this set lives on cuda:{dev}")
        n = obs[0].numel() if obs else 0
        for t in obs:
            if t.numel() != n:
                raise AssertionError("Dimension mismatch")
        if out is None:
            out = torch.empty((self.nfields, n), dtype=want, device=torch.device("cuda", dev))
        elif not (out.is_cuda and out.dim() == 2 and out.dtype == want and tuple(out.shape) == (self.nfields, n)):
            raise TypeError(f"out: expected a ({self.nfields}, {n}) {want} CUDA tensor")
        elif n and (out.stride(1) != 1 or out.stride(0) < n):
            raise ValueError("out: rows must be contiguous")
        owner = torch.cuda.current_stream(dev) if stream is None else stream
        raw = owner.cuda_stream if hasattr(owner, "cuda_stream") else int(owner)
        self.eval_device_ptrs([t.data_ptr() for t in obs], out.data_ptr(), max(out.stride(0), n) if n else 0, n, raw, no_alloc)
        self._pending_streams[raw] = owner if hasattr(owner, "cuda_stream") else None
        return out

    def finish(self, stream=None) -> None:
        """Wait for the evaluations enqueued since the last finish; AssertionError("Unrepresentable coordinate
        value") with `.first_bad_index` if a point could not be evaluated (the same index for every field)."""
        lib = _lib.load()
        if stream is not None:
            raws = [stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)]
        else:
            raws = list(self._pending_streams) or [0]
        first_bad, bad_status, status = None, _lib.ERR_UNREPRESENTABLE, _lib.OK
        for raw in raws:
            bad = c_uint64(0)
            st = lib.interpn_hip_fields_finish(self._h, c_void_p(int(raw)), ctypes.byref(bad))
            self._pending_streams.pop(raw, None)
            if st in _lib.UNREPRESENTABLE:
                bad_status = st
                first_bad = bad.value if first_bad is None else min(first_bad, bad.value)
            elif st != _lib.OK and status == _lib.OK:
                status = st
        _lib.raise_for_status(status)
        if first_bad is not None:
            err = AssertionError(_lib.strerror(bad_status))
            err.first_bad_index = first_bad
            raise err

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


def interpn_fields(obs, grids, vals, *, method="linear", field_axis: int = 0, out=None, linearize_extrapolation: bool = True,
                   assume_regular: bool = False, check_bounds: bool = False, bounds_atol: float = 1e-8):
    """`interpn()` for K fields on one grid: the same rules (ravelled inputs, dtype from `vals`, exact-spacing
    regularity test, host arrays or torch CUDA tensors as points), one pass over the points.

    `vals` has shape (K, *dims) and the result (K, *obs[0].shape); with `field_axis=-1` the scipy layout:
    `vals` (*dims, K), result (*obs[0].shape, K)."""
    from . import _check_regular, _is_cuda_tensor, raw

    if field_axis not in (0, -1):
        raise ValueError("field_axis: expected 0 (fields first) or -1 (fields last)")
    if method not in ("linear", "cubic", "nearest"):
        raise ValueError(f"Unsupported interpolation configuration: {method}")
    if not (isinstance(vals, np.ndarray) or _is_tensor(vals)):
        raise TypeError("vals: expected a numpy array or a torch tensor with a field axis")
    assert str(vals.dtype).endswith(("float64", "float32")), "`interpn` defined only for float32 and float64 data"
    dtype = np.dtype(np.float64 if str(vals.dtype).endswith("64") else np.float32)
    if len(vals.shape) < 2:
        raise ValueError("vals: expected a field axis besides the grid's values")
    grids = [np.ascontiguousarray(np.asarray(g).ravel()).astype(dtype, copy=False) for g in grids]
    nper = int(np.prod([g.size for g in grids], dtype=object))
    k = int(vals.shape[field_axis])
    if k * nper != int(np.prod(tuple(vals.shape), dtype=object)):
        raise ValueError(f"vals: expected {k} x {nper} values for grids of {[g.size for g in grids]}, got shape {tuple(vals.shape)}")
    if field_axis == -1:  # (*dims, K) -> (K, prod(dims))
        vals = vals.reshape(nper, k).T
    vals = (vals.contiguous() if _is_tensor(vals) else np.ascontiguousarray(vals)).reshape(k, nper)

    on_device = bool(len(obs)) and _is_cuda_tensor(obs[0])
    pshape = tuple(obs[0].shape) if len(obs) else (0,)
    rshape = (k,) + pshape if field_axis == 0 else pshape + (k,)
    if out is not None and tuple(out.shape) != rshape:
        raise ValueError(f"out: expected shape {rshape}, got {tuple(out.shape)}")
    regular = assume_regular or _check_regular(grids)
    device = -1
    if on_device:
        import torch

        device = obs[0].device.index if obs[0].device.index is not None else torch.cuda.current_device()
        obs_flat = [x.reshape(-1).contiguous() for x in obs]
    else:
        if _is_tensor(vals):
            vals = vals.cpu().numpy()
        obs_flat = [np.ascontiguousarray(np.asarray(x).ravel()) for x in obs]
    if regular:
        dims = [g.size for g in grids]
        starts = np.array([g[0] for g in grids], dtype=dtype)
        steps = np.array([g[1] - g[0] for g in grids], dtype=dtype)
    sfx = "f64" if dtype == np.float64 else "f32"
    if check_bounds and not on_device:
        outb = np.zeros(len(grids), dtype=bool)
        if regular:
            getattr(raw, f"check_bounds_regular_{sfx}")(dims, starts, steps, obs_flat, bounds_atol, outb)
        else:
            getattr(raw, f"check_bounds_rectilinear_{sfx}")(grids, obs_flat, bounds_atol, outb)
        if any(outb):
            raise ValueError("Observation points violate interpolator bounds")
    if regular:
        fs = Fields.regular(method, dims, starts, steps, vals, linearize_extrapolation=linearize_extrapolation, device=device,
                            dtype=dtype)
    else:
        fs = Fields.rectilinear(method, grids, vals, linearize_extrapolation=linearize_extrapolation, device=device, dtype=dtype)
    try:
        if on_device:
            if check_bounds:  # the bounds are the grid's: any one field's interpolator checks them on the device
                from .handle import Interpolator

                one = (Interpolator.regular(method, dims, starts, steps, vals[0], device=device, dtype=dtype) if regular
                       else Interpolator.rectilinear(method, grids, vals[0], device=device, dtype=dtype))
                try:
                    if one.check_bounds_tensors(obs_flat, bounds_atol).any():
                        raise ValueError("Observation points violate interpolator bounds")
                finally:
                    one.close()
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
