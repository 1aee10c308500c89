"""Persistent, device-resident interpolators over the handle API of include/interpn_hip.h.

`Interpolator` is the counterpart of the reference's interpolator structs
(`MultilinearRegular::new(..).interp(obs, out)`, src/multilinear/regular.rs:225-283 and the
three siblings) with the grid kept in HBM between evaluations.  Observation points may be host
numpy arrays (`eval_host`) or device buffers (`eval_device`, e.g. torch tensors on the GPU —
torch is only plumbing for device memory and streams here).
"""

from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_float, c_size_t, c_uint64, c_void_p

import numpy as np

from . import _args, _lib
from .raw import _check_arr, _dims, _slice_of_slices


class Interpolator:
    def __init__(self, handle: int, dtype, ndims: int, keepalive=None):
        self._h = c_void_p(handle)
        self.dtype = np.dtype(dtype)
        self._ndims = ndims
        self._keepalive = keepalive  # e.g. a torch tensor whose storage the handle borrows
        # Streams that evaluations were enqueued on since the last finish(): raw handle -> the
        # object that owns it (a torch Stream kept alive here; None for a caller-supplied integer).
        self._pending_streams = {}
        self.method = None           # "linear" | "cubic" | "nearest" for handles made by regular() / rectilinear(); kept by replicate()
        self.last_path = None        # "in_place" | "binned" | "sweep": what the most recent device evaluation did
        self.last_path_reason = ""   # why a handle that can sort its points did not

    # -- construction ---------------------------------------------------------------------
    @staticmethod
    def _vals_arg(vals, dtype):
        """Return (void* address, nvals, mem kind, keepalive) for a numpy array or a torch tensor."""
        if isinstance(vals, np.ndarray):
            v = _check_arr("vals", vals, dtype)
            return v.ctypes.data_as(c_void_p), v.size, _lib.MEM_HOST, v
        # torch tensor (duck-typed so that torch stays an optional import)
        if hasattr(vals, "data_ptr") and hasattr(vals, "is_cuda"):
            if not vals.is_contiguous() or vals.dim() != 1:
                raise ValueError("argument 'vals': expected a contiguous 1-D tensor")
            want = "torch.float64" if dtype == np.float64 else "torch.float32"
            if str(vals.dtype) != want:
                raise TypeError(f"argument 'vals': expected {want}, got {vals.dtype}")
            mem = _lib.MEM_DEVICE if vals.is_cuda else _lib.MEM_HOST
            return c_void_p(vals.data_ptr()), vals.numel(), mem, vals
        raise TypeError("argument 'vals': expected a numpy array or a torch tensor")

    @staticmethod
    def _method_arg(method: str, fma) -> int:
        """`method` of interpn_hip_create_*: the method plus the per-interpolator flavour of the
        reference's `fma` cargo feature (None = the process default, on)."""
        m = _lib.METHODS[method]
        if fma is None:
            return m
        return m | (_lib.FLAVOUR_FMA if fma else _lib.FLAVOUR_NO_FMA)

    @classmethod
    def regular(cls, method: str, dims, starts, steps, vals, linearize_extrapolation: bool = False,
                device: int = -1, dtype=None, fma=None) -> "Interpolator":
        dtype = np.dtype(dtype or starts.dtype)
        sfx = "f64" if dtype == np.float64 else "f32"
        ct = c_double if dtype == np.float64 else c_float
        lib = _lib.load()
        d, nd = _dims(dims)
        starts = _check_arr("starts", starts, dtype)
        steps = _check_arr("steps", steps, dtype)
        vptr, nvals, mem, keep = cls._vals_arg(vals, dtype)
        h = c_void_p()
        st = getattr(lib, f"interpn_hip_create_regular_{sfx}")(
            cls._method_arg(method, fma), d, nd, starts.ctypes.data_as(POINTER(ct)),
            starts.size, steps.ctypes.data_as(POINTER(ct)), steps.size, vptr, nvals, mem,
            int(bool(linearize_extrapolation)), int(device), ctypes.byref(h))
        _lib.raise_for_status(st)
        it = cls(h.value, dtype, nd, keep if mem == _lib.MEM_DEVICE else None)
        it.method = method
        return it

    @classmethod
    def rectilinear(cls, method: str, grids, vals, linearize_extrapolation: bool = False, device: int = -1,
                    dtype=None, fma=None) -> "Interpolator":
        dtype = np.dtype(dtype or grids[0].dtype)
        sfx = "f64" if dtype == np.float64 else "f32"
        lib = _lib.load()
        gptr, glen, ng, _keep_grids = _slice_of_slices("grids", grids, dtype)
        vptr, nvals, mem, keep = cls._vals_arg(vals, dtype)
        h = c_void_p()
        st = getattr(lib, f"interpn_hip_create_rectilinear_{sfx}")(
            cls._method_arg(method, fma), gptr, glen, ng, vptr, nvals, mem,
            int(bool(linearize_extrapolation)), int(device), ctypes.byref(h))
        _lib.raise_for_status(st)
        it = cls(h.value, dtype, ng, keep if mem == _lib.MEM_DEVICE else None)
        it.method = method
        return it

    @classmethod
    def grid1d_regular(cls, method: str, start, step, vals, device: int = -1, dtype=None, fma=None) -> "Interpolator":
        """interpn::one_dim on RegularGrid1D::new(start, step, vals) (`interpn_hip_create_grid1d_regular_*`);
        `method` is one of "Linear1D", "LinearHoldLast1D", "Left1D", "Right1D", "Nearest1D"."""
        if dtype is None:
            dtype = vals.dtype if isinstance(vals, np.ndarray) else np.float64
        dtype = np.dtype(dtype)
        sfx = "f64" if dtype == np.float64 else "f32"
        lib = _lib.load()
        vptr, nvals, mem, keep = cls._vals_arg(vals, dtype)
        h = c_void_p()
        st = getattr(lib, f"interpn_hip_create_grid1d_regular_{sfx}")(
            cls._method_arg_1d(method, fma), float(start), float(step), vptr, nvals, mem, int(device), ctypes.byref(h))
        _lib.raise_for_status(st)
        return cls(h.value, dtype, 1, keep if mem == _lib.MEM_DEVICE else None)

    @classmethod
    def grid1d_rectilinear(cls, method: str, grid, vals, device: int = -1, dtype=None, fma=None) -> "Interpolator":
        """interpn::one_dim on RectilinearGrid1D::new(grid, vals) (`interpn_hip_create_grid1d_rectilinear_*`)."""
        dtype = np.dtype(dtype or grid.dtype)
        sfx = "f64" if dtype == np.float64 else "f32"
        ct = c_double if dtype == np.float64 else c_float
        lib = _lib.load()
        g = _check_arr("grid", grid, dtype)
        vptr, nvals, mem, keep = cls._vals_arg(vals, dtype)
        h = c_void_p()
        st = getattr(lib, f"interpn_hip_create_grid1d_rectilinear_{sfx}")(
            cls._method_arg_1d(method, fma), g.ctypes.data_as(POINTER(ct)), g.size, vptr, nvals, mem, int(device),
            ctypes.byref(h))
        _lib.raise_for_status(st)
        return cls(h.value, dtype, 1, keep if mem == _lib.MEM_DEVICE else None)

    @staticmethod
    def _method_arg_1d(method: str, fma) -> int:
        m = _lib.METHODS_1D[method]
        if fma is None:
            return m
        return m | (_lib.FLAVOUR_FMA if fma else _lib.FLAVOUR_NO_FMA)

    def replicate(self, device: int = -1) -> "Interpolator":
        """Clone onto another GPU of this process, grid copied device to device
        (`interpn_hip_replicate`); the clone owns its copy."""
        h = c_void_p()
        _lib.raise_for_status(_lib.load().interpn_hip_replicate(self._h, int(device), ctypes.byref(h)))
        it = Interpolator(h.value, self.dtype, self._ndims)
        it.method = self.method
        return it

    # -- evaluation -----------------------------------------------------------------------
    def ndims(self) -> int:
        return self._ndims

    def device(self) -> int:
        return _lib.load().interpn_hip_device(self._h)

    def set_blocks_per_cu(self, n: int) -> None:
        _lib.raise_for_status(_lib.load().interpn_hip_set_blocks_per_cu(self._h, int(n)))

    def set_option(self, name: str, value: int) -> None:
        """Per-handle tuning / testing option (`interpn_hip_set_option`; names in include/interpn_hip.h)."""
        _lib.raise_for_status(_lib.load().interpn_hip_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = ctypes.c_longlong(0)
        _lib.raise_for_status(_lib.load().interpn_hip_get_option(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def kernel_name(self) -> str:
        """Instantiation the most recent evaluation launched, in rocprofv3's spelling ("" before any)."""
        buf = ctypes.create_string_buffer(256)
        _lib.raise_for_status(_lib.load().interpn_hip_kernel_name(self._h, buf, len(buf)))
        return buf.value.decode()

    def table_layout(self):
        """(bytes, step_i, step_j) of the re-laid grid copy the kernels read; (0, 0, 0) = C order.
        After an evaluation that took the 3-D multilinear sweep kernel (`k_linear_sweep<`): that kernel's table (a handle
        may keep two brick tables, e.g. 64^3 f64: (1,2) for the brick kernel, (1,1) for the sweep).  The steps alone do
        not tell the f64 2 x 2 x KW bricks from the f32 2 x 4 x 4 ones (both report (1, 1)): `sweep_brick_form()` does.
        The 2-D, nearest-neighbour and multicubic sweep kernels read the handle's one table (brick / C order / tile):
        for them this returns that table, as for the one-pass kernels."""
        if self.kernel_name().startswith("interpn::k_linear_sweep<"):
            lay = self.get_option("sweep_layout")
            return self.get_option("sweep_table_bytes"), lay // 10, lay % 10
        si, sj = ctypes.c_int(0), ctypes.c_int(0)
        nbytes = _lib.load().interpn_hip_table_bytes(self._h, ctypes.byref(si), ctypes.byref(sj))
        return int(nbytes), int(si.value), int(sj.value)

    def sweep_brick_form(self) -> str:
        """Brick shape of the 3-D multilinear sweep kernel's table: "2x2xKW" (f64; f32 with KW = 8), "2x4x4" (f32), or ""
        when the handle has no such table."""
        if not self.get_option("sweep_table_bytes"):
            return ""
        return "2x4x4" if self.get_option("sweep_cell") == 2 else "2x2xKW"

    def pci_address(self):
        """(domain, bus, device) of the GPU this interpolator lives on, or None if the runtime does not say."""
        v = self.get_option("dev_pci")
        return None if v < 0 else (v >> 16, (v >> 8) & 0xFF, v & 0xFF)

    def _check_same_device(self, what: str, tensor) -> None:
        """`_args.same_device` against this interpolator's GPU."""
        _args.same_device(what, tensor, self.device(), "interpolator", True)

    def eval_host(self, obs, out: np.ndarray) -> np.ndarray:
        """`.interp(obs, out)` on host arrays (synchronous)."""
        lib = _lib.load()
        out = _check_arr("out", out, self.dtype, writable=True)
        optr, olen, nobs, _keep = _slice_of_slices("obs", obs, self.dtype)
        vp = _args.void_pp(optr)
        st = lib.interpn_hip_eval_host(self._h, vp, olen, nobs, out.ctypes.data_as(c_void_p), out.size)
        _lib.raise_for_status(st)
        return out

    def reserve(self, npoints: int, nstreams: int = 1) -> None:
        """Pre-allocate what device evaluations of up to `npoints` points on up to `nstreams`
        concurrent streams need (`interpn_hip_reserve`); afterwards such evaluations allocate
        nothing, also with `no_alloc=True`."""
        _lib.raise_for_status(_lib.load().interpn_hip_reserve(self._h, int(npoints), int(nstreams)))

    def stage_ms(self):
        """Durations (ms) of the most recent sorted evaluation's stages — histogram, scan, scatter,
        evaluation kernel — recorded when option "stage_timing" is 1 (`interpn_hip_stage_ms`)."""
        ms = (c_double * 4)()
        _lib.raise_for_status(_lib.load().interpn_hip_stage_ms(self._h, ms, 4))
        return {"hist": ms[0], "scan": ms[1], "scatter": ms[2], "kernel": ms[3]}

    def eval_device_ptrs(self, obs_ptrs, out_ptr: int, npoints: int, stream: int = 0, no_alloc: bool = False) -> str:
        """Enqueue one evaluation on device buffers given as raw addresses (asynchronous).
        Returns the path taken, "in_place", "binned" or "sweep" (also kept in `.last_path`, with
        `.last_path_reason` saying why a handle that can sort its points evaluated in place)."""
        lib = _lib.load()
        vp = _args.ptr_array(int(p) for p in obs_ptrs)
        path, why = ctypes.c_int(0), ctypes.c_int(0)
        st = lib.interpn_hip_eval_device_ex(self._h, vp, len(obs_ptrs), c_void_p(int(out_ptr)), int(npoints),
                                            c_void_p(int(stream)), _args.eval_flags(no_alloc), ctypes.byref(path),
                                            ctypes.byref(why))
        _lib.raise_for_status(st)
        self.last_path = {_lib.PATH_BINNED: "binned", _lib.PATH_SWEEP: "sweep"}.get(path.value, "in_place")
        self.last_path_reason = _lib.WHY.get(why.value, str(why.value))
        self._pending_streams.setdefault(int(stream), None)
        return self.last_path

    def eval_tensors(self, obs, out=None, stream=None, no_alloc: bool = False):
        """Evaluate on torch CUDA tensors (asynchronous on torch's current stream unless given: a
        torch Stream or a raw hipStream_t integer).  Call `finish()` to synchronise and surface
        "Unrepresentable coordinate value"."""
        want = _args.torch_dtype(self.dtype)
        obs = list(obs)
        dev = self.device()
        n = _args.coord_tensors("obs", obs, want, dev, "interpolator", True)
        out = _args.out_tensor(out, n, want, dev)
        raw, owner = _args.resolve_stream(stream, dev)
        self.eval_device_ptrs([t.data_ptr() for t in obs], out.data_ptr(), n, raw, no_alloc)
        self._pending_streams[raw] = owner
        return out

    # -- value and gradient (multilinear handles) --------------------------------------------
    def _host_grad(self, grad, shape) -> None:
        """What the host forms require of a caller's `grad` before they look at its strides."""
        _args.check_ndarray("grad", grad, self.dtype)
        if grad.shape != shape:
            raise ValueError(f"grad: expected shape {shape}, got {grad.shape}")

    def eval_grad_host(self, obs, out: np.ndarray = None, grad: np.ndarray = None, _entry="interpn_hip_eval_grad_host"):
        """Value and gradient on host arrays (synchronous; `interpn_hip_eval_grad_host`): returns `(out, grad)` with
        `out[i]` the bits of `eval_host` and `grad[d, i]` the derivative of the interpolant with respect to coordinate d
        at point i (shape `(N, n)`), the slope of the cell the value path selects.  Multilinear handles only; on
        "Unrepresentable coordinate value" exactly the entries in front of the failing point have been written."""
        lib = _lib.load()
        optr, olen, nobs, _keep = _slice_of_slices("obs", obs, self.dtype)
        n = int(olen[0]) if nobs else 0
        if out is None:
            out = np.zeros(n, dtype=self.dtype)
        if grad is None:
            grad = np.zeros((nobs, n), dtype=self.dtype)
        out = _check_arr("out", out, self.dtype, writable=True)
        self._host_grad(grad, (nobs, out.size))
        if grad.size and grad.strides[-1] != grad.itemsize:
            raise ValueError("argument 'grad': every row must be contiguous")
        if not grad.flags.writeable:
            raise ValueError("argument 'grad': array is read-only")
        vp = _args.void_pp(optr)
        gp = _args.ptr_array(grad[i].ctypes.data for i in range(nobs))
        st = getattr(lib, _entry)(self._h, vp, olen, nobs, out.ctypes.data_as(c_void_p), out.size, gp)
        _lib.raise_for_status(st)
        return out, grad

    def eval_grad_tensors(self, obs, out=None, grad=None, stream=None, _entry="interpn_hip_eval_grad_device"):
        """The same on torch CUDA tensors (`interpn_hip_eval_grad_device`): one kernel, asynchronous like `eval_tensors`
        and capturable into a graph; `grad` is a tensor of shape `(N, n)` whose rows are contiguous.  `finish()`
        synchronises and surfaces "Unrepresentable coordinate value"."""
        want = _args.torch_dtype(self.dtype)
        obs = list(obs)
        dev = self.device()
        n = _args.coord_tensors("obs", obs, want, dev, "interpolator", True)
        out = _args.out_tensor(out, n, want, dev)
        k = len(obs)
        if grad is None:
            import torch

            grad = torch.empty((k, n), dtype=want, device=torch.device("cuda", dev))
        elif not (grad.is_cuda and grad.dim() == 2 and grad.dtype == want and (grad.numel() == 0 or grad.stride(1) == 1)):
            raise TypeError(f"grad: expected a 2-D {want} CUDA tensor with contiguous rows")
        elif tuple(grad.shape) != (k, n):
            raise ValueError(f"grad: expected shape {(k, n)}, got {tuple(grad.shape)}")
        else:
            _args.same_device("grad", grad, dev, "interpolator", True)
        raw, owner = _args.resolve_stream(stream, dev)
        vp = _args.ptr_array(t.data_ptr() for t in obs)
        gp = _args.ptr_array(grad[d].data_ptr() for d in range(k))
        st = getattr(_lib.load(), _entry)(self._h, vp, k, c_void_p(out.data_ptr()), gp, n, c_void_p(int(raw)))
        _lib.raise_for_status(st)
        self._pending_streams[raw] = owner
        return out, grad

    # -- value and gradient (multicubic handles) ----------------------------------------------
    def eval_cubic_grad_host(self, obs, out: np.ndarray = None, grad: np.ndarray = None):
        """`eval_grad_host` for multicubic handles (`interpn_hip_eval_cubic_grad_host`): `grad[d, i]` is the derivative of
        the Hermite piece the value uses (DESIGN.md "Multicubic gradients"); every other handle raises "unsupported"."""
        return self.eval_grad_host(obs, out, grad, _entry="interpn_hip_eval_cubic_grad_host")

    def eval_cubic_grad_tensors(self, obs, out=None, grad=None, stream=None):
        """`eval_grad_tensors` for multicubic handles (`interpn_hip_eval_cubic_grad_device`): one kernel, capturable."""
        return self.eval_grad_tensors(obs, out, grad, stream, _entry="interpn_hip_eval_cubic_grad_device")

    # -- point-major observation points (one array of shape (n, N)) ---------------------------
    def last_points_path(self):
        """"fused", "split" or "direct": what the most recent point-major evaluation did (None before any)."""
        return _lib.POINTS_PATHS.get(self.get_option("last_points_path"))

    def reserve_points(self, npoints: int, nstreams: int = 1) -> None:
        """Pre-allocate the scratch that point-major evaluations of up to `npoints` points on up to `nstreams` concurrent
        streams need where they de-interleave the points first (`interpn_hip_reserve_points`); afterwards they work with
        `no_alloc=True`.  The fused kernel (multilinear N = 2, 3) needs none."""
        _lib.raise_for_status(_lib.load().interpn_hip_reserve_points(self._h, int(npoints), int(nstreams)))

    def _host_rows(self, name: str, a: np.ndarray) -> int:
        """The row stride of a host `(n, N)` array, points or gradient."""
        return _args.row_stride(name, a.shape[0], self._ndims, _args.elem_strides(a), ValueError,
                                "argument '{name}': every row must be contiguous",
                                "argument '{name}': the row stride must be a whole number of elements, at least {width}")

    def _host_points(self, pts, out):
        """`(n, row stride, out)` of the host point-major forms: `pts` checked, `out` checked or made."""
        _args.check_ndarray("pts", pts, self.dtype)
        if pts.ndim != 2:
            raise TypeError(f"argument 'pts': expected a 2-D array of shape (n, {self._ndims}), got {pts.ndim} dimension(s)")
        n, width = pts.shape
        if width != self._ndims:
            raise _args.dim_mismatch(True)
        stride = self._host_rows("pts", pts)
        if out is None:
            out = np.zeros(n, dtype=self.dtype)
        out = _check_arr("out", out, self.dtype, writable=True)
        if out.size != n:
            raise _args.dim_mismatch(True)
        return n, stride, out

    def _tensor_points(self, pts, out, want, dev: int):
        """`(n, row stride, out)` of the device point-major forms: `pts` checked, `out` checked or made."""
        nd = self._ndims
        what = f"pts: expected a 2-D {want} CUDA tensor of shape (n, {nd}) with stride(1) == 1 and stride(0) >= {nd}"
        if not (hasattr(pts, "is_cuda") and pts.is_cuda and pts.dim() == 2 and pts.dtype == want):
            raise TypeError(what)
        n, width = int(pts.shape[0]), int(pts.shape[1])
        stride = _args.row_stride("pts", n, width, pts.stride(), TypeError, what, what)
        if width != nd:
            raise _args.dim_mismatch(True)
        _args.same_device("pts", pts, dev, "interpolator", True)
        return n, stride, _args.out_tensor(out, n, want, dev, via_lib=True)

    def eval_points_host(self, pts: np.ndarray, out: np.ndarray = None) -> np.ndarray:
        """`.interp` on a host array of shape `(n, N)` whose rows are points (synchronous; `interpn_hip_eval_points_host`):
        `out[i]` has the bits of `eval_host` on the columns `pts[:, d]`, which are never made.  Rows must be contiguous
        (`pts.strides[1] == itemsize`); the row stride may be any whole number of elements >= N, so `buf[:, :3]` of an
        `(n, 4)` array is taken as it is.  On "Unrepresentable coordinate value" exactly the results in front of the
        failing point have been written."""
        n, stride, out = self._host_points(pts, out)
        st = _lib.load().interpn_hip_eval_points_host(self._h, c_void_p(pts.ctypes.data), stride, n, out.ctypes.data_as(c_void_p))
        _lib.raise_for_status(st)
        return out

    def eval_points_tensors(self, pts, out=None, stream=None, no_alloc: bool = False):
        """The same on a torch CUDA tensor of shape `(n, N)` with `stride(1) == 1` and `stride(0) >= N` — a contiguous
        `(n, N)` tensor, or `buf[:, :N]` of a wider one — without `pts.T.contiguous()` (`interpn_hip_eval_points_device`).
        Asynchronous like `eval_tensors`; multilinear N = 2, 3 is one kernel and capturable.  `last_points_path()` says
        which path ran; `finish()` synchronises and surfaces "Unrepresentable coordinate value"."""
        dev = self.device()
        n, stride, out = self._tensor_points(pts, out, _args.torch_dtype(self.dtype), dev)
        raw, owner = _args.resolve_stream(stream, dev)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_eval_points_device(self._h, c_void_p(pts.data_ptr()), stride, n, c_void_p(out.data_ptr()),
                                                        c_void_p(int(raw)), _args.eval_flags(no_alloc), ctypes.byref(path))
        _lib.raise_for_status(st)
        self._pending_streams[raw] = owner
        return out

    # -- point-major value and gradient (positions (n, N) in, gradient (n, N) out) -----------------
    def reserve_points_grad(self, npoints: int, nstreams: int = 1) -> None:
        """`reserve_points` for `eval_points_grad_tensors`: a slice of its split path needs N coordinate and N component
        arrays (`interpn_hip_reserve_points_grad`).  The fused kernels (multilinear and multicubic N = 2, 3) need none."""
        _lib.raise_for_status(_lib.load().interpn_hip_reserve_points_grad(self._h, int(npoints), int(nstreams)))

    def eval_points_grad_host(self, pts: np.ndarray, out: np.ndarray = None, grad: np.ndarray = None):
        """Value and gradient on a host array of shape `(n, N)` whose rows are points (synchronous;
        `interpn_hip_eval_points_grad_host`): returns `(out, grad)` of shapes `(n,)` and `(n, N)` with the bits of
        `eval_grad_host` (multilinear handles) or `eval_cubic_grad_host` (multicubic handles) on the columns `pts[:, d]`,
        `grad[i, d]` being the derivative with respect to coordinate d at point i.  `pts` as for `eval_points_host`; a
        caller's `grad` may be a row-strided view such as `g[:, :3]` of an `(n, 4)` array, whose other columns are left
        alone.  On "Unrepresentable coordinate value" exactly the entries in front of the failing point have been written."""
        n, stride, out = self._host_points(pts, out)
        if grad is None:
            grad = np.zeros((n, self._ndims), dtype=self.dtype)
        self._host_grad(grad, (n, self._ndims))
        if not grad.flags.writeable:
            raise ValueError("argument 'grad': array is read-only")
        gstride = self._host_rows("grad", grad)
        st = _lib.load().interpn_hip_eval_points_grad_host(self._h, c_void_p(pts.ctypes.data), stride, n, out.ctypes.data_as(c_void_p),
                                                           c_void_p(grad.ctypes.data), gstride)
        _lib.raise_for_status(st)
        return out, grad

    def eval_points_grad_tensors(self, pts, out=None, grad=None, stream=None, no_alloc: bool = False):
        """The same on a torch CUDA tensor of shape `(n, N)` with `stride(1) == 1` and `stride(0) >= N`, without
        `pts.T.contiguous()` in front and `grad.T.contiguous()` behind (`interpn_hip_eval_points_grad_device`): returns
        `(out, grad)` of shapes `(n,)` and `(n, N)`.  A caller's `grad` may be a row-strided view (`stride(1) == 1`,
        `stride(0) >= N`) that does not overlap `pts`.  Asynchronous like `eval_tensors`; multilinear and multicubic
        N = 2, 3 are one kernel and capturable.  `last_points_path()` says which path ran; `finish()` synchronises and
        surfaces "Unrepresentable coordinate value"."""
        want = _args.torch_dtype(self.dtype)
        nd = self._ndims
        dev = self.device()
        n, stride, out = self._tensor_points(pts, out, want, dev)
        gwhat = f"grad: expected a 2-D {want} CUDA tensor of shape ({n}, {nd}) with stride(1) == 1 and stride(0) >= {nd}"
        if grad is None:
            import torch

            grad = torch.empty((n, nd), dtype=want, device=torch.device("cuda", dev))
        elif not (hasattr(grad, "is_cuda") and grad.is_cuda and grad.dim() == 2 and grad.dtype == want):
            raise TypeError(gwhat)
        elif tuple(grad.shape) != (n, nd):
            raise ValueError(f"grad: expected shape {(n, nd)}, got {tuple(grad.shape)}")
        gstride = _args.row_stride("grad", n, nd, grad.stride(), TypeError, gwhat, gwhat)
        _args.same_device("grad", grad, dev, "interpolator", True)
        raw, owner = _args.resolve_stream(stream, dev)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_eval_points_grad_device(self._h, c_void_p(pts.data_ptr()), stride, n, c_void_p(out.data_ptr()),
                                                             c_void_p(grad.data_ptr()), gstride, c_void_p(int(raw)),
                                                             _args.eval_flags(no_alloc), ctypes.byref(path))
        _lib.raise_for_status(st)
        self._pending_streams[raw] = owner
        return out, grad

    # -- lattice evaluation (points = tensor product of one coordinate vector per axis) ----
    @property
    def last_lattice_path(self):
        """"fused" or "expanded": what the most recent lattice evaluation did (None before any)."""
        return _lib.LATTICE_PATHS.get(self.get_option("last_lattice_path"))

    def reserve_lattice(self, axis_lens, nstreams: int = 1) -> None:
        """Pre-allocate the scratch of lattice evaluations with up to these axis lengths on up to `nstreams`
        concurrent streams (`interpn_hip_reserve_lattice`); afterwards they work with `no_alloc=True`."""
        lens, n = _dims(axis_lens)
        _lib.raise_for_status(_lib.load().interpn_hip_reserve_lattice(self._h, lens, n, int(nstreams)))

    def _lattice_host(self, axes, out):
        """`(void** axes, lengths, count, shape, out)` of the host lattice forms: `axes` checked, `out` checked or made."""
        aptr, alen, naxes, _keep = _slice_of_slices("axes", axes, self.dtype)
        shape = tuple(int(alen[i]) for i in range(naxes))
        if out is None:
            out = np.zeros(shape, dtype=self.dtype)
        _args.check_ndarray("out", out, self.dtype)
        if naxes == self._ndims and out.shape != shape and out.shape != (int(np.prod(shape, dtype=object)),):
            raise ValueError(f"out: expected shape {shape}, got {out.shape}")
        if not out.flags.c_contiguous:
            raise ValueError("argument 'out': The given array is not contiguous")
        if not out.flags.writeable:
            raise ValueError("argument 'out': array is read-only")
        return _args.void_pp(aptr), alen, naxes, shape, out, _keep

    def _lattice_tensors(self, axes, out):
        """`(axes, lengths, shape, out, device, dtype)` of the device lattice forms: `axes` checked, `out` checked or made."""
        want = _args.torch_dtype(self.dtype)
        axes = list(axes)
        dev = self.device()
        _args.coord_tensors("axes", axes, want, dev, "interpolator", True, same_length=False)
        shape = tuple(int(t.numel()) for t in axes)
        count = int(np.prod(shape, dtype=object)) if shape else 0
        if out is None:
            import torch

            out = torch.empty(shape, dtype=want, device=torch.device("cuda", dev))
        elif not (out.is_cuda and out.is_contiguous() and out.dtype == want):
            raise TypeError(f"out: expected a contiguous {want} CUDA tensor")
        elif len(axes) == self._ndims and tuple(out.shape) != shape and tuple(out.shape) != (count,):
            raise ValueError(f"out: expected shape {shape}, got {tuple(out.shape)}")
        else:
            _args.same_device("out", out, dev, "interpolator", True)
        lens = (c_size_t * max(len(axes), 1))(*shape)
        return axes, lens, shape, out, dev, want

    def eval_lattice_host(self, axes, out: np.ndarray = None) -> np.ndarray:
        """Evaluate on the lattice axes[0] x .. x axes[N-1] of host coordinate vectors (synchronous): the result has
        shape `tuple(len(a) for a in axes)` and equals `eval_host` on `np.meshgrid(*axes, indexing="ij")`, bit for bit
        (`interpn_hip_eval_lattice_host`).  On "Unrepresentable coordinate value" the AssertionError carries
        `first_bad_index` (C order) and exactly the results in front of it have been written."""
        lib = _lib.load()
        vp, alen, naxes, _shape, out, _keep = self._lattice_host(axes, out)
        bad = c_uint64(0)
        st = lib.interpn_hip_eval_lattice_host(self._h, vp, alen, naxes, out.ctypes.data_as(c_void_p), ctypes.byref(bad))
        _args.raise_for_indexed_status(st, bad)
        return out

    def eval_lattice_tensors(self, axes, out=None, stream=None, no_alloc: bool = False):
        """The same on torch CUDA tensors: `axes` are contiguous 1-D tensors of the handle's dtype, the result a tensor of
        shape `tuple(len(a) for a in axes)`.  Asynchronous like `eval_tensors`; `finish()` synchronises and raises
        for a coordinate the reference cannot evaluate, with `first_bad_index` in C order.  `.last_lattice_path` says
        which path ran (`interpn_hip_eval_lattice_device`)."""
        axes, lens, _shape, out, dev, _want = self._lattice_tensors(axes, out)
        raw, owner = _args.resolve_stream(stream, dev)
        path = ctypes.c_int(0)
        st = _lib.load().interpn_hip_eval_lattice_device(self._h, _args.ptr_array(t.data_ptr() for t in axes), lens, len(axes),
                                                         c_void_p(out.data_ptr()), c_void_p(int(raw)), _args.eval_flags(no_alloc),
                                                         ctypes.byref(path))
        _lib.raise_for_status(st)
        self._pending_streams[raw] = owner
        return out

    # -- value and gradient on a lattice ---------------------------------------------------------
    def eval_lattice_grad_host(self, axes, out: np.ndarray = None, grad: np.ndarray = None):
        """Value and gradient on the lattice axes[0] x .. x axes[N-1] of host coordinate vectors (synchronous;
        `interpn_hip_eval_lattice_grad_host`): returns `(out, grad)` of shapes `(*m)` and `(N, *m)`, m = the vectors'
        lengths.  `out` has the bits of `eval_lattice_host`, `grad[d]` those of component d of `eval_grad_host`
        (multilinear handles) or `eval_cubic_grad_host` (multicubic handles) on `np.meshgrid(*axes, indexing="ij")`; every
        other handle raises "unsupported".  On "Unrepresentable coordinate value" the AssertionError carries
        `first_bad_index` (C order) and exactly the entries of `out` and of every `grad[d]` in front of it have been
        written."""
        lib = _lib.load()
        vp, alen, naxes, shape, out, _keep = self._lattice_host(axes, out)
        if grad is None:
            grad = np.zeros((naxes,) + shape, dtype=self.dtype)
        self._host_grad(grad, (naxes,) + shape)
        if not all(grad[d].flags.c_contiguous for d in range(naxes)):
            raise ValueError("argument 'grad': every component grad[d] must be contiguous")
        if not grad.flags.writeable:
            raise ValueError("argument 'grad': array is read-only")
        gp = _args.ptr_array(grad[d].ctypes.data for d in range(naxes))
        bad = c_uint64(0)
        st = lib.interpn_hip_eval_lattice_grad_host(self._h, vp, alen, naxes, out.ctypes.data_as(c_void_p), gp, ctypes.byref(bad))
        _args.raise_for_indexed_status(st, bad)
        return out, grad

    def eval_lattice_grad_tensors(self, axes, out=None, grad=None, stream=None, no_alloc: bool = False):
        """The same on torch CUDA tensors (`interpn_hip_eval_lattice_grad_device`): `axes` as for `eval_lattice_tensors`,
        `grad` a tensor of shape `(N, *m)` whose components `grad[d]` are contiguous.  Asynchronous like `eval_tensors`; the scratch is that of
        `eval_lattice_tensors`, so `reserve_lattice` serves `no_alloc=True` and graph capture here too.
        `.last_lattice_path` says which path ran; `finish()` synchronises and raises for a coordinate the reference cannot
        evaluate, with `first_bad_index` in C order."""
        axes, lens, shape, out, dev, want = self._lattice_tensors(axes, out)
        k = len(axes)
        if grad is None:
            import torch

            grad = torch.empty((k,) + shape, dtype=want, device=torch.device("cuda", dev))
        elif not (hasattr(grad, "is_cuda") and grad.is_cuda and grad.dtype == want):
            raise TypeError(f"grad: expected a {want} CUDA tensor")
        elif tuple(grad.shape) != (k,) + shape:
            raise ValueError(f"grad: expected shape {(k,) + shape}, got {tuple(grad.shape)}")
        elif not all(grad[d].is_contiguous() for d in range(k)):
            raise TypeError("grad: every component grad[d] must be contiguous")
        else:
            _args.same_device("grad", grad, dev, "interpolator", True)
        raw, owner = _args.resolve_stream(stream, dev)
        path = ctypes.c_int(0)
        gp = _args.ptr_array(grad[d].data_ptr() for d in range(k))
        st = _lib.load().interpn_hip_eval_lattice_grad_device(self._h, _args.ptr_array(t.data_ptr() for t in axes), lens, k,
                                                              c_void_p(out.data_ptr()), gp, c_void_p(int(raw)),
                                                              _args.eval_flags(no_alloc), ctypes.byref(path))
        _lib.raise_for_status(st)
        self._pending_streams[raw] = owner
        return out, grad

    def check_bounds_tensors(self, obs, atol: float, stream=None) -> np.ndarray:
        """`check_bounds` on torch CUDA tensors against this interpolator's grid: one flag per
        dimension, True where any coordinate lies outside the grid by `atol` or more
        (src/multilinear/regular.rs:145-182).  The points stay on the device."""
        obs = list(obs)
        dev = self.device()
        n = _args.coord_tensors("obs", obs, _args.torch_dtype(self.dtype), dev, "interpolator", True, via_lib=True)
        raw = _args.resolve_stream(None, dev)[0] if stream is None else int(stream)
        flags = (ctypes.c_uint8 * max(len(obs), 1))()
        st = _lib.load().interpn_hip_check_bounds_device(self._h, _args.ptr_array(t.data_ptr() for t in obs), len(obs), n,
                                                         float(atol), flags, len(obs), c_void_p(int(raw)))
        _lib.raise_for_status(st)
        return np.array([bool(flags[i]) for i in range(len(obs))])

    def finish(self, stream=None) -> None:
        """Wait for the evaluations enqueued since the last finish and raise
        AssertionError("Unrepresentable coordinate value") if any of them hit a NaN/inf/out-of-range
        coordinate.  Without `stream`, EVERY stream used since the last finish is waited for (the
        status word is sticky per handle, not per stream); with `stream` (a torch Stream or a raw
        integer) only that one."""
        lib = _lib.load()
        if stream is not None:
            raws = [_args.resolve_stream(stream, None)[0]]
        else:
            raws = list(self._pending_streams)
        if not raws:
            try:
                import torch

                raws = [torch.cuda.current_stream(self.device()).cuda_stream if torch.cuda.is_available() else 0]
            except ImportError:
                raws = [0]
        _args.finish_streams(lib.interpn_hip_finish, self._h, raws, self._pending_streams)

    def close(self) -> None:
        if self._h is not None and self._h.value:
            _lib.load().interpn_hip_destroy(self._h)
            self._h = c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def eval_host_sharded(interps, obs, out: np.ndarray) -> np.ndarray:
    """Single-process multi-GPU `.interp(obs, out)`: contiguous ranges of the observation index,
    one per interpolator in `interps` (create one per device from the same grid), evaluated
    concurrently (`interpn_hip_eval_host_sharded`).  On "Unrepresentable coordinate value" the
    AssertionError carries `first_bad_index` (global)."""
    interps = list(interps)
    if not interps:
        raise ValueError("eval_host_sharded needs at least one interpolator")
    lib = _lib.load()
    dtype = interps[0].dtype
    out = _check_arr("out", out, dtype, writable=True)
    optr, olen, nobs, _keep = _slice_of_slices("obs", obs, dtype)
    vp = _args.void_pp(optr)
    hs = (c_void_p * len(interps))()
    for i, it in enumerate(interps):
        hs[i] = it._h
    bad = c_uint64(0)
    st = lib.interpn_hip_eval_host_sharded(hs, len(interps), vp, olen, nobs, out.ctypes.data_as(c_void_p), out.size,
                                           ctypes.byref(bad))
    _args.raise_for_indexed_status(st, bad)
    return out


def eval_device_sharded(interps, obs_shards, out_shards=None):
    """Single-process multi-GPU evaluation of device-resident shards (`interpn_hip_eval_device_sharded`):
    `obs_shards[r]` is the list of N coordinate tensors of shard r on the device of `interps[r]`
    (clones made with `.replicate(device)`), `out_shards[r]` its result tensor (allocated when
    omitted).  Every shard is enqueued on its device's current torch stream before the first is
    waited for; returns the list of result tensors.  On "Unrepresentable coordinate value" the
    AssertionError carries `first_bad_index`, counting the shards' points in shard order."""
    import torch

    interps = list(interps)
    if not interps or len(obs_shards) != len(interps):
        raise ValueError("eval_device_sharded needs one list of coordinate tensors per interpolator")
    lib = _lib.load()
    n = len(interps)
    nd = interps[0].ndims()
    tdt = _args.torch_dtype(interps[0].dtype)
    outs = list(out_shards) if out_shards is not None else [None] * n
    hs = (c_void_p * n)()
    obs_pp = (ctypes.POINTER(c_void_p) * n)()
    out_p = (c_void_p * n)()
    npts = (c_size_t * n)()
    streams = (c_void_p * n)()
    keep = []
    for r, it in enumerate(interps):
        shard = list(obs_shards[r])
        if len(shard) != nd:
            raise AssertionError("Dimension mismatch")
        count = int(shard[0].numel())
        for t in shard:
            if t.dtype != tdt or not t.is_contiguous() or int(t.numel()) != count:
                raise ValueError("coordinate tensors of a shard must be contiguous, of the interpolator's dtype and equally long")
            it._check_same_device("obs", t)
        if outs[r] is None:
            outs[r] = torch.empty(count, dtype=tdt, device=shard[0].device)
        it._check_same_device("out", outs[r])
        arr = _args.ptr_array(t.data_ptr() for t in shard)
        keep.append(arr)
        hs[r] = it._h
        obs_pp[r] = ctypes.cast(arr, ctypes.POINTER(c_void_p))
        out_p[r] = outs[r].data_ptr()
        npts[r] = count
        streams[r] = torch.cuda.current_stream(shard[0].device).cuda_stream
    bad = c_uint64(0)
    st = lib.interpn_hip_eval_device_sharded(hs, n, obs_pp, nd, out_p, npts, streams, ctypes.byref(bad))
    _args.raise_for_indexed_status(st, bad)
    return outs

