"""interpn::one_dim (src/one_dim/*.rs of the reference crate, re-exported at its root, src/lib.rs:102-105): the
one-dimensional grids and the five interpolators with hold semantics, evaluated by the HIP kernels of
interpn_amd/csrc/k_one_dim.hip.

    grid = RegularGrid1D(start, step, vals)        # or RectilinearGrid1D(grid, vals)
    out = Linear1D(grid).eval(locs)                # numpy in, numpy out (host path)
    out = Linear1D(grid, device=0).eval(t)         # contiguous 1-D torch CUDA tensor in, tensor out

Reference errors raise AssertionError(msg) like the rest of the package: "Length mismatch", and for regular grids
"Unrepresentable number" with `first_bad_index` (the evaluation stops at the first failing point; on the host path
out[0..i) is written and out[i..] untouched).  A regular grid of fewer than two values raises ReferencePanic (the
reference panics).  `fma` selects the flavour of the reference's `fma` cargo feature (None: the process default, on).
"""

from __future__ import annotations

import ctypes
from ctypes import c_uint64, c_void_p

import numpy as np

from . import _args, _lib
from .handle import Interpolator
from .raw import _check_arr

__all__ = ["RegularGrid1D", "RectilinearGrid1D", "Linear1D", "LinearHoldLast1D", "Left1D", "Right1D", "Nearest1D"]


def _dtype_of(a):
    if isinstance(a, np.ndarray):
        return a.dtype
    if hasattr(a, "dtype") and hasattr(a, "data_ptr"):
        return np.dtype(np.float64) if str(a.dtype) == "torch.float64" else np.dtype(np.float32)
    raise TypeError("expected a numpy array or a torch tensor")


class RegularGrid1D:
    """RegularGrid1D::new(start, step, vals) (one_dim/mod.rs:86-95).  No check of `step`; `vals` (numpy, or a
    torch CUDA tensor that the interpolator then borrows) holds at least two values."""

    def __init__(self, start, step, vals):
        self.dtype = _dtype_of(vals)
        self.start = self.dtype.type(start)
        self.step = self.dtype.type(step)
        self.vals = vals

    def _create(self, method, device, fma):
        return Interpolator.grid1d_regular(method, self.start, self.step, self.vals, device=device, dtype=self.dtype,
                                           fma=fma)


class RectilinearGrid1D:
    """RectilinearGrid1D::new(grid, vals) (one_dim/mod.rs:148-154): "Length mismatch" unless the two have the
    same length of at least 2.  The grid is not checked for sortedness."""

    def __init__(self, grid, vals):
        self.dtype = _dtype_of(vals)
        self.grid = _check_arr("grid", grid, self.dtype)
        if len(self.grid) != int(vals.shape[0]) or len(self.grid) < 2:
            raise AssertionError("Length mismatch")
        self.vals = vals

    def _create(self, method, device, fma):
        return Interpolator.grid1d_rectilinear(method, self.grid, self.vals, device=device, dtype=self.dtype, fma=fma)


class _Interp1D:
    _method = ""

    def __init__(self, grid, device: int = -1, fma=None):
        self.grid = grid
        self.dtype = grid.dtype
        self.interpolator = grid._create(self._method, device, fma)

    def eval(self, locs, out=None):
        """Interp1D::eval / eval_alloc (one_dim/mod.rs:51-73).  numpy: through the host path, returns `out`.  A
        contiguous 1-D torch CUDA tensor: through the device path on the current stream, synchronised before
        returning (use `.interpolator.eval_tensors` / `.finish` for asynchronous work)."""
        if isinstance(locs, np.ndarray):
            locs = _check_arr("locs", locs, self.dtype)
            if out is None:
                out = np.zeros(locs.shape[0], dtype=self.dtype)
            out = _check_arr("out", out, self.dtype, writable=True)
            if out.shape[0] != locs.shape[0]:
                raise AssertionError("Length mismatch")
            lib = _lib.load()
            vp = (c_void_p * 1)(locs.ctypes.data_as(c_void_p))
            lens = (ctypes.c_size_t * 1)(locs.shape[0])
            hs = (c_void_p * 1)(self.interpolator._h)
            bad = c_uint64(0)
            # the one-handle sharded form: the host path's abort-at-first-bad-point contract plus the failing index
            st = lib.interpn_hip_eval_host_sharded(hs, 1, vp, lens, 1, out.ctypes.data_as(c_void_p), out.shape[0],
                                                   ctypes.byref(bad))
            _args.raise_for_indexed_status(st, bad)
            return out
        if out is not None and int(out.numel()) != int(locs.numel()):
            raise AssertionError("Length mismatch")
        res = self.interpolator.eval_tensors([locs], out)
        self.interpolator.finish()
        return res

    def eval_one(self, x):
        """Interp1D::eval_one: one point."""
        return self.eval(np.array([x], dtype=self.dtype))[0]

    def kernel_name(self) -> str:
        return self.interpolator.kernel_name()

    def close(self) -> None:
        self.interpolator.close()


class Linear1D(_Interp1D):
    """Linear interpolation, linear extrapolation (one_dim/linear.rs:26-37)."""
    _method = "Linear1D"


class LinearHoldLast1D(_Interp1D):
    """Linear inside, the end value of the clamped cell outside (one_dim/linear.rs:60-85)."""
    _method = "LinearHoldLast1D"


class Left1D(_Interp1D):
    """Hold-last (one_dim/hold.rs:26-38)."""
    _method = "Left1D"


class Right1D(_Interp1D):
    """Hold-next (one_dim/hold.rs:61-73)."""
    _method = "Right1D"


class Nearest1D(_Interp1D):
    """Nearest value, ties to the left (one_dim/hold.rs:94-107)."""
    _method = "Nearest1D"
