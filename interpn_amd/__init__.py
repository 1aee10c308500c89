"""interpn_amd — MI355X (gfx950) implementation of the batched per-observation-point hot path of
jlogan03/interpn (multilinear / multicubic interpolation on regular and rectilinear grids).

The public names mirror the reference's Python package (src/interpn/__init__.py): `interpn()`,
`raw`, and the `Multilinear*/Multicubic*` classes.  Everything evaluates through the HIP kernels
behind the C ABI of include/interpn_hip.h; there is no CPU evaluation path in this package.
"""

from __future__ import annotations

from collections.abc import Sequence
from typing import Literal

import numpy as np

from . import _args, _lib, _setup, one_dim, raw
from ._setup import check_regular as _check_regular
from ._setup import is_cuda_tensor as _is_cuda_tensor
from .classes import (MulticubicRectilinear, MulticubicRegular, MultilinearRectilinear, MultilinearRegular,
                      NearestRectilinear, NearestRegular)
from .fields import (Fields, fields_lattice_grad_plan, fields_lattice_plan, fields_layout, interpn_fields, interpn_fields_grad,
                     interpn_fields_lattice, interpn_fields_lattice_grad, interpn_fields_points, interpn_fields_points_grad)
from .handle import Interpolator, eval_device_sharded, eval_host_sharded

__version__ = "0.1.0"

def trim(device: int = -1) -> int:
    """Release the device memory of destroyed interpolators that the library keeps for reuse on
    `device` (`interpn_hip_trim`; -1 = the current device).  Returns the bytes released."""
    import ctypes

    freed = ctypes.c_size_t(0)
    _lib.raise_for_status(_lib.load().interpn_hip_trim(int(device), ctypes.byref(freed)))
    return int(freed.value)


__all__ = [
    "one_dim",
    "trim",
    "eval_host_sharded",
    "eval_device_sharded",
    "__version__",
    "raw",
    "interpn",
    "interpn_fields",
    "interpn_fields_grad",
    "interpn_fields_lattice",
    "interpn_fields_lattice_grad",
    "interpn_fields_points",
    "interpn_fields_points_grad",
    "interpn_grad",
    "interpn_lattice",
    "interpn_points",
    "interpn_points_grad",
    "interpn_lattice_grad",
    "lattice_plan",
    "lattice_grad_plan",
    "Fields",
    "fields_lattice_plan",
    "fields_lattice_grad_plan",
    "fields_layout",
    "Interpolator",
    "MultilinearRegular",
    "MultilinearRectilinear",
    "MulticubicRegular",
    "MulticubicRectilinear",
    "NearestRegular",
    "NearestRectilinear",
]


def interpn(
    obs: Sequence,
    grids: Sequence,
    vals,
    *,
    method: Literal["linear", "cubic", "nearest"] = "linear",
    out=None,
    linearize_extrapolation: bool = True,
    assume_regular: bool = False,
    check_bounds: bool = False,
    bounds_atol: float = 1e-8,
):
    """Evaluate an N-dimensional grid at the supplied observation points.

    Same contract as the reference's helper (src/interpn/__init__.py:48-194): inputs are
    ravelled and made contiguous, the dtype is taken from `vals` (float64 / float32), a grid is
    treated as regular iff every axis has exactly equal spacing (`_check_regular`, :197-203)
    or `assume_regular` is set, and the call dispatches to the matching raw function (:135-192).
    """
    if len(obs) and _is_cuda_tensor(obs[0]):
        return _interpn_on_device(obs, grids, vals, method, out, linearize_extrapolation, assume_regular,
                                  check_bounds, bounds_atol)
    # src/interpn/__init__.py:86-88 (the reference's `out or ...` raises on multi-element arrays;
    # `is None` is what it means)
    out = out if out is not None else np.zeros_like(obs[0])
    outshape = out.shape
    out = out.ravel()

    obs = [np.ascontiguousarray(x.ravel()) for x in obs]
    grids = [np.ascontiguousarray(x.ravel()) for x in grids]
    vals = np.ascontiguousarray(vals.ravel())

    dtype = vals.dtype
    assert dtype in [np.float64, np.float32], "`interpn` defined only for float32 and float64 data"

    is_regular = assume_regular or _check_regular(grids)

    if is_regular:
        dims = [len(grid) for grid in grids]
        starts = np.array([grid[0] for grid in grids], dtype=dtype)
        steps = np.array([grid[1] - grid[0] for grid in grids], dtype=dtype)

    sfx = "f64" if dtype == np.float64 else "f32"

    if check_bounds:
        outb = np.zeros(len(grids), dtype=bool)
        if is_regular:
            getattr(raw, f"check_bounds_regular_{sfx}")(dims, starts, steps, obs, bounds_atol, outb)
        else:
            getattr(raw, f"check_bounds_rectilinear_{sfx}")(grids, obs, bounds_atol, outb)
        if any(outb):
            raise ValueError("Observation points violate interpolator bounds")

    if method == "linear":
        if is_regular:
            getattr(raw, f"interpn_linear_regular_{sfx}")(dims, starts, steps, vals, obs, out)
        else:
            getattr(raw, f"interpn_linear_rectilinear_{sfx}")(grids, vals, obs, out)
    elif method == "nearest":
        if is_regular:
            getattr(raw, f"interpn_nearest_regular_{sfx}")(dims, starts, steps, vals, obs, out)
        else:
            getattr(raw, f"interpn_nearest_rectilinear_{sfx}")(grids, vals, obs, out)
    elif method == "cubic":
        if is_regular:
            getattr(raw, f"interpn_cubic_regular_{sfx}")(dims, starts, steps, vals, linearize_extrapolation, obs, out)
        else:
            getattr(raw, f"interpn_cubic_rectilinear_{sfx}")(grids, vals, linearize_extrapolation, obs, out)
    else:
        raise ValueError(f"Unsupported interpolation configuration: {dtype}, {is_regular}, {method}")

    return out.reshape(outshape)


def _interpn_on_device(obs, grids, vals, method, out, linearize_extrapolation, assume_regular, check_bounds,
                       bounds_atol):
    """`interpn()` for observation points that already live on the GPU (torch CUDA tensors): same
    rules as the host form (ravelled inputs, dtype from `vals`, exact-spacing regularity test,
    optional bounds check), the points and the result never cross PCIe.  Returns a tensor."""
    import torch

    _setup.check_method(method)
    shape = (out if out is not None else obs[0]).shape
    obs_t = _setup.flat_coords(obs, True)
    if not _is_cuda_tensor(vals):
        vals = np.asarray(vals)
    dtype, grids, vals = _setup.grids_and_values(grids, vals)
    device = _setup.device_index(obs_t[0])
    if _is_cuda_tensor(vals) and vals.device.index not in (None, device):
        raise ValueError(f"vals is on {vals.device} but the observation points are on cuda:{device}")
    it, _spec = _setup.interpolator(method, grids, vals, dtype, device, assume_regular, linearize_extrapolation)
    try:
        if check_bounds:
            _setup.check_device_bounds(it, obs_t, bounds_atol)
        if out is not None:
            if not out.is_contiguous():
                raise ValueError("out: expected a contiguous CUDA tensor")
            out_t = out.reshape(-1)
        else:
            out_t = torch.empty_like(obs_t[0])
        it.eval_tensors(obs_t, out_t)
        it.finish()
    finally:
        it.close()
    return out_t.reshape(shape)


def interpn_grad(
    obs: Sequence,
    grids: Sequence,
    vals,
    *,
    method: str = "linear",
    linearize_extrapolation: bool = True,
    assume_regular: bool = False,
    check_bounds: bool = False,
    bounds_atol: float = 1e-8,
):
    """Multilinear (or, with `method="cubic"`, multicubic) value and gradient at the observation points in one pass: returns `(out, grad)`, `out` shaped like
    `obs[0]` with the bits of `interpn(obs, grids, vals, method="linear")`, `grad` of shape `(N, *obs[0].shape)` with
    `grad[d]` the derivative of the interpolant with respect to coordinate d — the slope of the cell the value uses
    (outside the grid: of the linear extrapolation).  Arrays for numpy points, tensors for torch CUDA points.

    The rules are those of `interpn()`: inputs ravelled, dtype from `vals`, regular iff every spacing is exactly equal or
    `assume_regular`.  `method="cubic"`: the value is `interpn(..., method="cubic", linearize_extrapolation=...)` and the
    gradient that of the C1 Hermite piece the value uses (DESIGN.md "Multicubic gradients"); `linearize_extrapolation` has no
    effect on the linear method."""
    if method not in ("linear", "cubic"):
        raise ValueError(f"interpn_grad: method must be \"linear\" or \"cubic\", got {method!r}")
    cubic = method == "cubic"
    lin = bool(linearize_extrapolation) if cubic else False
    obs = list(obs)
    on_device = bool(obs) and _is_cuda_tensor(obs[0])
    dtype, grids, vals = _setup.grids_and_values(grids, vals)
    shape = tuple(obs[0].shape) if obs else (0,)
    device = _setup.device_index(obs[0]) if on_device else -1
    flat = _setup.flat_coords(obs, on_device)
    it, spec = _setup.interpolator(method, grids, vals, dtype, device, assume_regular, lin)
    try:
        if check_bounds:
            _setup.check_bounds(it, flat, on_device, grids, spec, dtype, bounds_atol)
        if on_device:
            out, grad = (it.eval_cubic_grad_tensors if cubic else it.eval_grad_tensors)(flat)
            it.finish()
        else:
            out, grad = (it.eval_cubic_grad_host if cubic else it.eval_grad_host)(flat)
    finally:
        it.close()
    return out.reshape(shape), grad.reshape((len(flat),) + shape)


def _rows_set_up(xi, grids, vals, method, linearize_extrapolation, assume_regular, check_bounds, bounds_atol):
    """What `interpn_points` and `interpn_points_grad` do before they evaluate: `(interpolator, rows, shape, on_device)`
    with `xi` of shape `(..., N)` flattened to `(n, N)` rows, `shape` its leading dimensions, and the bounds checked on the
    unstacked columns.  The caller closes the interpolator."""
    on_device = _is_cuda_tensor(xi)
    if not on_device:
        xi = np.asarray(xi)
    if len(xi.shape) < 1 or xi.shape[-1] != len(grids):
        raise AssertionError(_lib.strerror(_lib.ERR_DIM_MISMATCH))
    dtype, grids, vals = _setup.grids_and_values(grids, vals)
    n = len(grids)
    device = _setup.device_index(xi) if on_device else -1
    flat = xi if len(xi.shape) == 2 else xi.reshape(-1, n)
    if n > 1 and (flat.stride(1) != 1 if on_device else flat.strides[1] != flat.itemsize):  # copied only if it has to be
        flat = flat.contiguous() if on_device else np.ascontiguousarray(flat)
    it, spec = _setup.interpolator(method, grids, vals, dtype, device, assume_regular, linearize_extrapolation)
    try:
        if check_bounds:
            cols = [flat[:, d].contiguous() if on_device else np.ascontiguousarray(flat[:, d]) for d in range(n)]
            _setup.check_bounds(it, cols, on_device, grids, spec, dtype, bounds_atol)
    except BaseException:
        it.close()
        raise
    return it, flat, tuple(xi.shape[:-1]), on_device


def interpn_points(
    xi,
    grids: Sequence,
    vals,
    *,
    method: Literal["linear", "cubic", "nearest"] = "linear",
    out=None,
    linearize_extrapolation: bool = True,
    assume_regular: bool = False,
    check_bounds: bool = False,
    bounds_atol: float = 1e-8,
):
    """`interpn()` for points kept as ONE array `xi` of shape `(..., N)` — scipy's `xi`, particle positions, ray samples:
    returns an array (numpy `xi`) or a tensor (torch CUDA `xi`) of shape `xi.shape[:-1]` whose entries have the bits of
    `interpn([xi[..., 0], .., xi[..., N-1]], grids, vals, ...)`.  The columns are never made: multilinear N = 2, 3 reads
    the rows in its one kernel, everything else de-interleaves slices of them on the device.

    The rules are those of `interpn()`: dtype from `vals` (`xi` must have it), regular iff every spacing is exactly equal
    or `assume_regular`.  `check_bounds` unstacks the columns for the existing check."""
    _setup.check_method(method)
    it, flat, shape, on_device = _rows_set_up(xi, grids, vals, method, linearize_extrapolation, assume_regular, check_bounds,
                                              bounds_atol)
    try:
        if out is not None:
            if on_device and not out.is_contiguous():
                raise ValueError("out: expected a contiguous CUDA tensor")
            if not on_device and not (isinstance(out, np.ndarray) and out.flags.c_contiguous):
                raise ValueError("argument 'out': The given array is not contiguous")
            out = out.reshape(-1)
        if on_device:
            res = it.eval_points_tensors(flat, out)
            it.finish()
        else:
            res = it.eval_points_host(flat, out)
    finally:
        it.close()
    return res.reshape(shape)


def interpn_points_grad(
    xi,
    grids: Sequence,
    vals,
    *,
    method: str = "linear",
    linearize_extrapolation: bool = True,
    assume_regular: bool = False,
    check_bounds: bool = False,
    bounds_atol: float = 1e-8,
):
    """`interpn_grad()` for points kept as ONE array `xi` of shape `(..., N)`, the gradient in the same layout: returns
    `(out, grad)` of shapes `xi.shape[:-1]` and `xi.shape` — arrays for a numpy `xi`, tensors for a torch CUDA `xi` — with
    the bits of `interpn_grad([xi[..., 0], .., xi[..., N-1]], grids, vals, ...)`, `grad[..., d]` being its `grad[d]`.
    Neither the columns nor the component arrays are made: multilinear and multicubic N = 2, 3 read the rows and write the
    gradient rows in their one kernel, everything else works on slices on the device.

    The rules are those of `interpn_points()` and `interpn_grad()`: `method` "linear" or "cubic", dtype from `vals` (`xi`
    must have it), regular iff every spacing is exactly equal or `assume_regular`; `linearize_extrapolation` has no
    effect on the linear method; `check_bounds` unstacks the columns for the existing check."""
    if method not in ("linear", "cubic"):
        raise ValueError(f"interpn_points_grad: method must be \"linear\" or \"cubic\", got {method!r}")
    lin = bool(linearize_extrapolation) if method == "cubic" else False
    it, flat, shape, on_device = _rows_set_up(xi, grids, vals, method, lin, assume_regular, check_bounds, bounds_atol)
    try:
        if on_device:
            res, grad = it.eval_points_grad_tensors(flat)
            it.finish()
        else:
            res, grad = it.eval_points_grad_host(flat)
    finally:
        it.close()
    return res.reshape(shape), grad.reshape(shape + (flat.shape[1],))


def interpn_lattice(
    axes: Sequence,
    grids: Sequence,
    vals,
    *,
    method: Literal["linear", "cubic", "nearest"] = "linear",
    out=None,
    linearize_extrapolation: bool = True,
    assume_regular: bool = False,
    check_bounds: bool = False,
    bounds_atol: float = 1e-8,
):
    """`interpn()` on the lattice axes[0] x .. x axes[N-1]: one coordinate vector per grid axis instead of N arrays of
    expanded points.  Returns an array (a tensor, if the vectors are torch CUDA tensors) of shape
    `tuple(len(a) for a in axes)` whose element [i_0, .., i_{N-1}] is the interpolant at (axes[0][i_0], ..,
    axes[N-1][i_{N-1}]) — the bits of `interpn(np.meshgrid(*axes, indexing="ij"), ...)`, without the meshgrid.

    The rules are those of `interpn()`: inputs ravelled, dtype from `vals`, regular iff every spacing is exactly equal or
    `assume_regular`.  `check_bounds` checks the N vectors (a lattice is inside the grid exactly when each axis is)."""
    _setup.check_method(method)
    return _lattice_call(axes, grids, vals, method, out, linearize_extrapolation, assume_regular, check_bounds, bounds_atol, False)


def _lattice_call(axes, grids, vals, method, out, linearize_extrapolation, assume_regular, check_bounds, bounds_atol, with_grad):
    """What `interpn_lattice` and `interpn_lattice_grad` share: set-up, the bounds check on the N vectors, the evaluation."""
    axes, grids = list(axes), list(grids)
    if len(axes) != len(grids):
        raise ValueError(f"axes: expected {len(grids)} coordinate vectors (one per grid axis), got {len(axes)}")
    on_device = bool(axes) and _is_cuda_tensor(axes[0])
    dtype, grids, vals = _setup.grids_and_values(grids, vals)
    shape = tuple(int(a.numel()) if _is_cuda_tensor(a) else int(np.asarray(a).size) for a in axes)
    if out is not None and tuple(out.shape) != shape:
        raise ValueError(f"out: expected shape {shape}, got {tuple(out.shape)}")
    device = _setup.device_index(axes[0]) if on_device else -1
    axes = _setup.flat_coords(axes, on_device)
    it, _spec = _setup.interpolator(method, grids, vals, dtype, device, assume_regular, linearize_extrapolation)
    try:
        if check_bounds:
            # N short batches: axis d is checked against dimension d with the other coordinates held at the grid's origin
            import torch

            dev = torch.device("cuda", it.device())
            tdt = _args.torch_dtype(dtype)
            for d, a in enumerate(axes):
                a_t = a if on_device else torch.from_numpy(a).to(dev)
                if a_t.numel() == 0:
                    continue
                batch = [a_t if e == d else torch.full((a_t.numel(),), float(grids[e][0]), dtype=tdt, device=dev)
                         for e in range(len(grids))]
                if it.check_bounds_tensors(batch, bounds_atol)[d]:
                    raise ValueError(_setup.OUT_OF_BOUNDS)
        if on_device:
            res = it.eval_lattice_grad_tensors(axes, out) if with_grad else it.eval_lattice_tensors(axes, out)
            it.finish()
        else:
            res = it.eval_lattice_grad_host(axes, out) if with_grad else it.eval_lattice_host(axes, out)
    finally:
        it.close()
    return res


def interpn_lattice_grad(
    axes: Sequence,
    grids: Sequence,
    vals,
    *,
    method: str = "linear",
    out=None,
    linearize_extrapolation: bool = True,
    assume_regular: bool = False,
    check_bounds: bool = False,
    bounds_atol: float = 1e-8,
):
    """`interpn_grad()` on the lattice axes[0] x .. x axes[N-1]: returns `(out, grad)` of shapes `(*m)` and `(N, *m)`, m =
    the vectors' lengths — arrays for numpy vectors, tensors for torch CUDA ones — with the bits of
    `interpn_grad(np.meshgrid(*axes, indexing="ij"), grids, vals, ...)`, without the meshgrid: forces on a finer mesh, the
    partial derivatives of a refined table.  `method` "linear" or "cubic"; `linearize_extrapolation` has no effect on the
    linear method; the other rules are those of `interpn_lattice()`."""
    if method not in ("linear", "cubic"):
        raise ValueError(f"interpn_lattice_grad: method must be \"linear\" or \"cubic\", got {method!r}")
    lin = bool(linearize_extrapolation) if method == "cubic" else False
    return _lattice_call(axes, grids, vals, method, out, lin, assume_regular, check_bounds, bounds_atol, True)


def lattice_plan(dtype, method: str, dims, axis_lens):
    """(path, lds_bytes, npoints): the path ("fused" / "expanded") a lattice of `axis_lens` coordinates per axis takes in
    automatic mode on a grid of `dims`, the LDS bytes of the fused kernel's workgroup and the point count
    (`interpn_hip_lattice_plan`; needs no device)."""
    return _lattice_plan("interpn_hip_lattice_plan", dtype, method, dims, axis_lens)


def lattice_grad_plan(dtype, method: str, dims, axis_lens):
    """`lattice_plan` for a value-and-gradient call (`interpn_hip_lattice_grad_plan`; needs no device): the fused kernel
    keeps L lines per wave (multilinear N + 1, multicubic N) where the value's keeps one.  `method` "linear" or "cubic"."""
    return _lattice_plan("interpn_hip_lattice_grad_plan", dtype, method, dims, axis_lens)


def _lattice_plan(entry, dtype, method, dims, axis_lens):
    import ctypes

    from .raw import _dims

    d, nd = _dims(dims)
    m, nm = _dims(axis_lens)
    if nd != nm:
        raise ValueError(f"axis_lens: expected {nd} lengths, got {nm}")
    path, lds, npts = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    st = getattr(_lib.load(), entry)(np.dtype(dtype).itemsize, _lib.METHODS[method], nd, d, m, ctypes.byref(path),
                                     ctypes.byref(lds), ctypes.byref(npts))
    _lib.raise_for_status(st)
    return _lib.LATTICE_PATHS[path.value], int(lds.value), int(npts.value)


