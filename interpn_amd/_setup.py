"""Grid set-up of the one-call helpers (`interpn_grad`, `interpn_points`, `interpn_lattice`, `interpn_fields*`, ..): from
`grids` and `vals` as the caller has them to a device-resident `Interpolator` or `Fields`, and the bounds check in front
of the evaluation.  The rules are those of `interpn()`: inputs ravelled, dtype from `vals`, a grid regular iff every
spacing is exactly equal or the caller says so.  `interpn()` on host arrays mirrors the reference's helper line by line
and does not come through here."""

from __future__ import annotations

import numpy as np

from . import raw
from .handle import Interpolator

OUT_OF_BOUNDS = "Observation points violate interpolator bounds"


def is_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def is_cuda_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda") and bool(x.is_cuda)


def check_regular(grids) -> bool:
    """src/interpn/__init__.py:197-203 — exact equality of all spacings."""
    is_regular = True
    for grid in grids:
        dgrid = np.diff(grid)
        is_regular = is_regular and np.all(dgrid == dgrid[0])
    return bool(is_regular)


def check_method(method) -> None:
    if method not in ("linear", "cubic", "nearest"):
        raise ValueError(f"Unsupported interpolation configuration: {method}")


def device_index(t) -> int:
    """The GPU a CUDA tensor is on: the interpolator lives where the points are, not on whatever device is current."""
    if t.device.index is not None:
        return t.device.index
    import torch

    return torch.cuda.current_device()


def value_dtype(vals) -> np.dtype:
    assert str(vals.dtype).endswith(("float64", "float32")), "`interpn` defined only for float32 and float64 data"
    return np.dtype(np.float64 if str(vals.dtype).endswith("64") else np.float32)


def canonical_grids(grids, dtype):
    return [np.ascontiguousarray(np.asarray(g).ravel()).astype(dtype, copy=False) for g in grids]


def grids_and_values(grids, vals):
    """`(dtype, grids, vals)`: the dtype of `vals`, the grids as contiguous 1-D arrays of it, `vals` flattened (a numpy
    array, or a torch CUDA tensor that stays on its device)."""
    if not (is_cuda_tensor(vals) or isinstance(vals, np.ndarray)):
        raise TypeError("argument 'vals': expected a numpy array or a torch tensor")
    dtype = value_dtype(vals)
    vals = vals.reshape(-1).contiguous() if is_cuda_tensor(vals) else np.ascontiguousarray(vals.ravel())
    return dtype, canonical_grids(grids, dtype), vals


def field_values_dtype(vals, axis_words: str = "a field axis") -> np.dtype:
    if not (isinstance(vals, np.ndarray) or is_tensor(vals)):
        raise TypeError(f"vals: expected a numpy array or a torch tensor with {axis_words}")
    return value_dtype(vals)


def value_count_error(k, nper, grids, vals) -> ValueError:
    return ValueError(f"vals: expected {k} x {nper} values for grids of {[g.size for g in grids]}, got shape {tuple(vals.shape)}")


def field_major(vals, k: int, nper: int, fields_last: bool, on_device: bool):
    """`vals` of shape (K, *dims), or (*dims, K) with `fields_last`, as a contiguous (K, prod(dims)) array or tensor: done
    once, as part of setting the fields up.  Host points take a host table."""
    if fields_last:
        vals = vals.reshape(nper, k).T
    vals = (vals.contiguous() if is_tensor(vals) else np.ascontiguousarray(vals)).reshape(k, nper)
    if not on_device and is_tensor(vals):
        vals = vals.cpu().numpy()
    return vals


def grids_and_fields(grids, vals, field_axis, naxes=None):
    """`grids_and_values` for a field set with its fields along `field_axis` (0 or -1): `(dtype, grids, k, nper)`, `vals`
    still in the caller's layout (`field_major` re-lays it).  `naxes`: the number of coordinate vectors of a lattice, which
    must be that of the grids."""
    dtype = field_values_dtype(vals)
    if len(vals.shape) < 2:
        raise ValueError("vals: expected a field axis besides the grid's values")
    grids = canonical_grids(grids, dtype)
    if naxes is not None and naxes != len(grids):
        raise ValueError(f"axes: expected {len(grids)} coordinate vectors (one per grid axis), got {naxes}")
    nper = int(np.prod([g.size for g in grids], dtype=object))
    k = int(vals.shape[field_axis])
    if k * nper != int(np.prod(tuple(vals.shape), dtype=object)):
        raise value_count_error(k, nper, grids, vals)
    return dtype, grids, k, nper


def regular_spec(grids, dtype, assume_regular: bool):
    """`(dims, starts, steps)` of a grid that is regular (or assumed so); None for a rectilinear one."""
    if not (assume_regular or check_regular(grids)):
        return None
    return ([len(g) for g in grids], np.array([g[0] for g in grids], dtype=dtype),
            np.array([g[1] - g[0] for g in grids], dtype=dtype))


def create(cls, method, grids, spec, vals, dtype, device, **how):
    """An `Interpolator` or a `Fields` (`cls`) on the grid: regular from `spec`, else rectilinear from `grids`."""
    if spec is not None:
        return cls.regular(method, *spec, vals, device=device, dtype=dtype, **how)
    return cls.rectilinear(method, grids, vals, device=device, dtype=dtype, **how)


def interpolator(method, grids, vals, dtype, device, assume_regular: bool, linearize_extrapolation: bool):
    """`(interpolator, spec)` of a helper on its canonical grids."""
    spec = regular_spec(grids, dtype, assume_regular)
    return create(Interpolator, method, grids, spec, vals, dtype, device, linearize_extrapolation=linearize_extrapolation), spec


def check_host_bounds(grids, spec, dtype, cols, atol) -> None:
    """The reference's bounds check on host coordinate arrays, one per dimension."""
    sfx = "f64" if dtype == np.float64 else "f32"
    outb = np.zeros(len(grids), dtype=bool)
    if spec is not None:
        getattr(raw, f"check_bounds_regular_{sfx}")(*spec, cols, atol, outb)
    else:
        getattr(raw, f"check_bounds_rectilinear_{sfx}")(grids, cols, atol, outb)
    if any(outb):
        raise ValueError(OUT_OF_BOUNDS)


def check_device_bounds(it, cols, atol) -> None:
    if it.check_bounds_tensors(cols, atol).any():
        raise ValueError(OUT_OF_BOUNDS)


def check_bounds(it, cols, on_device: bool, grids, spec, dtype, atol) -> None:
    """The bounds check of the helpers on one coordinate array or tensor per dimension."""
    if on_device:
        check_device_bounds(it, cols, atol)
    else:
        check_host_bounds(grids, spec, dtype, cols, atol)


def check_field_device_bounds(method, grids, spec, vals, dtype, device, cols, atol) -> None:
    """The bounds are the grid's: any one field's interpolator checks them on the device."""
    one = create(Interpolator, method, grids, spec, vals[0], dtype, device)
    try:
        check_device_bounds(one, cols, atol)
    finally:
        one.close()


def flat_coords(coords, on_device: bool):
    """Coordinate arrays or tensors, one per dimension, each ravelled and contiguous."""
    if on_device:
        return [x.reshape(-1).contiguous() for x in coords]
    return [np.ascontiguousarray(np.asarray(x).ravel()) for x in coords]
