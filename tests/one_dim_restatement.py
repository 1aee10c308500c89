"""CPU restatement of interpn::one_dim (src/one_dim/*.rs of the reference crate), written from the Rust and used by
tests/test_one_dim_cpu.py (which pins it to hand-derived answers) and tests/test_one_dim_gpu.py (which compares the
kernels with it).  Test infrastructure only: IEEE arithmetic in the element type through numpy, the fused step of the
`fma` flavour exactly through fractions.Fraction, rounded once to the element type (ties to even).

    eval(method, kind, dtype, fma, locs, start=, step=, vals=)   regular grid
    eval(method, kind, dtype, fma, locs, grid=, vals=)           rectilinear grid
returns (out, first_bad): out[i] for every point the reference evaluates, first_bad = index of the first point on
which it returns Err("Unrepresentable number") (None if none).  Values at and behind first_bad are NaN.
"""

from __future__ import annotations

from fractions import Fraction

import numpy as np

METHODS = ("Linear1D", "LinearHoldLast1D", "Left1D", "Right1D", "Nearest1D")
INSIDE, LOW, HIGH = 0, 1, 2


def round_to(fr: Fraction, dtype) -> np.floating:
    """The exact rational `fr` rounded to the nearest value of `dtype`, ties to even."""
    dtype = np.dtype(dtype)
    try:
        f64 = float(fr)  # correctly rounded to f64
    except OverflowError:
        return dtype.type(np.inf if fr > 0 else -np.inf)
    if dtype == np.float64:
        return np.float64(f64)
    with np.errstate(over="ignore"):
        c = np.float32(f64)
    if not np.isfinite(c):
        return c
    best = None
    for cand in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        d = abs(Fraction(float(cand)) - fr)
        key = (d, int(np.array(cand).view(np.uint32)) & 1)  # nearer first, then the even one
        if best is None or key < best[0]:
            best = (key, cand)
    return np.float32(best[1])


def fma(a, b, c, dtype):
    """a * b + c with one rounding to `dtype` (Float::mul_add)."""
    T = np.dtype(dtype).type
    a, b, c = T(a), T(b), T(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return T(a * b + c)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if exact == 0:
        with np.errstate(all="ignore"):
            return T(a * b + c)  # the sign of an exact zero: IEEE's rules for the sum of the rounded terms
    return round_to(exact, dtype)


def partition_point_lt(g: np.ndarray, x: np.ndarray) -> np.ndarray:
    """core::slice::partition_point(|v| v < &x) with Rust std's probe sequence, restated from
    oracle/interpn_oracle.cpp:74-90 (size-halving binary search; on an unsorted slice it is this exact sequence that
    decides the answer)."""
    n = len(g)
    size = n
    base = np.zeros(x.shape, dtype=np.int64)
    while size > 1:
        half = size >> 1
        mid = base + half
        base = np.where(g[mid] < x, mid, base)
        size -= half
    return base + (g[base] < x).astype(np.int64)


def regular_stop(start, step, n, dtype):
    """RegularGrid1D::new: stop = start + step * T(n - 1), two roundings in T (one_dim/mod.rs:87-88)."""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        return T(T(start) + T(step) * T(n - 1))


def grid_at(kind, dtype, locs, start=None, step=None, grid=None, vals=None):
    """Grid1D::at for every point: (i, extrap, x0, x1, y0, y1, bad)."""
    T = np.dtype(dtype).type
    x = np.asarray(locs, dtype=dtype)
    vals = np.asarray(vals, dtype=dtype)
    n = len(vals)
    with np.errstate(all="ignore"):
        if kind == "regular":
            start, step = T(start), T(step)
            stop = regular_stop(start, step, n, dtype)
            # one_dim/mod.rs:100-104: > stop first, then < start; NaN is inside
            ext = np.where(x > stop, HIGH, np.where(x < start, LOW, INSIDE))
            q = np.floor((x - start) / step)  # one_dim/mod.rs:107, in T
            # <isize as NumCast>::from: Some iff -2^63 <= q < 2^63 (one_dim/mod.rs:110-111)
            bad = ~((q >= -(2.0**63)) & (q < 2.0**63))
            # the cast to isize comes first, then .max(0).min(n - 2) in integers (one_dim/mod.rs:110-113): clamping in T
            # would round n - 2 in f32 past 2^24
            i = np.clip(np.where(bad, 0, q).astype(np.float64).astype(np.int64), 0, n - 2)
            x0 = start + step * i.astype(dtype)  # one_dim/mod.rs:124-126: not fused; T(i) rounds in f32 past 2^24
            x1 = x0 + step
        else:
            g = np.asarray(grid, dtype=dtype)
            # one_dim/mod.rs:158-159
            i = np.clip(partition_point_lt(g, x) - 1, 0, n - 2)
            # one_dim/mod.rs:161-165: < g[0] first, then > g[n-1]
            ext = np.where(x < g[0], LOW, np.where(x > g[n - 1], HIGH, INSIDE))
            x0, x1 = g[i], g[i + 1]  # one_dim/mod.rs:176
            bad = np.zeros(x.shape, dtype=bool)
    return i, ext, x0, x1, vals[i], vals[i + 1], bad


def eval(method, kind, dtype, fma_flavour, locs, start=None, step=None, grid=None, vals=None):
    dtype = np.dtype(dtype)
    x = np.asarray(locs, dtype=dtype)
    i, ext, x0, x1, y0, y1, bad = grid_at(kind, dtype, x, start, step, grid, vals)
    with np.errstate(all="ignore"):
        if method == "Left1D":  # one_dim/hold.rs:33-36
            out = np.where(ext == HIGH, y1, y0)
        elif method == "Right1D":  # one_dim/hold.rs:68-71
            out = np.where(ext == LOW, y0, y1)
        elif method == "Nearest1D":  # one_dim/hold.rs:98-104: a tie goes left, NaN right
            dx0 = np.abs(x - x0)
            dx1 = np.abs(x - x1)
            out = np.where(dx1 >= dx0, y0, y1)
        else:
            slope = (y1 - y0) / (x1 - x0)  # one_dim/linear.rs:28 / :70
            dx = x - x0
            if fma_flavour:  # slope.mul_add(dx, y0), one_dim/linear.rs:34 / :76
                lin = np.array([fma(s, d, y, dtype) for s, d, y in zip(slope, dx, y0)], dtype=dtype)
            else:
                lin = y0 + slope * dx
            if method == "Linear1D":
                out = lin
            else:  # one_dim/linear.rs:68-81
                out = np.where(ext == INSIDE, lin, np.where(ext == LOW, y0, y1))
    out = np.asarray(out, dtype=dtype).copy()
    first_bad = None
    if bad.any():
        first_bad = int(np.argmax(bad))
        out[first_bad:] = np.nan
    return out, first_bad
