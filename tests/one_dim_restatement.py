"""CPU restatement of interpn::one_dim (src/one_dim/*.rs of the reference crate), written from the Rust and used by
tests/test_one_dim_cpu.py (which pins it to hand-derived answers) and tests/test_one_dim_gpu.py (which compares the
kernels with it).  Test infrastructure only: IEEE arithmetic in the element type through numpy, the fused step of the
`fma` flavour exactly through fractions.Fraction, rounded once to the element type (ties to even).

    eval(method, kind, dtype, fma, locs, start=, step=, vals=)   regular grid
    eval(method, kind, dtype, fma, locs, grid=, vals=)           rectilinear grid
returns (out, first_bad): out[i] for every point the reference evaluates, first_bad = index of the first point on
which it returns Err("Unrepresentable number") (None if none).  Values at and behind first_bad are NaN.

    fma_vec(a, b, c, dtype)      the fused step for arrays, vectorised and still rounded once (eval uses it)
    exact(method, kind, dtype, locs, ...)   the reference's formula in exact rationals, cells by exact comparison
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


def _round_to_odd_sum(x, y):
    """RO(x + y) for f64 arrays: the f64 neighbour of the exact sum whose last significand bit is 1 when the sum is not
    itself an f64 (round to odd), the sum when it is.  s = RN(x + y) and Knuth's TwoSum gives e with s + e = x + y
    exactly (no overflow: the callers bound the operands).  The exact sum lies strictly between s and its neighbour on
    the side of e; neighbouring floats alternate in parity (also across a power of two: 1.11..1 is odd, 1.00..0 even),
    so if s is even that neighbour is the odd one."""
    s = x + y
    bb = s - x
    e = (x - (s - bb)) + (y - bb)
    even = (s.view(np.int64) & 1) == 0
    return np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def _two_prod(a, b):
    """Dekker's product with Veltkamp's split (f64 arrays): p = RN(a b) and e with p + e = a b exactly, provided nothing
    overflows or underflows (the callers bound the operands)."""
    c = 134217729.0  # 2^27 + 1
    p = a * b
    t = c * a
    ah = t - (t - a)
    al = a - ah
    t = c * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_vec(a, b, c, dtype):
    """`fma` for arrays, without a Python loop and still with ONE rounding.  Why it is exact:

    f32.  a, b, c convert to f64 exactly.  a b has at most 48 significant bits and an exponent within +-300, so the f64
    product p is exact.  r = RO(p + c) is the sum rounded to odd in f64 (53 bits); rounding r to f32 (24 bits, ties to
    even, numpy's conversion) equals rounding the exact sum directly, because 53 >= 24 + 2 (Boldo and Melquiond,
    "Emulation of a FMA and correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 57(4), 2008,
    theorem 1; a subnormal f32 result has fewer bits still, and f64 neither over- nor underflows on these operands).  A
    plain RN(p + c) in f64 followed by the conversion would round twice; that is the shortcut this is not.  An exact
    zero sum has e = 0 and the sign IEEE gives x + (-x), which is also fma's.

    f64.  The same paper's FMA emulation (its algorithm 5): (uh, ul) = a b exactly (Dekker), (th, tl) = c + uh exactly
    (TwoSum), v = RO(tl + ul), result RN(th + v); proven to be RN(a b + c) when nothing underflows.  It is applied only
    where 2^-400 <= |a|, |b| <= 2^400 and 2^-800 <= |c| <= 2^900: every intermediate is then a multiple of 2^-906 below
    2^901, so no step over- or underflows.  With a, b in that range and c = 0 the result is RN(a b) (nonzero, its own
    sign).  With a or b zero the product is an exact signed zero and a b + c in f64 is already exact.

    Everything else (non-finite operands, magnitudes outside those ranges) goes through `fma` one element at a time.
    tests/test_one_dim_cpu.py pins this function to `fma` on random, tie and next-to-tie operands."""
    dtype = np.dtype(dtype)
    shape = np.broadcast(np.asarray(a), np.asarray(b), np.asarray(c)).shape
    a, b, c = (np.broadcast_to(np.asarray(v, dtype=dtype), shape).ravel() for v in (a, b, c))
    a64, b64, c64 = a.astype(np.float64), b.astype(np.float64), c.astype(np.float64)
    out = np.empty(a.shape, dtype=dtype)
    with np.errstate(all="ignore"):
        finite = np.isfinite(a64) & np.isfinite(b64) & np.isfinite(c64)
        if dtype == np.float32:
            vec = finite
            out[vec] = _round_to_odd_sum(a64[vec] * b64[vec], c64[vec]).astype(np.float32)
        else:
            aa, ab, ac = np.abs(a64), np.abs(b64), np.abs(c64)
            mid = lambda v: (v >= 2.0**-400) & (v <= 2.0**400)
            zero_prod = finite & ((a64 == 0) | (b64 == 0))
            prod_only = finite & mid(aa) & mid(ab) & (c64 == 0)
            full = finite & mid(aa) & mid(ab) & (ac >= 2.0**-800) & (ac <= 2.0**900)
            out[zero_prod] = a64[zero_prod] * b64[zero_prod] + c64[zero_prod]
            out[prod_only] = a64[prod_only] * b64[prod_only]
            uh, ul = _two_prod(a64[full], b64[full])
            cf = c64[full]
            th = cf + uh
            bb = th - cf
            tl = (cf - (th - bb)) + (uh - bb)
            out[full] = th + _round_to_odd_sum(tl, ul)
            vec = zero_prod | prod_only | full
    for k in np.flatnonzero(~vec):
        out[k] = fma(a[k], b[k], c[k], dtype)
    return out.reshape(shape)


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
                lin = fma_vec(slope, dx, y0, dtype)  # pinned to `fma` by tests/test_one_dim_cpu.py
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


def exact(method, kind, dtype, locs, start=None, step=None, grid=None, vals=None):
    """The value of the reference's formula in exact rationals, independent of `eval`'s arithmetic.

    The cell is chosen by exact comparison against the floating-point knots: on a regular grid the knots
    T(start + step T(i)) as the reference rounds them (they are the grid it defines; cell i holds K_i <= x < K_i+1), on a
    rectilinear one the axis itself with partition_point's convention (g_i < x <= g_i+1); both clamped to [0, n - 2].
    x0 is that knot and x1 what the formula uses (regular: T(x0 + step), one_dim/mod.rs:126; rectilinear: g[i + 1]).
    Linear1D is y0 + (y1 - y0) (x - x0) / (x1 - x0) without any rounding, LinearHoldLast1D that inside and y0 / y1 outside,
    Left1D / Right1D / Nearest1D select a grid value.

    Returns (value, scale, cell, tie): per point a Fraction (None where x, a knot or a value of the cell is not finite or
    x1 = x0), the error scale |y0| + |(y1 - y0) (x - x0) / (x1 - x0)| of the linear pair (0 for a selected value), the
    cell, and for Nearest1D whether |x - x0| = |x - x1| exactly.  Axes must be sorted (NaN-free)."""
    dtype = np.dtype(dtype)
    T = dtype.type
    x = np.asarray(locs, dtype=dtype)
    v = np.asarray(vals, dtype=dtype)
    n = len(v)
    with np.errstate(all="ignore"):
        if kind == "regular":
            knots = (T(start) + T(step) * np.arange(n).astype(dtype)).astype(dtype)
            stop = regular_stop(start, step, n, dtype)
            cell = np.clip(np.searchsorted(knots, x, side="right") - 1, 0, n - 2)
            ext = np.where(x > stop, HIGH, np.where(x < T(start), LOW, INSIDE))
            x0 = knots[cell]
            x1 = (x0 + T(step)).astype(dtype)
        else:
            g = np.asarray(grid, dtype=dtype)
            cell = np.clip(np.searchsorted(g, x, side="left") - 1, 0, n - 2)
            ext = np.where(x < g[0], LOW, np.where(x > g[n - 1], HIGH, INSIDE))
            x0, x1 = g[cell], g[cell + 1]
    y0, y1 = v[cell], v[cell + 1]
    usable = np.isfinite(x) & np.isfinite(x0) & np.isfinite(x1) & np.isfinite(y0) & np.isfinite(y1)
    value, scale, tie = [None] * len(x), [Fraction(0)] * len(x), np.zeros(len(x), dtype=bool)
    fr = lambda f: Fraction(float(f))
    for j in np.flatnonzero(usable):
        e = ext[j]
        if method == "Left1D":
            value[j] = fr(y1[j] if e == HIGH else y0[j])
        elif method == "Right1D":
            value[j] = fr(y0[j] if e == LOW else y1[j])
        elif method == "Nearest1D":
            d0, d1 = abs(fr(x[j]) - fr(x0[j])), abs(fr(x[j]) - fr(x1[j]))
            tie[j] = d0 == d1
            value[j] = fr(y0[j] if d1 >= d0 else y1[j])
        elif method == "LinearHoldLast1D" and e != INSIDE:
            value[j] = fr(y0[j] if e == LOW else y1[j])
        elif x1[j] != x0[j]:
            t = (fr(y1[j]) - fr(y0[j])) * (fr(x[j]) - fr(x0[j])) / (fr(x1[j]) - fr(x0[j]))
            value[j] = fr(y0[j]) + t
            scale[j] = abs(fr(y0[j])) + abs(t)
    return value, scale, cell, tie
