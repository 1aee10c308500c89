"""Shared helpers for the parity tests: seeded synthetic workloads and
dispatch of a `kat.Case` to either the oracle or the HIP path."""

from __future__ import annotations

import numpy as np


def run_oracle(oracle, case, fma=True, dtype=None, out=None):
    dtype = dtype or case.vals.dtype
    if out is None:
        out = np.zeros(case.obs[0].size, dtype=dtype)
    if case.method == "nearest" and case.kind == "regular":
        oracle.nearest_regular(case.dims, case.starts, case.steps, case.vals, case.obs, out, fma=fma)
    elif case.method == "nearest":
        oracle.nearest_rectilinear(case.grids, case.vals, case.obs, out, fma=fma)
    elif case.method == "linear" and case.kind == "regular":
        oracle.linear_regular(case.dims, case.starts, case.steps, case.vals, case.obs, out, fma=fma)
    elif case.method == "linear":
        oracle.linear_rectilinear(case.grids, case.vals, case.obs, out, fma=fma)
    elif case.kind == "regular":
        oracle.cubic_regular(case.dims, case.starts, case.steps, case.vals, case.linearize, case.obs, out, fma=fma)
    else:
        oracle.cubic_rectilinear(case.grids, case.vals, case.linearize, case.obs, out, fma=fma)
    return out


def run_hip_raw(case, dtype=None, out=None):
    """Through the reference-named raw functions -> C ABI one-shot entry points."""
    from interpn_amd import raw

    dtype = np.dtype(dtype or case.vals.dtype)
    sfx = "f64" if dtype == np.float64 else "f32"
    cv = lambda a: np.ascontiguousarray(a, dtype=dtype)
    if out is None:
        out = np.zeros(case.obs[0].size, dtype=dtype)
    obs = [cv(o) for o in case.obs]
    if case.method == "nearest" and case.kind == "regular":
        getattr(raw, f"interpn_nearest_regular_{sfx}")(case.dims, cv(case.starts), cv(case.steps), cv(case.vals), obs, out)
    elif case.method == "nearest":
        getattr(raw, f"interpn_nearest_rectilinear_{sfx}")([cv(g) for g in case.grids], cv(case.vals), obs, out)
    elif case.method == "linear" and case.kind == "regular":
        getattr(raw, f"interpn_linear_regular_{sfx}")(case.dims, cv(case.starts), cv(case.steps), cv(case.vals), obs, out)
    elif case.method == "linear":
        getattr(raw, f"interpn_linear_rectilinear_{sfx}")([cv(g) for g in case.grids], cv(case.vals), obs, out)
    elif case.kind == "regular":
        getattr(raw, f"interpn_cubic_regular_{sfx}")(case.dims, cv(case.starts), cv(case.steps), cv(case.vals),
                                                      case.linearize, obs, out)
    else:
        getattr(raw, f"interpn_cubic_rectilinear_{sfx}")([cv(g) for g in case.grids], cv(case.vals), case.linearize,
                                                          obs, out)
    return out


def synthetic_case(method, kind, n, npts_axis, nobs, seed, dtype=np.float64, linearize=False, extrap=0.05,
                   specials=True):
    """Synthetic workload of SURVEY.md §8(d): axes linspace(-1,1,n) (rectilinear: interior nodes
    jittered by up to a quarter step), vals U(-1,1), obs i.i.d. uniform over the grid extent
    widened by `extrap` on each side, plus injected special points (exact nodes, domain ends,
    +-0)."""
    from tests.kat import Case

    rng = np.random.default_rng(seed)
    grids = []
    for d in range(n):
        g = np.linspace(-1.0, 1.0, npts_axis[d])
        if kind == "rectilinear":
            step = g[1] - g[0]
            j = (rng.random(g.size) - 0.5) * 0.5 * step
            j[0] = j[-1] = 0.0
            g = g + j
        g = g.astype(dtype)
        assert np.all(np.diff(g) > 0)
        grids.append(g)
    vals = rng.uniform(-1.0, 1.0, int(np.prod(npts_axis))).astype(dtype)
    obs = []
    for d in range(n):
        lo, hi = float(grids[d][0]), float(grids[d][-1])
        w = (hi - lo) * extrap
        o = rng.uniform(lo - w, hi + w, nobs).astype(dtype)
        if specials and nobs >= 64:
            k = min(grids[d].size, 24)
            o[:k] = grids[d][:k]  # exact nodes
            o[k] = grids[d][-1]
            o[k + 1] = grids[d][0]
            o[k + 2] = 0.0
            o[k + 3] = -0.0
            o[k + 4] = np.nextafter(grids[d][-1], np.inf, dtype=dtype)
            o[k + 5] = np.nextafter(grids[d][0], -np.inf, dtype=dtype)
            o[k + 6] = grids[d][-2]
            o[k + 7] = grids[d][1]
        obs.append(o)
    if specials and nobs >= 64 and n > 1:
        # de-correlate the special rows across dimensions
        for d in range(1, n):
            obs[d][:40] = np.roll(obs[d][:40], 3 * d)
    return Case(f"syn_{method}_{kind}_N{n}", method, kind, grids, vals, obs, np.zeros(nobs, dtype=dtype), 0.0,
                linearize=linearize)


# (start, step) of axis d of `anisotropic_case`: origins large against the step (d = 0, 2), steps that are no binary
# fraction (1, 3), one that is (4), and eight decades between the smallest and the largest step.
ANISO_AXES = ((1000.25, 0.0375), (-3e-3, 7e-4), (-5e4, 1.3e3), (0.5, 1.0 / 3.0), (7.0, 2.0 ** -7), (-0.125, 11.0))


def anisotropic_axis(d, n, kind, dtype, rng):
    """Axis d of `anisotropic_case`, n nodes.  Regular: start + step * arange(n).  Rectilinear: the same ends, the
    intervals by d % 3 — growing geometrically (x1.7 per interval, ~70 between first and last), shrinking (x0.55,
    ~1/120), or equal with a cluster of intervals at 1e-3 of the others in the middle (two; twenty from 24 nodes on) —
    each scaled by 1 + 0.2 (U - 0.5).  Axes of more than 9 nodes spread the same total ratio over their intervals."""
    start, step = ANISO_AXES[d % len(ANISO_AXES)]
    step *= 2.0 ** (d // len(ANISO_AXES))
    if kind == "regular":
        g = (start + step * np.arange(n)).astype(dtype)
    else:
        m = n - 1  # intervals
        mode = d % 3
        if mode < 2:
            q = (1.7, 0.55)[mode]
            if m > 8:
                q = q ** (8.0 / (m - 1))
            h = q ** np.arange(m)
        else:
            h = np.ones(m)
            short = 20 if n >= 24 else min(2, m - 1)
            lo = (m - short) // 2
            h[lo:lo + short] = 1e-3
        h = h * (1.0 + 0.2 * (rng.random(m) - 0.5))
        h *= step * m / h.sum()
        g = start + np.concatenate([[0.0], np.cumsum(h)])
        g[-1] = start + step * m
        g = g.astype(dtype)
    assert np.all(np.diff(g) > 0), (d, n, kind, np.dtype(dtype).name)
    return g


def anisotropic_points(g, count, rng, dtype, extrap=0.2):
    """`count` coordinates on axis g by the point rule of `anisotropic_case`: exact nodes (12 at most), both ends and
    their floating-point neighbours outside the grid; of the rest one half cell-uniform (a cell drawn uniformly, then a
    position in it: short intervals are hit as often as long ones) and one half uniform over the extent widened by
    `extrap` on each side; shuffled."""
    g64 = g.astype(np.float64)
    nodes = g[rng.choice(g.size, min(g.size, 12), replace=False)]
    special = np.concatenate([nodes, [g[0], g[-1], np.nextafter(g[0], dtype(-np.inf)), np.nextafter(g[-1], dtype(np.inf))]])
    special = special[:max(0, count - 2)].astype(dtype)
    rest = count - special.size
    ncell = rest // 2
    c = rng.integers(0, g.size - 1, ncell)
    in_cell = (g64[c] + rng.random(ncell) * (g64[c + 1] - g64[c])).astype(dtype)
    w = (g64[-1] - g64[0]) * extrap
    wide = rng.uniform(g64[0] - w, g64[-1] + w, rest - ncell).astype(dtype)
    x = np.concatenate([special, in_cell, wide]).astype(dtype)
    rng.shuffle(x)
    return x


def anisotropic_case(method, kind, shape, nobs, seed, dtype=np.float64, linearize=False, extrap=0.2):
    """The second workload: every axis with its own origin, scale and spacing (ANISO_AXES, `anisotropic_axis`), so that
    a per-axis quantity taken from the wrong axis, or a search that only works on near-uniform axes, changes the result
    — on `synthetic_case` neither does.  vals U(-1, 1); points by `anisotropic_points`, shuffled per axis."""
    from tests.kat import Case

    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype).type
    grids = [anisotropic_axis(d, shape[d], kind, dtype, rng) for d in range(len(shape))]
    vals = rng.uniform(-1.0, 1.0, int(np.prod(shape))).astype(dtype)
    obs = [anisotropic_points(g, nobs, rng, dtype, extrap) for g in grids]
    return Case(f"aniso_{method}_{kind}_N{len(shape)}", method, kind, grids, vals, obs, np.zeros(nobs, dtype=dtype), 0.0,
                linearize=linearize)


def poison_count(shape, method):
    """How many nodes `poison_table` makes non-finite ("nan", "mixed"): with F nodes in a point's footprint (2^N
    multilinear, 4^N multicubic, 1 nearest) a share 1 - 0.5^(1/F) of the table leaves about half the points clean."""
    size = int(np.prod(shape))
    f = {"linear": 2.0, "cubic": 4.0, "nearest": 1.0}[method] ** len(shape)
    return max(1, int(round(size * (1.0 - 0.5 ** (1.0 / f)))))


def poison_table(vals, shape, method, seed, kind):
    """A copy of the table `vals` with non-finite nodes; every other node keeps its value.  kind "nan": `poison_count`
    distinct nodes, drawn by a seeded `rng.choice`, are NaN.  "mixed": the same nodes, each NaN, +inf or -inf at random.
    "plane": every node with index 3 along the shape's longest axis (the first of them; it needs n >= 5) is NaN — for
    multicubic the fourth node of that axis's first cell, which the saturated cell does not use."""
    out = np.array(vals, copy=True)
    assert out.size == int(np.prod(shape))
    if kind == "plane":
        d = int(np.argmax(shape))
        assert shape[d] >= 5, shape
        index = [slice(None)] * len(shape)
        index[d] = 3
        out.reshape(shape)[tuple(index)] = np.nan
        return out
    assert kind in ("nan", "mixed"), kind
    rng = np.random.default_rng(seed)
    where = rng.choice(out.size, poison_count(shape, method), replace=False)
    if kind == "nan":
        out[where] = np.nan
    else:
        out[where] = rng.choice(np.array([np.nan, np.inf, -np.inf]), where.size).astype(out.dtype)
    return out


def footprint_cells(case):
    """Per axis the cell index c of every point of `case`: j = floor((x - start) / step) in the element type (regular)
    or (number of nodes < x) - 1 (rectilinear), clamped to [0, n - 2]."""
    dt = case.vals.dtype.type
    cells = []
    for d, (g, x) in enumerate(zip(case.grids, case.obs)):
        x = np.asarray(x, dtype=dt)
        if case.kind == "regular":
            j = np.floor((x - dt(case.starts[d])) / dt(case.steps[d])).astype(np.float64)
        else:
            j = np.searchsorted(np.asarray(g, dtype=dt), x, side="left").astype(np.float64) - 1.0
        cells.append(np.clip(j, 0, g.size - 2).astype(np.int64))
    return cells


def footprint_poisoned(case):
    """One bool per point of `case` (linear or cubic): the nodes its arithmetic touches include a non-finite one.  Along
    an axis of n nodes with cell c (`footprint_cells`) multilinear uses nodes c and c + 1; multicubic uses c - 1 .. c + 2,
    but 0 .. 2 in the first cell and n - 3 .. n - 1 in the last (the fourth node of a saturated cell is not used).  The
    footprint is the product over the axes, for coordinates outside the grid too.  Written with numpy alone: a summed
    table of the non-finite nodes, and the box sum of every point's footprint by inclusion and exclusion."""
    assert case.method in ("linear", "cubic"), case.method
    shape = case.dims
    bad = ~np.isfinite(case.vals.reshape(shape))
    summed = np.zeros([n + 1 for n in shape], dtype=np.int64)  # summed[i0, i1, ..] = bad nodes with index < i_d on every axis
    summed[tuple(slice(1, None) for _ in shape)] = bad
    for d in range(len(shape)):
        summed = np.cumsum(summed, axis=d)
    lo, hi = [], []  # the footprint's nodes along axis d: lo <= i < hi
    for c, n in zip(footprint_cells(case), shape):
        if case.method == "linear":
            lo.append(c)
            hi.append(c + 2)
        else:
            assert n >= 3, shape
            lo.append(np.where(c == 0, 0, np.where(c == n - 2, n - 3, c - 1)))
            hi.append(np.where(c == 0, 3, np.where(c == n - 2, n, c + 3)))
    count = np.zeros(case.obs[0].size, dtype=np.int64)
    for corner in range(1 << len(shape)):
        index = tuple(hi[d] if (corner >> d) & 1 else lo[d] for d in range(len(shape)))
        sign = -1 if (len(shape) - bin(corner).count("1")) & 1 else 1
        count += sign * summed[index]
    return count > 0


def rel_err(a, b):
    """|a-b| / max(|b|, 1) — the reference's normalisation (test/test_multicubic_regular.py:97-100)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1.0)
