"""Shared helpers for the parity tests: seeded synthetic workloads and
dispatch of a `kat.Case` to either the oracle or the HIP path."""

from __future__ import annotations

import dataclasses

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


def class_draw(g, c, count, rng, dtype, outside=False):
    """`count` coordinates of saturation class `c` on the axis `g` (n nodes): the class is the clamped cell index of
    `footprint_cells`, 0 .. n - 2; class 0 also holds everything below the grid, class n - 2 everything above it.  Inside
    the grid the points are uniform in the cell [g[c], g[c + 1]] shrunk by a tenth of its width at each end, so that an
    estimate of the class ((x - start) * scale on regular grids, the counting sort's) and the exact class agree.  With
    `outside` the points of class 0 lie below g[0] and those of class n - 2 above g[-1], by 0.001 to 0.3 of the span."""
    g64 = np.asarray(g, dtype=np.float64)
    n = g64.size
    assert 0 <= c <= n - 2, (c, n)
    u = rng.random(count)
    if outside:
        assert c in (0, n - 2), (c, n)
        off = (g64[-1] - g64[0]) * (0.001 + 0.299 * u)
        x = g64[0] - off if c == 0 else g64[-1] + off
    else:
        w = g64[c + 1] - g64[c]
        x = g64[c] + w * (0.1 + 0.8 * u)
    return x.astype(dtype)


def class_pairs(case):
    """Every pair of saturation classes of axes 0 and 1: the bins of the sorted multicubic path, in C order."""
    return [(c0, c1) for c0 in range(case.dims[0] - 1) for c1 in range(case.dims[1] - 1)]


SKEWED_CHUNK = 4096  # points per workgroup of the sort's scatter kernels


def skewed_obs(case, dist, rng, **kw):
    """New observation arrays for `case` (one per axis, the case's element type) that are NOT spread evenly over the bins
    of the sorted multicubic path.  The sort key is the pair of saturation classes of axes 0 and 1 (`class_pairs`,
    `class_draw`); axes that a distribution does not name keep the point rule of `anisotropic_points`.  `count` is the
    number of points wherever the distribution does not fix it.

      one_pair(pair, count)       every point in the class pair `pair` (inside the grid);
      heavy(pair, c)              one point in every class pair, `c` points in all in `pair` (its own among them): P - 1 + c
                                  points for P pairs, shuffled;
      one_each(k[, empty])        exactly k points per class pair, shuffled; the pair `empty` gets none;
      ordered(count)              a batch by the point rule, stably sorted by (c0, c1);
      reversed(count)             the same batch in reverse order;
      striped(pairs, count)       every chunk of SKEWED_CHUNK points holds points of one pair, pairs[0] and pairs[1] in turn;
      outside0(count)             every point outside the grid along axis 0, below or above at random;
      one_outside                 3000 points of class 0 of axis 0 inside the grid and one below it, at index 1234;
      local_one(pair, c2[, c3], count)  every point in `pair`, of class c2 on axis 2 (and c3 on axis 3);
      local_ends(pair, count)     every point in `pair`, of the first or the last class of axis 2 at random;
      identical(which, count)     one point repeated: "interior" (inside an interior cell of every axis), "node" (a grid
                                  node on every axis), "beyond" (past the high corner on every axis);
      on_nodes(count)             every coordinate a node of its axis, drawn uniformly;
      nan0(count)                 a batch by the point rule, NaN on axis 0 for every point;
      half_nan0(count)            ... NaN on axis 0 for every second point of the second half."""
    grids, dt = case.grids, case.vals.dtype.type
    n = len(grids)
    pairs = class_pairs(case)

    def rule(count, skip=()):
        return [None if d in skip else anisotropic_points(grids[d], count, rng, dt) for d in range(n)]

    def in_pair(pair, count):
        obs = rule(count, skip=(0, 1))
        obs[0] = class_draw(grids[0], pair[0], count, rng, dt)
        obs[1] = class_draw(grids[1], pair[1], count, rng, dt)
        return obs

    def by_pair(counts):
        """counts[p] points in pair p, shuffled as a whole"""
        which = np.repeat(np.arange(len(pairs)), counts)
        rng.shuffle(which)
        obs = rule(which.size, skip=(0, 1))
        obs[0], obs[1] = np.empty(which.size, dtype=dt), np.empty(which.size, dtype=dt)
        for p, (c0, c1) in enumerate(pairs):
            at = which == p
            obs[0][at] = class_draw(grids[0], c0, int(at.sum()), rng, dt)
            obs[1][at] = class_draw(grids[1], c1, int(at.sum()), rng, dt)
        return obs

    if dist == "one_pair":
        return in_pair(kw["pair"], kw["count"])
    if dist == "heavy":
        counts = np.ones(len(pairs), dtype=np.int64)
        counts[pairs.index(tuple(kw["pair"]))] = kw["c"]
        return by_pair(counts)
    if dist == "one_each":
        counts = np.full(len(pairs), kw["k"], dtype=np.int64)
        if kw.get("empty") is not None:
            counts[pairs.index(tuple(kw["empty"]))] = 0
        return by_pair(counts)
    if dist in ("ordered", "reversed"):
        obs = rule(kw["count"])
        c = footprint_cells(dataclasses.replace(case, obs=obs))
        order = np.lexsort((c[1], c[0]))  # stable; c0 is the primary key
        if dist == "reversed":
            order = order[::-1]
        return [np.ascontiguousarray(o[order]) for o in obs]
    if dist == "striped":
        count = kw["count"]
        obs = rule(count, skip=(0, 1))
        obs[0], obs[1] = np.empty(count, dtype=dt), np.empty(count, dtype=dt)
        for k, lo in enumerate(range(0, count, SKEWED_CHUNK)):
            m = min(SKEWED_CHUNK, count - lo)
            c0, c1 = kw["pairs"][k % 2]
            obs[0][lo:lo + m] = class_draw(grids[0], c0, m, rng, dt)
            obs[1][lo:lo + m] = class_draw(grids[1], c1, m, rng, dt)
        return obs
    if dist == "outside0":
        count = kw["count"]
        obs = rule(count, skip=(0,))
        below = rng.random(count) < 0.5
        below[:2] = (True, False)
        obs[0] = np.where(below, class_draw(grids[0], 0, count, rng, dt, outside=True),
                          class_draw(grids[0], grids[0].size - 2, count, rng, dt, outside=True)).astype(dt)
        return obs
    if dist == "one_outside":
        obs = rule(3001, skip=(0,))
        obs[0] = class_draw(grids[0], 0, 3001, rng, dt)
        obs[0][1234] = class_draw(grids[0], 0, 1, rng, dt, outside=True)[0]
        return obs
    if dist == "local_one":
        obs = in_pair(kw["pair"], kw["count"])
        obs[2] = class_draw(grids[2], kw["c2"], kw["count"], rng, dt)
        if kw.get("c3") is not None:
            obs[3] = class_draw(grids[3], kw["c3"], kw["count"], rng, dt)
        return obs
    if dist == "local_ends":
        count = kw["count"]
        obs = in_pair(kw["pair"], count)
        first = rng.random(count) < 0.5
        first[:2] = (True, False)
        obs[2] = np.where(first, class_draw(grids[2], 0, count, rng, dt), class_draw(grids[2], grids[2].size - 2, count, rng, dt)).astype(dt)
        return obs
    if dist == "identical":
        which = kw["which"]
        if which == "interior":
            point = [class_draw(g, (g.size - 1) // 2, 1, rng, dt)[0] for g in grids]
        elif which == "node":
            point = [g[int(rng.integers(1, g.size - 1))] for g in grids]
        else:
            assert which == "beyond", which
            point = [class_draw(g, g.size - 2, 1, rng, dt, outside=True)[0] for g in grids]
        return [np.full(kw["count"], x, dtype=dt) for x in point]
    if dist == "on_nodes":
        return [np.ascontiguousarray(g[rng.integers(0, g.size, kw["count"])]) for g in grids]
    if dist in ("nan0", "half_nan0"):
        count = kw["count"]
        obs = rule(count)
        if dist == "nan0":
            obs[0][:] = np.nan
        else:
            obs[0][count // 2::2] = np.nan
        return obs
    raise ValueError(dist)


# ---- the k1 probe: tables on which 2 dy overflows in an end cell while 2 dy - k0 does not -------------------------------------------------
# The saturated classes of a multicubic axis, in the order of the probe's class codes 0..3; K1_MIDDLE marks the points of the cells
# between the end cells (class None).
K1_CLASSES = ("InsideLow", "OutsideLow", "InsideHigh", "OutsideHigh")
K1_MIDDLE = 4
# The table along the probed axis, in units of finfo(dtype).max: in both end cells max / 2 < |dy| < max (0.6 and 0.6; 0.6 and 0.55), and
# the three values an end cell's slopes are taken from keep one trend, so that 2 dy - k0 (1.2 - 0.46 = 0.74 on a uniform axis) is
# representable although 2 dy is not.  No difference of two values that a node forms reaches max.
K1_PROFILES = {4: (0.62, 0.02, -0.3, -0.9), 5: (0.62, 0.02, -0.3, -0.35, -0.9)}
# Intervals of the probed axis on a rectilinear grid, before scaling: the end intervals are the longer ones, because the interior
# cells' central difference divides an end cell's difference by the ratio (end interval) / (its neighbour) — 0.6 max / 1.25 stays in
# range, 0.6 max / 0.8 would not.
K1_INTERVALS = {4: (1.25, 1.0, 1.2), 5: (1.25, 1.0, 0.9, 1.15)}


def fma_sites():
    """tests/golden/fma_sites.json: the reference's fused multiply-add sites ("fused") and their unfused twins ("unfused")."""
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fma_sites.json")) as f:
        return json.load(f)


def k1_expected_fused(kind, n, cls):
    """From the site table: is `k1 <class>` (cls: index in K1_CLASSES) of multicubic `kind` fused under `fma` in the arm of the
    reference that serves N = n?  Exactly one row, fused or unfused, must say."""
    sites = fma_sites()
    hits = [status for status in ("fused", "unfused") for r in sites[status]
            if r["method"] == "cubic" and r["kind"] == kind and r["label"] == "k1 " + K1_CLASSES[cls] and r["n"][0] <= n <= r["n"][1]]
    assert len(hits) == 1, (kind, n, K1_CLASSES[cls], hits)
    return hits[0] == "fused"


def k1_assert_classes(values, cls, kind, n, fma, what=""):
    """Per class of the probe: finite where the table says fused (under `fma`) and in the middle cells, non-finite elsewhere."""
    values = np.asarray(values)
    for c in range(5):
        at = cls == c
        assert at.any()
        finite = np.isfinite(values[at])
        name = "middle" if c == K1_MIDDLE else K1_CLASSES[c]
        if c == K1_MIDDLE or (fma and k1_expected_fused(kind, n, c)):
            assert finite.all(), (what, name, "non-finite results", int((~finite).sum()))
        else:
            assert not finite.any(), (what, name, "finite results where 2 dy overflows unfused", int(finite.sum()))


def k1_probe_case(kind, shape, axis, dtype, per_class=24, seed=0, linearize=False):
    """(case, cls): a multicubic case whose table varies along `axis` only (K1_PROFILES times finfo(dtype).max), so that every
    node of another axis sees four equal values and hands one of them on unchanged, and the result is the 1-D node of `axis` on
    the profile.  `shape[axis]` is 4 or 5.  Along `axis`, `per_class` points in each of the four saturated classes — inside an
    end cell, a tenth of its width away from its ends; outside the grid by 0.005 to 0.04 of the end cell's width, where the
    exact value is still representable — and `per_class` in the cells between (cls == K1_MIDDLE), all shuffled; cls[i] is the
    index of point i's class in K1_CLASSES.  Every other axis: its own origin and step (regular) or mildly uneven intervals
    (rectilinear), coordinates uniform inside the grid."""
    from tests.kat import Case

    dtype = np.dtype(dtype)
    dt = dtype.type
    n = len(shape)
    na = shape[axis]
    rng = np.random.default_rng(77_000 + 1000 * seed + 100 * n + 10 * axis + (kind == "regular") + 2 * (dtype == np.float32))
    grids = []
    for d in range(n):
        start, step = 0.5 * d - 1.0, 0.25 + 0.125 * d
        if kind == "regular":
            g = start + step * np.arange(shape[d])
        else:
            h = np.array(K1_INTERVALS[na]) if d == axis else np.ones(shape[d] - 1)
            h = h * (1.0 + (0.06 if d == axis else 0.3) * (rng.random(h.size) - 0.5))
            g = start + step * np.concatenate([[0.0], np.cumsum(h)])
        g = g.astype(dtype)
        assert np.all(np.diff(g) > 0)
        grids.append(g)
    index = [None] * n
    index[axis] = slice(None)
    with np.errstate(over="raise"):
        profile = (np.array(K1_PROFILES[na]) * float(np.finfo(dtype).max)).astype(dtype)
    vals = np.ascontiguousarray(np.broadcast_to(profile[tuple(index)], shape)).ravel()
    g64 = grids[axis].astype(np.float64)
    w_lo, w_hi = g64[1] - g64[0], g64[-1] - g64[-2]
    u = lambda lo, hi: lo + (hi - lo) * rng.random(per_class)
    cell = rng.integers(1, na - 2, per_class)
    xa = np.concatenate([g64[0] + w_lo * u(0.1, 0.9), g64[0] - w_lo * u(0.005, 0.04), g64[-2] + w_hi * u(0.1, 0.9),
                         g64[-1] + w_hi * u(0.005, 0.04), g64[cell] + (g64[cell + 1] - g64[cell]) * u(0.1, 0.9)])
    cls = np.repeat(np.arange(5), per_class)
    order = rng.permutation(cls.size)
    obs = []
    for d in range(n):
        if d == axis:
            obs.append(np.ascontiguousarray(xa[order].astype(dtype)))
        else:
            lo, hi = float(grids[d][0]), float(grids[d][-1])
            obs.append((lo + (hi - lo) * (0.02 + 0.96 * rng.random(cls.size))).astype(dtype))
    case = Case(f"k1probe_{kind}_N{n}_a{axis}_{dtype.name}", "cubic", kind, grids, vals, obs, np.zeros(cls.size, dtype=dtype), 0.0,
                linearize=linearize)
    return case, cls[order]


def rel_err(a, b):
    """|a-b| / max(|b|, 1) — the reference's normalisation (test/test_multicubic_regular.py:97-100)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1.0)
