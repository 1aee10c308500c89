"""numpy restatement of the multicubic value-and-gradient definition (DESIGN.md "Multicubic gradients"), vectorised over the
observation points: both grid kinds, f64 / f32, both `fma` flavours, `linearize_extrapolation` on and off, N = 1..8.

Per point, with every operation rounded in the element type, on the arm of the reference the value path runs (the
flattened arm of multicubic/regular.rs / rectilinear.rs for N <= 4, the recursive arm for N >= 5; the two differ in three
fused sites, `k1_plain`, `fma_linear` and `k1_fused` below):

  per dimension   footprint origin, saturation class (None / Low / High), the linearized flag (outside the grid with
                  linearize_extrapolation) and the local coordinate tt — regular: floc = floor((x - start) / step),
                  origin = clamp(floc - 1, 0, n - 4), t = (x - (start + step * (origin + 1))) / step (never fused), tt = t,
                  -t (Low), t - 1 (High); rectilinear: origin from partition_point(g < x) - 2, the spacing ratios of the
                  non-uniform central difference, t = (x - g1) / h12, -(x - g1) / h01 (Low), (x - g2) / h23 (High)
  node            y0, dy, k0, k1 of the class, then c1, c2, c3 of normalized_hermite_spline (multicubic/mod.rs:72-91);
                  I = ((c3 tt + c2) tt + c1) tt + y0, linearized: k1.mul_add(tt - 1, y1)
                  D = (e3 tt + e2) tt + c1 with e2 = c2 + c2, e3 = ((1 + 1) + 1) * c3; linearized: k1
  value           the 4^N footprint reduced over dimension 0 first, N - 1 last, with I
  grad[d]         levels e < d: the value's partial results; level d: D; levels e > d: I; then
                  (Low along d ? -s : s) / h_d, h_d = steps[d] or the spacing t was divided by.

The fused step is tests.one_dim_restatement.fma_vec (pinned to a single-rounding fma by tests/test_one_dim_cpu.py).
"""

from __future__ import annotations

import numpy as np

from tests.one_dim_restatement import fma_vec

NONE, LOW, HIGH = 0, 1, 2


def _fma(a, b, c, dtype):
    shape = np.broadcast(np.asarray(a), np.asarray(b), np.asarray(c)).shape
    return np.asarray(fma_vec(a, b, c, dtype), dtype=dtype).reshape(shape)


def _mul_add(a, b, c, fma, dtype):
    """a.mul_add(b, c) with the `fma` feature, a * b + c (two roundings) without."""
    if fma:
        return _fma(a, b, c, dtype)
    return (a * b).astype(dtype) + c


def locate_regular(x, start, step, n, linearize, recursive, dtype):
    dtype = np.dtype(dtype)
    T = dtype.type
    x = np.asarray(x, dtype=dtype)
    start, step = T(start), T(step)
    floc = np.floor(((x - start) / step).astype(dtype))
    ok = (floc > -(2.0**63)) & (floc < 2.0**63)  # isize::from, and `- 1` must not overflow; NaN and +-inf fail too
    loc = np.clip(np.where(ok, floc, T(0)) - T(1), 0.0, float(n - 4)).astype(np.int64)
    low = floc <= 0
    high = ~low & (floc >= T(n - 2))
    outside = (floc < 0) | (floc > T(n - 2))
    sat = np.where(low, LOW, np.where(high, HIGH, NONE))
    iol = ((step * (loc + 1).astype(dtype)).astype(dtype) + start).astype(dtype)  # index_one_loc: never fused
    t = ((x - iol).astype(dtype) / step).astype(dtype)
    tt = np.where(low, -t, np.where(high, t - T(1), t)).astype(dtype)
    return dict(kind="regular", loc=loc, sat=sat, tt=tt, linear=outside & bool(linearize), k1_plain=low & outside & bool(recursive),
                width=np.full(x.shape, step, dtype=dtype), ok=ok)


def locate_rectilinear(x, g, linearize, recursive, dtype):
    dtype = np.dtype(dtype)
    T = dtype.type
    one = T(1)
    x = np.asarray(x, dtype=dtype)
    g = np.asarray(g, dtype=dtype)
    n = g.size
    cnt = np.searchsorted(g, x, side="left")  # partition_point(g < x) on a sorted axis (NaN: 0)
    cnt = np.where(np.isnan(x), 0, cnt)
    iloc = cnt - 2
    loc = np.clip(iloc, 0, n - 4).astype(np.int64)
    low = iloc <= -1
    high = ~low & (iloc >= n - 3)
    outside = (iloc == -2) | (iloc == n - 2)
    sat = np.where(low, LOW, np.where(high, HIGH, NONE))
    g0, g1, g2, g3 = g[loc], g[loc + 1], g[loc + 2], g[loc + 3]
    h12 = g2 - g1
    # None: (hA, hB) = (r0, 1) for k0 and (1, r1) for k1
    h01, h23 = g1 - g0, g3 - g2
    r0n = h01 / h12
    a0n, c0n = r0n / (r0n + one), one / (one + r0n)
    r1n = h23 / h12
    a1n, c1n = one / (one + r1n), r1n / (r1n + one)
    tn = (x - g1) / h12
    # Low: r0 = h12 / h01, a0 = 1 / (1 + r0), c0 = r0 / (r0 + 1), t = -(x - g1) / h01; High: r0 = h12 / h23, a0 = r0 / (r0 + 1), ...
    ho = np.where(low, h01, h23)
    r0s = h12 / ho
    wr, w1 = r0s / (r0s + one), one / (one + r0s)
    num = x - np.where(low, g1, g2)
    ts = np.where(low, -num, num) / ho
    none = sat == NONE
    sel = lambda a, b: np.where(none, a, b).astype(dtype)
    return dict(kind="rectilinear", loc=loc, sat=sat, tt=sel(tn, ts), linear=outside & bool(linearize),
                fma_linear=bool(recursive), k1_fused=(low | high) & ~outside & bool(recursive), r0=sel(r0n, r0s), a0=sel(a0n, np.where(low, w1, wr)), c0=sel(c0n, np.where(low, wr, w1)),
                r1=sel(r1n, one), a1=sel(a1n, one), c1=sel(c1n, one), width=sel(h12, ho), ok=np.ones(x.shape, dtype=bool))


def _hermite(tt, y0, dy, k0, k1, fma, dtype):
    """(I, D) of the Hermite arms: normalized_hermite_spline's coefficients, Horner for both."""
    T = np.dtype(dtype).type
    a = k0 - dy
    b = -k1 + dy
    c1 = dy + a
    c2 = b - (a + a)
    c3 = a - b
    three = (T(1) + T(1)) + T(1)
    e2 = c2 + c2
    e3 = three * c3
    if fma:
        val = _fma(_fma(_fma(c3, tt, c2, dtype), tt, c1, dtype), tt, y0, dtype)  # multicubic/mod.rs:89
        der = _fma(_fma(e3, tt, e2, dtype), tt, c1, dtype)
    else:
        val = y0 + tt * (c1 + tt * (c2 + tt * c3))
        der = c1 + tt * (e2 + tt * e3)
    return val, der


def node(dim, v0, v1, v2, v3, fma, dtype):
    """(I, D) of one 1-D node of dimension state `dim` on the four inputs."""
    dtype = np.dtype(dtype)
    T = dtype.type
    one, two = T(1), T(2)
    low, high = dim["sat"] == LOW, dim["sat"] == HIGH
    tt = dim["tt"]
    if dim["kind"] == "regular":
        y0 = np.where(high, v2, v1)
        ya = np.where(low, v0, np.where(high, v3, v2))
        dy = ya - y0
        cd = np.where(high, v3 - v1, v2 - v0)
        k0 = cd / two
        k0 = np.where(low, -k0, k0)
        k1n = (v3 - v1) / two
        # multicubic/regular.rs:528, :549, :583, :605 and multicubic/regular_recursive.rs:519, :570, :592
        k1e = _mul_add(two, dy, -k0, fma, dtype)
        if fma:
            k1e = np.where(dim["k1_plain"], two * dy - k0, k1e)  # multicubic/regular_recursive.rs:536
        k1 = np.where(low | high, k1e, k1n)
        lin_val = _mul_add(k1, tt - one, ya, fma, dtype)  # multicubic/regular.rs:560, :616, multicubic/regular_recursive.rs:547, :603
    else:
        r0, a0, c0, r1, a1, c1 = (dim[k] for k in ("r0", "a0", "c0", "r1", "a1", "c1"))

        def combine(a, b, c, dd):
            if fma:
                return _fma(a, b, c * dd, dtype)  # multicubic/mod.rs:115
            return a * b + c * dd

        f01, f12, f23 = v1 - v0, v2 - v1, v3 - v2
        # None: k0 = cd_unit_b(v0, v1, v2), k1 = cd_unit_a(v1, v2, v3)
        k0n = combine(a0, f12, c0, f01 / r0)
        k1n = combine(a1, f23 / r1, c1, f12)
        # Low: k0 = -cd_unit_a(v0, v1, v2); High: k0 = cd_unit_b(v1, v2, v3)
        q = f12 / r0
        ks = combine(a0, np.where(low, q, f23), c0, np.where(low, f01, q))
        k0s = np.where(low, -ks, ks)
        dys = np.where(low, v0 - v1, f23)
        k1s = two * dys - k0s  # multicubic/rectilinear.rs:471, :493, :515, :532, multicubic/rectilinear_recursive.rs:469, :519: never fused
        if fma:  # the recursive arm's InsideLow and InsideHigh: multicubic/rectilinear_recursive.rs:447, :502
            k1s = np.where(dim["k1_fused"], _fma(two, dys, -k0s, dtype), k1s)
        none = ~(low | high)
        y0 = np.where(high, v2, v1)
        ya = np.where(low, v0, v3)
        dy = np.where(none, f12, dys)
        k0 = np.where(none, k0n, k0s)
        k1 = np.where(none, k1n, k1s)
        if fma and dim["fma_linear"]:
            lin_val = _fma(k1, tt - one, ya, dtype)  # multicubic/rectilinear_recursive.rs:482, :532
        else:
            lin_val = ya + k1 * (tt - one)  # multicubic/rectilinear.rs:500, :539: never fused
    val, der = _hermite(tt, y0, dy, k0, k1, fma, dtype)
    lin = dim["linear"]
    return np.where(lin, lin_val, val).astype(dtype), np.where(lin, k1, der).astype(dtype)


def eval_grad(kind, grid_args, vals, obs, linearize=True, fma=True, dtype=None):
    """(out, grad, ok): value (n,), gradient (N, n), and per point whether the reference can evaluate it (regular grids:
    the first False is the first failing index; what is returned for such a point is unspecified).

    kind == "regular": grid_args = (dims, starts, steps); kind == "rectilinear": grid_args = grids."""
    dtype = np.dtype(dtype or np.asarray(vals).dtype)
    vals = np.asarray(vals, dtype=dtype).ravel()
    obs = [np.asarray(o, dtype=dtype).ravel() for o in obs]
    N = len(obs)
    npts = obs[0].size
    recursive = N >= 5
    with np.errstate(all="ignore"):
        if kind == "regular":
            dims, starts, steps = grid_args
            dims = [int(v) for v in dims]
            dim = [locate_regular(obs[d], starts[d], steps[d], dims[d], linearize, recursive, dtype) for d in range(N)]
        else:
            dims = [len(g) for g in grid_args]
            dim = [locate_rectilinear(obs[d], grid_args[d], linearize, recursive, dtype) for d in range(N)]
        assert vals.size == int(np.prod(dims))
        strides = [int(np.prod(dims[d + 1:], dtype=np.int64)) for d in range(N)]
        ok = np.ones(npts, dtype=bool)
        base = np.zeros(npts, dtype=np.int64)
        for d in range(N):
            base += dim[d]["loc"] * strides[d]
            ok &= dim[d]["ok"]
        # leaves V[c], base-4 digit d of c = offset along dimension d (regular.rs:368-421: dimension 0 innermost)
        level = []
        for c in range(4**N):
            off = sum(((c >> (2 * d)) & 3) * strides[d] for d in range(N))
            level.append(vals[base + off])
        partial = {}  # d -> the partial results of component d at the current level
        for e in range(N):
            nxt = {d: [node(dim[e], *lst[4 * j:4 * j + 4], fma, dtype)[0] for j in range(len(lst) // 4)] for d, lst in partial.items()}
            both = [node(dim[e], *level[4 * j:4 * j + 4], fma, dtype) for j in range(len(level) // 4)]
            level = [b[0] for b in both]
            nxt[e] = [b[1] for b in both]
            partial = nxt
        out = level[0].astype(dtype)
        grad = np.empty((N, npts), dtype=dtype)
        for d in range(N):
            s = partial[d][0]
            s = np.where(dim[d]["sat"] == LOW, -s, s).astype(dtype)
            grad[d] = (s / dim[d]["width"]).astype(dtype)
    return out, grad, ok


def eval_grad_case(case, fma=True, dtype=None):
    """The same for a tests.kat.Case (multicubic; the case's `linearize`)."""
    dtype = np.dtype(dtype or case.vals.dtype)
    if case.kind == "regular":
        args = (case.dims, np.asarray(case.starts, dtype=dtype), np.asarray(case.steps, dtype=dtype))
    else:
        args = [np.asarray(g, dtype=dtype) for g in case.grids]
    return eval_grad(case.kind, args, case.vals, case.obs, linearize=case.linearize, fma=fma, dtype=dtype)
