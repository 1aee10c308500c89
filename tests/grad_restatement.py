"""numpy restatement of the multilinear value-and-gradient definition (DESIGN.md "Gradients"), vectorised over the
observation points: both grid kinds, f64 / f32, both `fma` flavours, N = 1..8.

Per point, with every operation rounded in the element type:
  cell, t   the reference's operations — regular: floor((x - start) / step) clamped to 0..n-2 (get_loc,
            multilinear/regular.rs:414-425), index_zero_loc = start + step * i (fused in the fma flavour for N <= 6, the
            flattened arm; never for N = 7, 8, the recursive arm), t = (x - index_zero_loc) / step; rectilinear:
            partition_point(g < x) - 1 clamped, t = (x - x0) / (x1 - x0) (rectilinear.rs:310-313, :353-370)
  value     the corners reduced over dimension 0 first, N - 1 last, with lerp(t, y0, y1): dy = y1 - y0, then
            t.mul_add(dy, y0) or y0 + t * dy (regular.rs:347-403)
  grad[d]   W[c'] = V[c' | 1 << d] - V[c'], reduced over the dimensions e != d in ascending order with the same lerp,
            divided by steps[d] or by the point's x1 - x0.

The fused step is tests.one_dim_restatement.fma_vec (pinned to a single-rounding fma by tests/test_one_dim_cpu.py).
"""

from __future__ import annotations

import numpy as np

from tests.one_dim_restatement import fma_vec


def _mul_add(a, b, c, fma, dtype):
    """a.mul_add(b, c) with the `fma` feature, a * b + c (two roundings) without."""
    if fma:
        return np.asarray(fma_vec(a, b, c, dtype), dtype=dtype).reshape(np.shape(c))
    with np.errstate(all="ignore"):
        return (a * b).astype(dtype) + c


def _lerp(t, y0, y1, fma, dtype):
    with np.errstate(all="ignore"):
        dy = (y1 - y0).astype(dtype)
    # multilinear/regular.rs:385, :402, multilinear/regular_recursive.rs:384, multilinear/rectilinear.rs:321, :344,
    # multilinear/rectilinear_recursive.rs:331
    return _mul_add(t, dy, y0, fma, dtype).astype(dtype)


def locate_regular(x, start, step, n, fma, fused_index, dtype):
    """(cell, t, width, representable) of one dimension of a regular grid."""
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=dtype)
    start, step = dtype.type(start), dtype.type(step)
    with np.errstate(all="ignore"):
        floc = np.floor(((x - start) / step).astype(dtype))
        ok = (floc >= -(2.0**63)) & (floc < 2.0**63)  # isize::from: NaN and +-inf fail too
        loc = np.clip(np.where(ok, floc, 0.0), 0.0, float(n - 2)).astype(np.int64)
        locf = loc.astype(dtype)
        if fma and fused_index:  # multilinear/regular.rs:337
            izl = np.asarray(fma_vec(np.full(x.shape, step, dtype=dtype), locf, np.full(x.shape, start, dtype=dtype), dtype),
                             dtype=dtype).reshape(x.shape)
        else:
            izl = ((step * locf).astype(dtype) + start).astype(dtype)
        t = ((x - izl).astype(dtype) / step).astype(dtype)
    return loc, t, np.full(x.shape, step, dtype=dtype), ok


def locate_rectilinear(x, g, dtype):
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=dtype)
    g = np.asarray(g, dtype=dtype)
    n = g.size
    with np.errstate(all="ignore"):
        # partition_point(g < x) on a sorted axis: the count of coordinates below x (NaN: 0)
        cnt = np.searchsorted(g, x, side="left")
        cnt = np.where(np.isnan(x), 0, cnt)
        loc = np.clip(cnt - 1, 0, n - 2).astype(np.int64)
        x0, x1 = g[loc], g[loc + 1]
        width = (x1 - x0).astype(dtype)
        t = ((x - x0).astype(dtype) / width).astype(dtype)
    return loc, t, width, np.ones(x.shape, dtype=bool)


def _reduce(level, ts, fma, dtype):
    """`level`: list of 2^m arrays indexed by the corner mask over the dimensions of `ts` (bit k = offset along
    ts[k]'s dimension); reduced in ascending k."""
    for t in ts:
        level = [_lerp(t, level[2 * j], level[2 * j + 1], fma, dtype) for j in range(len(level) // 2)]
    return level[0]


def eval_grad(kind, grid_args, vals, obs, fma=True, dtype=None):
    """(out, grad, ok): value (n,), gradient (N, n), and per point whether the reference can evaluate it (regular grids:
    the first False is the first failing index; what is returned for such a point is unspecified).

    kind == "regular": grid_args = (dims, starts, steps); kind == "rectilinear": grid_args = grids."""
    dtype = np.dtype(dtype or np.asarray(vals).dtype)
    vals = np.asarray(vals, dtype=dtype).ravel()
    obs = [np.asarray(o, dtype=dtype).ravel() for o in obs]
    N = len(obs)
    npts = obs[0].size
    if kind == "regular":
        dims, starts, steps = grid_args
        dims = [int(v) for v in dims]
        located = [locate_regular(obs[d], starts[d], steps[d], dims[d], fma, N <= 6, dtype) for d in range(N)]
    else:
        dims = [len(g) for g in grid_args]
        located = [locate_rectilinear(obs[d], grid_args[d], dtype) for d in range(N)]
    assert vals.size == int(np.prod(dims))
    strides = [int(np.prod(dims[d + 1:], dtype=np.int64)) for d in range(N)]
    ok = np.ones(npts, dtype=bool)
    base = np.zeros(npts, dtype=np.int64)
    for d in range(N):
        base += located[d][0] * strides[d]
        ok &= located[d][3]
    ts = [located[d][1] for d in range(N)]
    # corners V[c], bit d of c = offset along dimension d (regular.rs:362)
    V = []
    for c in range(1 << N):
        off = sum(strides[d] for d in range(N) if (c >> d) & 1)
        V.append(vals[base + off])
    out = _reduce(V, ts, fma, dtype)
    grad = np.empty((N, npts), dtype=dtype)
    for d in range(N):
        others = [e for e in range(N) if e != d]
        W = []
        for m in range(1 << (N - 1)):
            c = 0
            for k, e in enumerate(others):
                c |= ((m >> k) & 1) << e
            with np.errstate(all="ignore"):
                W.append((V[c | (1 << d)] - V[c]).astype(dtype))
        s = _reduce(W, [ts[e] for e in others], fma, dtype)
        with np.errstate(all="ignore"):
            grad[d] = (s / located[d][2]).astype(dtype)
    return out.astype(dtype), grad, ok


def eval_grad_case(case, fma=True, dtype=None):
    """The same for a tests.kat.Case (multilinear)."""
    dtype = np.dtype(dtype or case.vals.dtype)
    if case.kind == "regular":
        args = (case.dims, np.asarray(case.starts, dtype=dtype), np.asarray(case.steps, dtype=dtype))
    else:
        args = [np.asarray(g, dtype=dtype) for g in case.grids]
    return eval_grad(case.kind, args, case.vals, case.obs, fma=fma, dtype=dtype)
