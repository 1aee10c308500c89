"""The generators of tests/test_unevenly_filled_bins_gpu.py, on the CPU: every distribution of tests/helpers.py::skewed_obs
delivers the occupancy it names — checked with `footprint_cells`, the rule the kernels' exact cell follows — and the oracle
is finite on all of them (rectilinear `nan0` is NaN everywhere, regular `nan0` / `half_nan0` raise at their first NaN).
No point is excluded and no tolerance is involved: downstream everything is a bit comparison, and this file is what tells
a kernel's fault from a generator's.  Every grid of the GPU file (family_runs.SKEWED_SHAPES), both kinds, both element
types."""

import numpy as np
import pytest

from tests import family_runs as fr
from tests.helpers import SKEWED_CHUNK, class_draw, class_pairs, footprint_cells, run_oracle, skewed_obs

pytestmark = [pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"]),
              pytest.mark.parametrize("kind", ["regular", "rectilinear"]),
              pytest.mark.parametrize("shape", fr.SKEWED_SHAPES, ids=lambda s: "x".join(map(str, s)))]


def _cells(case, obs):
    assert all(o.dtype == case.vals.dtype and o.shape == obs[0].shape for o in obs)
    return footprint_cells(fr.with_obs(case, obs))


def _finite(oracle, case, obs):
    for linearize in (False, True):
        for fma in (True, False):
            got = run_oracle(oracle, fr.with_obs(fr.skewed_case(case.kind, case.dims, case.vals.dtype.type, linearize), obs), fma)
            assert np.isfinite(got).all(), (linearize, fma)


def _histogram(case, cells):
    m1 = case.dims[1] - 1
    return np.bincount(cells[0] * m1 + cells[1], minlength=len(class_pairs(case)))


def test_class_draw(shape, kind, dtype):
    """Every class of every axis: inside the grid the points are of that class and strictly inside its cell; outside they
    lie strictly beyond the end and saturate into the first / last class."""
    case = fr.skewed_case(kind, shape, dtype)
    rng = fr.skewed_rng(shape, 0)
    for d, g in enumerate(case.grids):
        for c in range(g.size - 1):
            x = class_draw(g, c, 50, rng, dtype)
            assert x.dtype == dtype and (x > g[c]).all() and (x < g[c + 1]).all()
            obs = [np.full(50, h[1], dtype=dtype) for h in case.grids]
            obs[d] = x
            assert (_cells(case, obs)[d] == c).all(), (d, c)
        for c, beyond in ((0, lambda x: x < g[0]), (g.size - 2, lambda x: x > g[-1])):
            x = class_draw(g, c, 50, rng, dtype, outside=True)
            obs = [np.full(50, h[1], dtype=dtype) for h in case.grids]
            obs[d] = x
            assert beyond(x).all() and (_cells(case, obs)[d] == c).all(), (d, c)
            assert np.abs(x.astype(np.float64) - float(g[0] if c == 0 else g[-1])).max() <= 0.3001 * (float(g[-1]) - float(g[0]))


def test_one_pair_heavy_one_each(oracle, shape, kind, dtype):
    case = fr.skewed_case(kind, shape, dtype)
    pairs = class_pairs(case)
    rng = fr.skewed_rng(shape, 1)
    for pair in fr.swept_pairs(shape):
        obs = skewed_obs(case, "one_pair", rng, pair=pair, count=301)
        c = _cells(case, obs)
        assert obs[0].size == 301 and (c[0] == pair[0]).all() and (c[1] == pair[1]).all()
        assert all(np.unique(o).size > 16 for o in obs)  # not one point repeated (the narrowest f32 cells are some 40 ulps wide)
    _finite(oracle, case, skewed_obs(case, "one_pair", rng, pair=pairs[-1], count=3001))
    # heavy: `c` counts the pair's own point
    for pair in fr.heavy_pairs(shape):
        for count in (63, 64, 129):
            obs = skewed_obs(case, "heavy", rng, pair=pair, c=count)
            hist = _histogram(case, _cells(case, obs))
            at = pairs.index(pair)
            assert obs[0].size == len(pairs) - 1 + count and hist[at] == count and (np.delete(hist, at) == 1).all()
        _finite(oracle, case, obs)
    for k in (1, 2):
        obs = skewed_obs(case, "one_each", rng, k=k)
        assert (_histogram(case, _cells(case, obs)) == k).all() and obs[0].size == k * len(pairs)
        _finite(oracle, case, obs)
    empty = pairs[len(pairs) // 3]
    obs = skewed_obs(case, "one_each", rng, k=1, empty=empty)
    hist = _histogram(case, _cells(case, obs))
    assert hist[pairs.index(empty)] == 0 and hist.sum() == len(pairs) - 1 and hist.max() == 1
    _finite(oracle, case, obs)


def test_ordered_reversed_striped(oracle, shape, kind, dtype):
    case = fr.skewed_case(kind, shape, dtype)
    m1 = shape[1] - 1
    count = 20_011
    obs = skewed_obs(case, "ordered", fr.skewed_rng(shape, 2), count=count)
    back = skewed_obs(case, "reversed", fr.skewed_rng(shape, 2), count=count)
    c = _cells(case, obs)
    key = c[0] * m1 + c[1]
    assert (np.diff(key) >= 0).all() and np.unique(key).size > min(len(class_pairs(case)), count) // 4
    for o, b in zip(obs, back):  # the same batch, the other way round
        assert np.array_equal(fr.bits(o), fr.bits(b[::-1]))
    assert (obs[0] < case.grids[0][0]).any() and (obs[0] > case.grids[0][-1]).any()  # the point rule's extrapolating share is kept
    _finite(oracle, case, obs)
    two = (fr.swept_pairs(shape)[1], fr.swept_pairs(shape)[-1])
    obs = skewed_obs(case, "striped", fr.skewed_rng(shape, 3), pairs=two, count=count)
    c = _cells(case, obs)
    for k, lo in enumerate(range(0, count, SKEWED_CHUNK)):
        for d in (0, 1):
            assert (c[d][lo:lo + SKEWED_CHUNK] == two[k % 2][d]).all(), (k, d)
    _finite(oracle, case, obs)


def test_outside_local_identical_on_nodes(oracle, shape, kind, dtype):
    case = fr.skewed_case(kind, shape, dtype)
    g0 = case.grids[0]
    rng = fr.skewed_rng(shape, 4)
    obs = skewed_obs(case, "outside0", rng, count=3001)
    assert not ((obs[0] >= g0[0]) & (obs[0] <= g0[-1])).any() and (obs[0] < g0[0]).sum() > 1000 and (obs[0] > g0[-1]).sum() > 1000
    assert set(np.unique(_cells(case, obs)[0])) == {0, shape[0] - 2}
    _finite(oracle, case, obs)
    obs = skewed_obs(case, "one_outside", rng)
    below = obs[0] < g0[0]
    assert obs[0].size == 3001 and below.sum() == 1 and below[1234] and (_cells(case, obs)[0] == 0).all() and (obs[0][~below] > g0[0]).all()
    _finite(oracle, case, obs)
    if len(shape) >= 3:
        pair = fr.heavy_pairs(shape)[2]
        for c2 in range(shape[2] - 1):
            c3 = (c2 % (shape[3] - 1)) if len(shape) == 4 else None
            obs = skewed_obs(case, "local_one", rng, pair=pair, c2=c2, c3=c3, count=501)
            c = _cells(case, obs)
            assert (c[0] == pair[0]).all() and (c[1] == pair[1]).all() and (c[2] == c2).all()
            assert c3 is None or (c[3] == c3).all()
        _finite(oracle, case, obs)
        obs = skewed_obs(case, "local_ends", rng, pair=pair, count=3001)
        c = _cells(case, obs)
        assert (c[0] == pair[0]).all() and (c[1] == pair[1]).all() and set(np.unique(c[2])) == {0, shape[2] - 2}
        _finite(oracle, case, obs)
    for which in ("interior", "node", "beyond"):
        obs = skewed_obs(case, "identical", rng, which=which, count=3001)
        assert all(o.size == 3001 and np.unique(o).size == 1 for o in obs)
        for o, g in zip(obs, case.grids):
            x = o[0]
            if which == "interior":
                assert g[1] < x < g[-2] and x not in g
            elif which == "node":
                assert x in g[1:-1]
            else:
                assert x > g[-1]
        _finite(oracle, case, obs)
    obs = skewed_obs(case, "on_nodes", rng, count=3001)
    for o, g in zip(obs, case.grids):
        assert np.isin(o, g).all() and np.unique(o).size == g.size
    _finite(oracle, case, obs)


def test_nan_batches(oracle, shape, kind, dtype):
    """Rectilinear grids never fail per point: NaN propagates.  Regular grids stop at the first NaN, like the reference."""
    from oracle.pyoracle import OracleError

    case = fr.skewed_case(kind, shape, dtype)
    count = 3001
    for dist, first in (("nan0", 0), ("half_nan0", count // 2)):
        obs = skewed_obs(case, dist, fr.skewed_rng(shape, 5), count=count)
        nan = np.isnan(obs[0])
        assert all(np.isfinite(o).all() for o in obs[1:]) and np.flatnonzero(nan)[0] == first
        if dist == "nan0":
            assert nan.all()
        else:
            assert not nan[:first].any() and nan[first::2].all() and not nan[first + 1::2].any()
        if kind == "rectilinear":
            got = run_oracle(oracle, fr.with_obs(case, obs), True)
            assert np.array_equal(np.isnan(got), nan) and np.isfinite(got[~nan]).all()
        else:
            with pytest.raises(OracleError) as err:
                run_oracle(oracle, fr.with_obs(case, obs), True)
            assert err.value.first_bad == first
