"""The anisotropic workload (tests/helpers.py::anisotropic_case) on the CPU: what the generator promises, the oracle
against exact-rational values at that geometry (N = 2..4; tests/test_oracle_exact.py stops at N = 3 on O(1) axes), and
the reason the generator exists — a per-axis quantity taken from the wrong axis is invisible on `synthetic_case` and
changes nearly every point here."""

import numpy as np
import pytest

from oracle import exact_rational
from tests.helpers import ANISO_AXES, anisotropic_axis, anisotropic_case, run_oracle, synthetic_case
from tests.test_golden import EXACT_K

SHAPES = ([9, 7], [6, 5, 7], [5, 6, 4, 5])
NOBS = 120
FLAVOURS = [("linear", False), ("cubic", False), ("cubic", True)]

_exact = {}


def _case_and_exact(method, linearize, kind, shape, dtype):
    key = (method, linearize, kind, tuple(shape), np.dtype(dtype).name)
    if key not in _exact:
        c = anisotropic_case(method, kind, shape, NOBS, 7100 + len(shape), dtype, linearize=linearize)
        ex = exact_rational.evaluate_with_condition(method, kind, c.grids, c.vals, c.obs, linearize, c.starts, c.steps)
        _exact[key] = (c, np.array([float(v) for v, _ in ex]), np.array([float(s) for _, s in ex]))
    return _exact[key]


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,linearize", FLAVOURS, ids=["linear", "cubic", "cubic_lin"])
def test_oracle_within_exact_rational_bound(oracle, method, linearize, kind, shape, dtype, fma):
    """The bound of tests/test_golden.py: EXACT_K u scale, scale = sum|w||v| + sum_d (|x_d| + max|g_d|) |dI/dx_d|.
    Measured: the worst ratio err / (u scale) over these 72 combinations is 0.03 (cubic rectilinear, N = 4),
    typical 1e-3: the scale carries |x_d| / h_d, which is 3e4 on axis 0 and 40 on axis 2, while x - g[i] is exact for
    coordinates this close to their node.  The relative figures 1e-12 / 1e-10 are not asserted: on the clustered axes
    cubic-rectilinear is ill-conditioned and only the condition-aware bound is fair.  With about 500x of slack this tier is
    weak on this geometry — it catches a wrong term, not a wrong rounding; the bit-for-bit comparisons with the oracle
    (tests/test_anisotropic_gpu.py, tests/test_golden.py) carry the tests."""
    c, exact, scale = _case_and_exact(method, linearize, kind, shape, dtype)
    got = run_oracle(oracle, c, fma)
    u = np.finfo(dtype).eps / 2
    ratio = np.abs(got.astype(np.float64) - exact) / (u * scale)
    print(f"{c.name} {np.dtype(dtype).name} fma={fma} lin={linearize}: worst ratio {ratio.max():.3g}")
    assert np.all(ratio <= EXACT_K), (c.name, float(ratio.max()))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["linear", "cubic", "nearest"])
def test_starts_of_two_axes_swapped(oracle, method, dtype):
    """Why this generator exists: with `starts` permuted between two axes a regular `synthetic_case` gives the very same
    bits (every start is -1), an `anisotropic_case` differs at more than 90 % of its points."""
    fn = {"linear": oracle.linear_regular, "nearest": oracle.nearest_regular,
          "cubic": lambda *a, **k: oracle.cubic_regular(*a[:4], False, *a[4:], **k)}[method]

    def both(c):
        swapped = c.starts.copy()
        swapped[[0, 2]] = swapped[[2, 0]]
        a, b = np.zeros(c.obs[0].size, dtype=dtype), np.zeros(c.obs[0].size, dtype=dtype)
        fn(c.dims, c.starts, c.steps, c.vals, c.obs, a)
        fn(c.dims, swapped, c.steps, c.vals, c.obs, b)
        return a, b

    a, b = both(synthetic_case(method, "regular", 3, [6, 5, 7], 2000, 31, dtype))
    assert np.array_equal(a, b)
    a, b = both(anisotropic_case(method, "regular", [6, 5, 7], 2000, 31, dtype))
    assert np.mean(a != b) > 0.9, float(np.mean(a != b))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_generator_geometry(dtype):
    """What the generator promises: the table's origins and steps (doubled per cycle), rectilinear axes with the regular
    axis's ends, interval ratios far from 1, a cluster of twenty short intervals from 24 nodes on, and points that hit
    exact nodes, both ends, the neighbours just outside them, the short intervals and the extrapolation range."""
    rng = np.random.default_rng(5)
    for d in range(8):
        start, step = ANISO_AXES[d % 6]
        step *= 2 ** (d // 6)
        for n in (2, 5, 9, 30, 70):
            reg = anisotropic_axis(d, n, "regular", dtype, rng)
            assert reg[0] == dtype(start) and np.allclose(np.diff(reg.astype(np.float64)), step, rtol=2e-3)
            g = anisotropic_axis(d, n, "rectilinear", dtype, rng)
            assert g.size == n and g[0] == dtype(start) and g[-1] == dtype(start + step * (n - 1))
            h = np.diff(g.astype(np.float64))
            if n < 9:
                continue
            if d % 3 == 0:
                assert 30 < h[-1] / h[0] < 90  # 1.7^7 = 41 on 9 nodes, 1.7^8 = 70 beyond
            elif d % 3 == 1:
                assert 50 < h[0] / h[-1] < 150  # 0.55^-7 = 66 on 9 nodes, 0.55^-8 = 120 beyond
            else:
                short = h < 5e-3 * h.max()
                assert short.sum() == (20 if n >= 24 else 2) and np.ptp(np.flatnonzero(short)) == short.sum() - 1
    for kind in ("regular", "rectilinear"):
        c = anisotropic_case("linear", kind, [30, 9, 7], 2000, 3, dtype)
        assert c.vals.dtype == dtype and c.vals.size == 30 * 9 * 7 and np.abs(c.vals).max() <= 1
        assert np.array_equal(c.starts, [g[0] for g in c.grids]) and np.array_equal(c.steps, [g[1] - g[0] for g in c.grids])
        for g, x in zip(c.grids, c.obs):
            assert x.dtype == dtype and x.size == 2000
            assert np.isin(x, g).sum() >= min(g.size, 12) and g[0] in x and g[-1] in x
            assert np.nextafter(g[0], dtype(-np.inf)) in x and np.nextafter(g[-1], dtype(np.inf)) in x
            span = float(g[-1]) - float(g[0])
            assert x.min() < g[0] - 0.1 * span and x.max() > g[-1] + 0.1 * span
            cell = np.searchsorted(g, x[(x > g[0]) & (x < g[-1])], side="right") - 1
            assert np.bincount(cell, minlength=g.size - 1).min() >= 5  # every cell, however short
    # the same seed gives the same case
    a, b = (anisotropic_case("cubic", "rectilinear", [6, 5, 7], 300, 9, dtype) for _ in range(2))
    assert all(np.array_equal(p, q) for p, q in zip(a.grids + a.obs + [a.vals], b.grids + b.obs + [b.vals]))
