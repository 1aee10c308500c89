"""interpn::one_dim on the MI355X (k_one_dim.hip): bit-for-bit parity with the CPU restatement
(tests/one_dim_restatement.py, pinned by tests/test_one_dim_cpu.py) on both evaluation paths, the error contract of
regular grids, degenerate grids, a full-size batch, and the multi-handle forms."""

import numpy as np
import pytest

from tests import one_dim_restatement as R

pytestmark = pytest.mark.gpu

KNOTS = [2, 3, 10, 77, 1000, 4096, 65536, 1_000_003]


def _bits_equal(a, b):
    """Equal values with equal signs (so -0 != +0); any two NaNs count as equal."""
    a, b = np.asarray(a), np.asarray(b)
    eq = (a == b) & (np.signbit(a) == np.signbit(b))
    return bool(np.all(eq | (np.isnan(a) & np.isnan(b))))


def _grid(kind, n, dtype, rng):
    vals = rng.normal(size=n).astype(dtype)
    if kind == "regular":
        start, step = dtype(-1.25), dtype(2.5 / (n - 1))
        stop = R.regular_stop(start, step, n, dtype)
        knots = (start + step * np.arange(n).astype(dtype)).astype(dtype)
        return dict(start=start, step=step, vals=vals), start, stop, knots
    g = np.cumsum(rng.uniform(0.1, 1.0, size=n)).astype(dtype) - dtype(n * 0.3)
    g = np.unique(g)
    if len(g) < n:  # f32 rounding merged two coordinates: keep the axis strictly increasing
        g = np.sort(rng.uniform(-1, 1, size=n)).astype(np.float64).astype(dtype)
        g = np.linspace(-1.0, 1.0, n).astype(dtype) if len(np.unique(g)) < n else g
    return dict(grid=g, vals=vals), g[0], g[-1], g


def _points(kind, dtype, start, stop, knots, rng, m=3000):
    """The reference tests' distribution (one_dim/hold.rs:137-139: normal samples scaled by 2 (stop - start) and shifted
    by 2 start, most of them outside), points inside, knots, midpoints, the ends +- 1 ulp, +-0 and a huge value; NaN and
    +-inf on rectilinear grids only (on regular grids they are errors)."""
    span = float(stop) - float(start)
    pts = [rng.normal(size=m) * 2 * span + 2 * float(start), rng.uniform(float(start), float(stop), size=m)]
    sel = knots if len(knots) <= 400 else knots[rng.integers(0, len(knots), 400)]
    pts.append(sel.astype(np.float64))
    mids = (sel[:-1].astype(np.float64) + sel[1:].astype(np.float64)) / 2 if len(sel) > 1 else sel
    pts.append(np.asarray(mids, dtype=np.float64))
    ends = []
    for v in (dtype(start), dtype(stop)):
        ends += [v, np.nextafter(v, dtype(np.inf)), np.nextafter(v, dtype(-np.inf))]
    pts.append(np.array(ends, dtype=np.float64))
    # huge values: 1e300 on rectilinear grids; on regular grids a value whose cell still converts to isize
    pts.append(np.array([0.0, -0.0, 1e12, -1e12] + ([1e300, -1e300] if kind == "rectilinear" else [])))
    with np.errstate(over="ignore"):  # 1e300 is +inf in f32
        x = np.concatenate(pts).astype(dtype)
        if kind == "rectilinear":
            x = np.concatenate([x, np.array([np.nan, np.inf, -np.inf], dtype=dtype)])
    rng.shuffle(x)
    return x


def _create(method, kind, args, dtype, fma):
    from interpn_amd import Interpolator

    if kind == "regular":
        return Interpolator.grid1d_regular(method, args["start"], args["step"], args["vals"], device=0, dtype=dtype, fma=fma)
    return Interpolator.grid1d_rectilinear(method, args["grid"], args["vals"], device=0, dtype=dtype, fma=fma)


def _eval_both(it, x):
    import torch

    host = np.full(len(x), -7.0, dtype=x.dtype)
    it.eval_host([x], host)
    dev = it.eval_tensors([torch.from_numpy(x).to("cuda:0")])
    it.finish()
    return host, dev.cpu().numpy()


@pytest.mark.parametrize("n", KNOTS)
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_parity_with_restatement(n, kind, dtype):
    rng = np.random.default_rng(n * 7 + (kind == "regular") + (dtype == np.float32) * 3)
    args, start, stop, knots = _grid(kind, n, dtype, rng)
    x = _points(kind, dtype, start, stop, knots, rng)
    for method in R.METHODS:
        for fma in (True, False):
            want, bad = R.eval(method, kind, dtype, fma, x, **args)
            assert bad is None
            it = _create(method, kind, args, dtype, fma)
            host, dev = _eval_both(it, x)
            assert "k_one_dim<" in it.kernel_name()
            assert _bits_equal(host, want), (method, fma, np.flatnonzero(~np.isclose(host, want, equal_nan=True))[:5])
            assert _bits_equal(dev, want), (method, fma)
            it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bad_value", ["nan", "inf", "-inf", "huge"])
def test_regular_errors_abort_at_first_bad_point(dtype, bad_value):
    import torch

    rng = np.random.default_rng(5)
    n = 100
    args, start, stop, knots = _grid("regular", n, dtype, rng)
    x = rng.uniform(-2, 2, size=20_000).astype(dtype)
    k = 12_345
    x[k] = {"nan": np.nan, "inf": np.inf, "-inf": -np.inf, "huge": 1e20 if dtype == np.float64 else 1e20}[bad_value]
    x[k + 7] = np.nan  # a later failure changes nothing
    for method in R.METHODS:
        want, bad = R.eval(method, "regular", dtype, True, x, **args)
        assert bad == k
        it = _create(method, "regular", args, dtype, True)
        out = np.full(len(x), 42.0, dtype=dtype)
        with pytest.raises(AssertionError, match="^Unrepresentable number$"):
            it.eval_host([x], out)
        assert _bits_equal(out[:k], want[:k])
        assert np.all(out[k:] == dtype(42.0))
        with pytest.raises(AssertionError, match="^Unrepresentable number$") as ei:
            it.eval_tensors([torch.from_numpy(x).to("cuda:0")])
            it.finish()
        assert ei.value.first_bad_index == k
        it.close()


def test_python_surface_errors_and_eval():
    import torch

    from interpn_amd import one_dim

    vals = np.array([1.0, 2.0, 4.0])
    lin = one_dim.Linear1D(one_dim.RegularGrid1D(0.0, 1.0, vals), device=0)
    x = np.array([0.5, 1.5, 3.0, -1.0])
    assert np.array_equal(lin.eval(x), np.array([1.5, 3.0, 6.0, 0.0]))
    assert lin.eval_one(2.5) == 5.0
    t = lin.eval(torch.from_numpy(x).to("cuda:0"))
    assert np.array_equal(t.cpu().numpy(), np.array([1.5, 3.0, 6.0, 0.0]))
    with pytest.raises(AssertionError, match="^Length mismatch$"):
        lin.eval(x, np.zeros(3))
    with pytest.raises(AssertionError, match="^Unrepresentable number$") as ei:
        lin.eval(np.array([0.0, 1.0, np.nan, 2.0]))
    assert ei.value.first_bad_index == 2
    # rectilinear: NaN is no error (Left1D: vals[0], Right1D / Nearest1D: vals[1], the linear pair NaN)
    rg = one_dim.RectilinearGrid1D(np.array([0.0, 1.0, 3.0]), vals)
    nan = np.array([np.nan, np.inf])
    assert np.array_equal(one_dim.Left1D(rg, device=0).eval(nan), [1.0, 4.0])
    assert np.array_equal(one_dim.Right1D(rg, device=0).eval(nan), [2.0, 4.0])
    assert one_dim.Nearest1D(rg, device=0).eval(nan)[0] == 2.0
    assert np.isnan(one_dim.Linear1D(rg, device=0).eval(nan)[0])
    assert np.isnan(one_dim.LinearHoldLast1D(rg, device=0).eval(nan)[0])


@pytest.mark.parametrize("case", ["unsorted", "duplicates", "step0", "negstep", "nanstep", "stop_inf"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_degenerate_grids(case, dtype):
    rng = np.random.default_rng(11)
    n = 50
    vals = rng.normal(size=n).astype(dtype)
    if case in ("unsorted", "duplicates"):
        kind = "rectilinear"
        g = rng.normal(size=n).astype(dtype) if case == "unsorted" else np.sort(rng.integers(0, 10, size=n)).astype(dtype)
        args = dict(grid=g, vals=vals)
        x = np.concatenate([rng.normal(size=3000) * 3, g.astype(np.float64), [np.nan, np.inf, -np.inf]]).astype(dtype)
    else:
        kind = "regular"
        start, step = {"step0": (0.5, 0.0), "negstep": (2.0, -0.125), "nanstep": (0.0, np.nan),
                       "stop_inf": (dtype(np.finfo(dtype).max) / 2, dtype(np.finfo(dtype).max) / 8)}[case]
        args = dict(start=dtype(start), step=dtype(step), vals=vals)
        if case == "stop_inf":
            assert np.isinf(R.regular_stop(start, step, n, dtype))
            # finite points only (u < 2: below max), above and below start; nothing is OutsideHigh since stop = +inf
            x = (np.asarray([start], dtype=np.float64) * rng.uniform(0.5, 2.0, size=2000)).astype(dtype)
            assert np.all(np.isfinite(x))
        else:
            x = rng.normal(size=3000).astype(dtype) * 10
    for method in R.METHODS:
        for fma in (True, False):
            want, bad = R.eval(method, kind, dtype, fma, x, **args)
            it = _create(method, kind, args, dtype, fma)
            out = np.full(len(x), 42.0, dtype=dtype)
            if case == "stop_inf":
                assert bad is None  # both paths are compared over every point
            if bad is None:
                host, dev = _eval_both(it, x)
                assert _bits_equal(host, want), (case, method, fma)
                assert _bits_equal(dev, want), (case, method, fma)
            else:
                with pytest.raises(AssertionError, match="^Unrepresentable number$"):
                    it.eval_host([x], out)
                assert _bits_equal(out[:bad], want[:bad])
            it.close()


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_full_size_batch(kind):
    import torch

    dtype = np.float64
    rng = np.random.default_rng(99)
    args, start, stop, knots = _grid(kind, 1000, dtype, rng)
    npts = 100_000_000
    span = float(stop) - float(start)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    x = torch.rand(npts, dtype=torch.float64, device="cuda:0", generator=gen) * (1.2 * span) + (float(start) - 0.1 * span)
    idx = np.concatenate([rng.integers(0, npts, 100_000), np.arange(npts - 1000, npts)])
    xs = x[torch.from_numpy(idx).to("cuda:0")].cpu().numpy()
    out = torch.empty_like(x)
    for method in R.METHODS:
        want, bad = R.eval(method, kind, dtype, True, xs, **args)
        it = _create(method, kind, args, dtype, True)
        it.eval_tensors([x], out)
        it.finish()
        got = out[torch.from_numpy(idx).to("cuda:0")].cpu().numpy()
        assert _bits_equal(got, want), method
        it.close()


def test_kernel_family_and_multilinear_unchanged(oracle):
    from interpn_amd import Interpolator

    rng = np.random.default_rng(2024)
    n = 37
    start, step = -0.3, 0.0731
    vals = rng.normal(size=n)
    x = rng.uniform(-0.5, 3.0, size=20_000)
    lin = Interpolator.grid1d_regular("Linear1D", start, step, vals, device=0, fma=True)
    got1 = np.zeros_like(x)
    lin.eval_host([x], got1)
    assert lin.kernel_name().startswith("interpn::k_one_dim<double, 16, 0, ")
    want1, _ = R.eval("Linear1D", "regular", np.float64, True, x, start=start, step=step, vals=vals)
    assert _bits_equal(got1, want1)
    ml = Interpolator.regular("linear", [n], np.array([start]), np.array([step]), vals, device=0, fma=True)
    got2 = np.zeros_like(x)
    ml.eval_host([x], got2)
    assert "k_one_dim" not in ml.kernel_name()
    want2 = np.zeros_like(x)
    oracle.linear_regular([n], np.array([start]), np.array([step]), vals, [x], want2)
    assert np.array_equal(got2, want2)
    assert np.any(got1 != got2)  # not multilinear with N = 1


def test_replicate_and_sharded():
    from interpn_amd import Interpolator, eval_host_sharded

    rng = np.random.default_rng(8)
    n = 513
    vals = rng.normal(size=n)
    a = Interpolator.grid1d_regular("LinearHoldLast1D", -2.0, 0.01, vals, device=0)
    b = a.replicate(0)
    x = rng.normal(size=200_001) * 5
    one = np.zeros_like(x)
    a.eval_host([x], one)
    two = np.zeros_like(x)
    eval_host_sharded([a, b], [x], two)
    assert np.array_equal(one, two)
    cl = np.zeros_like(x)
    b.eval_host([x], cl)
    assert np.array_equal(one, cl)
    x[150_000] = np.nan  # in the second shard
    with pytest.raises(AssertionError, match="^Unrepresentable number$") as ei:
        eval_host_sharded([a, b], [x], np.zeros_like(x))
    assert ei.value.first_bad_index == 150_000
    # rectilinear handles replicate their axis
    g = np.sort(rng.uniform(-3, 3, size=n))
    r = Interpolator.grid1d_rectilinear("Nearest1D", g, vals, device=0)
    r2 = r.replicate(0)
    o1, o2 = np.zeros_like(x), np.zeros_like(x)
    r.eval_host([x], o1)
    r2.eval_host([x], o2)
    assert np.array_equal(o1, o2) and r2.kernel_name().startswith("interpn::k_one_dim<")


def test_options_and_entry_points():
    import torch

    from interpn_amd import Interpolator, _lib

    vals = np.arange(10.0)
    it = Interpolator.grid1d_regular("Linear1D", 0.0, 1.0, vals, device=0)
    assert it.get_option("fma") == 1
    it.set_option("fma", 0)
    assert it.get_option("fma") == 0
    nb = _lib.load().interpn_hip_table_bytes(it._h, None, None)
    assert nb == 9 * 32
    with pytest.raises(ValueError):
        it.check_bounds_tensors([torch.zeros(4, dtype=torch.float64, device="cuda:0")], 0.0)
    with pytest.raises(ValueError):  # nobs != 1
        it.eval_host([np.zeros(3), np.zeros(3)], np.zeros(3))
    with pytest.raises(AssertionError, match="^Length mismatch$"):
        it.eval_host([np.zeros(3)], np.zeros(4))


def test_f32_regular_grid_beyond_2_24_knots():
    """f32: T(i) and T(n - 1) round once they pass 2^24 (one_dim/mod.rs:88, :125).  The device-built x0 of cells past
    2^24 (and stop) against the restatement, on a sample of points around the end of a grid of 2^24 + 2^20 + 1 knots."""
    dtype = np.float32
    n = 2**24 + 2**20 + 1
    rng = np.random.default_rng(24)
    vals = rng.normal(size=n).astype(dtype)
    start, step = np.float32(-3.0), np.float32(0.3712e-6)
    stop = R.regular_stop(start, step, n, dtype)
    span = float(stop) - float(start)
    x = np.concatenate([rng.uniform(float(stop) - 0.05 * span, float(stop) + 0.01 * span, 6000),
                        rng.uniform(float(start), float(stop), 1000), [float(stop) * 2, -50.0]]).astype(dtype)
    args = dict(start=start, step=step, vals=vals)
    i, *_ = R.grid_at("regular", dtype, x, **args)
    assert ((i > 2**24) & (i % 2 == 1)).sum() > 100  # odd cells past 2^24: T(i) is not i there
    for method in R.METHODS:
        for fma in ((True, False) if method.startswith("Linear") else (True,)):
            want, bad = R.eval(method, "regular", dtype, fma, x, **args)
            assert bad is None
            it = _create(method, "regular", args, dtype, fma)
            host, dev = _eval_both(it, x)
            assert _bits_equal(host, want), (method, fma)
            assert _bits_equal(dev, want), (method, fma)
            it.close()
