"""interpn::one_dim on the MI355X (k_one_dim.hip): bit-for-bit parity with the CPU restatement
(tests/one_dim_restatement.py, pinned by tests/test_one_dim_cpu.py) on both evaluation paths, the error contract of
regular grids, degenerate grids, a full-size batch, and the multi-handle forms; then every LDS x PPL form asserted from
the kernel tag, batch tails with guards, the error contract per pair and across chunk seams, the cell index next to
knots and at the admission limits of the divide-free form, stressed bucket tables, the staged host pipeline, a bound
against exact rationals, a fuzz slice, graph capture and a side stream."""

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


# ---------------------------------------------------------------------------------------------------------------------
# Every kernel form, named; batch tails; the error contract per pair; cell search next to knots; stressed bucket tables;
# the staged host pipeline; a bound against exact rationals; a fuzz slice; graph capture and a side stream.
# ---------------------------------------------------------------------------------------------------------------------

METHOD_FLAVOURS = [(m, f) for m in R.METHODS for f in ((True, False) if m.startswith("Linear") else (False,))]
MF_IDS = [f"{m}-{'fma' if f else 'nofma'}" if m.startswith("Linear") else m for m, f in METHOD_FLAVOURS]
BATCHES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 100_003]
SENTINEL = -777.0


def _tt(dtype):
    import torch

    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _assert_bits(got, want, x, ctx, args=None, kind=None):
    """Bit equality; on a mismatch the first offenders as (index, x, cell, got, want)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    eq = ((got == want) & (np.signbit(got) == np.signbit(want))) | (np.isnan(got) & np.isnan(want))
    if eq.all():
        return
    bad = np.flatnonzero(~eq)
    cell = R.grid_at(kind, got.dtype, np.asarray(x)[bad[:5]], **args)[0] if args is not None else [None] * 5
    rows = [(int(i), float(np.asarray(x)[i]).hex(), None if c is None else int(c), float(got[i]).hex(), float(want[i]).hex())
            for i, c in zip(bad[:5], cell)]
    print("MISMATCH", ctx, f"{bad.size} of {got.size}:", rows, flush=True)
    raise AssertionError((ctx, int(bad.size), rows))


def _form(it):
    """(LDS, PPL) from the last two template arguments of the tag (k_one_dim.hip::od_go)."""
    name = it.kernel_name()
    assert name.startswith("interpn::k_one_dim<") and name.endswith(">"), name
    a = [s.strip() for s in name[name.index("<") + 1:-1].split(",")]
    assert a[-2] in ("true", "false") and a[-1] in ("1", "2"), name
    return a[-2] == "true", int(a[-1])


def _dev_eval(it, x, obs_off=0, out_off=2, stream=None):
    """Device path on views `obs_off` / `out_off` elements into their buffers; out sits in a sentinel-filled buffer with
    out_off (>= 2) guard elements before and at least 2 behind.  Returns (out, guards_untouched, error)."""
    import torch

    m = len(x)
    tt = _tt(x.dtype)
    ob = torch.zeros(m + obs_off + 2, dtype=tt, device="cuda:0")
    ob[obs_off:obs_off + m] = torch.from_numpy(x).to("cuda:0")
    full = torch.full((m + out_off + 3,), SENTINEL, dtype=tt, device="cuda:0")
    out = full[out_off:out_off + m]
    assert ob.data_ptr() % 16 == 0 and full.data_ptr() % 16 == 0
    err = None
    try:
        it.eval_tensors([ob[obs_off:obs_off + m]], out, stream=stream)
        it.finish()
    except AssertionError as e:
        err = e
    h = full.cpu().numpy()
    guards = bool(np.all(h[:out_off] == SENTINEL) and np.all(h[out_off + m:] == SENTINEL))
    return h[out_off:out_off + m].copy(), guards, err


_WANT = {}


def _form_case(method, fma, kind, dtype):
    key = (method, fma, kind, np.dtype(dtype).name)
    if key not in _WANT:
        rng = np.random.default_rng(4242 + (kind == "regular") + 2 * (np.dtype(dtype) == np.float32))
        args, start, stop, knots = _grid(kind, 300, dtype, rng)
        x = _points(kind, dtype, start, stop, knots, rng, m=55_000)[:BATCHES[-1]]
        assert len(x) == BATCHES[-1]
        want, bad = R.eval(method, kind, dtype, fma, x, **args)
        assert bad is None
        _WANT[key] = (args, x, want)
    return _WANT[key]


# how the form is reached -> (obs element offset, out element offset, option ppl, expected PPL)
HOW = {"aligned": (0, 2, 0, 2), "opt_ppl1": (0, 2, 1, 1), "obs_off": (1, 2, 0, 1), "out_off": (0, 3, 0, 1), "both_off": (1, 3, 0, 1)}


@pytest.mark.parametrize("how", list(HOW))
@pytest.mark.parametrize("lds", [True, False], ids=["lds", "nolds"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,fma", METHOD_FLAVOURS, ids=MF_IDS)
def test_every_instantiation(method, fma, kind, dtype, lds, how):
    """k_one_dim<T, OP, KIND, FMA, LDS, PPL>: every LDS x PPL form of every method / kind / dtype / flavour, asserted from
    the tag, at batch sizes around the wave, the workgroup and the pair (1 .. 513 and 100 003), with untouched guards."""
    args, x, want = _form_case(method, fma, kind, dtype)
    obs_off, out_off, opt, ppl = HOW[how]
    it = _create(method, kind, args, dtype, fma)
    if not lds:
        it.set_option("axis_lds_kb", 0)
    it.set_option("ppl", opt)
    for m in BATCHES:
        got, guards, err = _dev_eval(it, x[:m], obs_off, out_off)
        assert err is None, (m, err)
        assert _form(it) == (lds, ppl), (m, it.kernel_name())
        assert guards, ("guard elements written", m)
        _assert_bits(got, want[:m], x[:m], (method, fma, kind, how, m), args, kind)
        if how in ("aligned", "opt_ppl1") and m <= 513:  # the host entry stages into aligned buffers of its own
            buf = np.full(m + 4, SENTINEL, dtype=dtype)
            it.eval_host([x[:m]], buf[2:2 + m])
            assert _form(it) == (lds, ppl), (m, it.kernel_name())
            assert np.all(buf[:2] == SENTINEL) and np.all(buf[2 + m:] == SENTINEL)
            _assert_bits(buf[2:2 + m], want[:m], x[:m], (method, fma, kind, how, m, "host"), args, kind)
    it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("method", ["Left1D", "Linear1D"])
def test_lds_switch_at_the_table_size(method, dtype):
    """The automatic LDS switch (k_one_dim.hip::launch_t: the table rounded up to 16 bytes against min(thr_axis_lds_wide,
    dev_lds_per_wg)): the largest n still staged runs LDS = true, n + 1 runs LDS = false, both with the restatement's
    bits, the last cell (the last staged 16-byte line) included.  n comes from the handle's own queries."""
    from interpn_amd import _lib

    lib = _lib.load()
    tb = lambda it: int(lib.interpn_hip_table_bytes(it._h, None, None))
    r16 = lambda b: (b + 15) & ~15
    rng = np.random.default_rng(77)
    probe = _create(method, "regular", dict(start=dtype(0), step=dtype(1), vals=np.zeros(1025, dtype=dtype)), dtype, True)
    per_cell, rem = divmod(tb(probe), 1024)
    assert rem == 0 and per_cell == np.dtype(dtype).itemsize * (2 if method == "Left1D" else 4)
    budget = min(probe.get_option("thr_axis_lds_wide"), probe.get_option("dev_lds_per_wg"))
    assert probe.get_option("axis_lds_kb") < 0  # the default: the threshold decides
    probe.close()
    cells = budget // per_cell
    while r16((cells + 1) * per_cell) <= budget:
        cells += 1
    while r16(cells * per_cell) > budget:
        cells -= 1
    assert cells > 100
    for n, lds in ((cells + 1, True), (cells + 2, False)):
        vals = rng.normal(size=n).astype(dtype)
        start, step = dtype(-1.25), dtype(0.0731)
        args = dict(start=start, step=step, vals=vals)
        stop = R.regular_stop(start, step, n, dtype)
        last = np.linspace(float(stop) - 1.5 * float(step), float(stop) + 0.5 * float(step), 3001)
        x = np.concatenate([rng.uniform(float(start) - 1, float(stop) + 1, 20_001), last, [float(stop), float(start)]]).astype(dtype)
        i = R.grid_at("regular", dtype, x, **args)[0]
        assert (i == n - 2).sum() > 1000 and (i == n - 3).sum() > 100
        for fma in (True, False):
            it = _create(method, "regular", args, dtype, fma)
            assert (r16(tb(it)) <= budget) == lds, (n, tb(it), budget)
            want, bad = R.eval(method, "regular", dtype, fma, x, **args)
            assert bad is None
            host, dev = _eval_both(it, x)
            assert _form(it) == (lds, 2), (n, it.kernel_name())
            _assert_bits(dev, want, x, (method, n, fma, "device"), args, "regular")
            _assert_bits(host, want, x, (method, n, fma, "host"), args, "regular")
            it.close()


@pytest.mark.parametrize("ppl", [1, 2])
@pytest.mark.parametrize("bad_value", ["nan", "inf", "huge"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_error_contract_per_pair(dtype, bad_value, ppl):
    """Regular grids, the PPL = 2 pair (ok0 && !ok1, !ok0 && ok1, both, index 0, the last index of an even and an odd
    batch) and the scalar form: host out[:k] has the restatement's bits and out[k:] is untouched; device first_bad_index
    is k, out[:k] has the bits, the guards around out are untouched (out[k..] is unspecified); a later bad point does not
    win; the next clean evaluation on the handle is complete (status word reset)."""
    rng = np.random.default_rng(51)
    args, start, stop, knots = _grid("regular", 100, dtype, rng)
    bv = dtype({"nan": np.nan, "inf": np.inf, "huge": 1e20}[bad_value])
    for m in (1000, 1001):
        clean = rng.uniform(-2, 2, size=m).astype(dtype)
        for where in ([500], [501], [500, 501], [0], [m - 1], [m - 2, m - 1]):
            x = clean.copy()
            x[where] = bv
            k = where[0]
            if k + 7 < m:
                x[k + 7] = np.nan  # later: must not win
            for method in R.METHODS:
                want, bad = R.eval(method, "regular", dtype, True, x, **args)
                assert bad == k
                it = _create(method, "regular", args, dtype, True)
                it.set_option("ppl", 1 if ppl == 1 else 0)
                out = np.full(m, 42.0, dtype=dtype)
                with pytest.raises(AssertionError, match="^Unrepresentable number$"):
                    it.eval_host([x], out)
                assert _form(it)[1] == ppl
                _assert_bits(out[:k], want[:k], x[:k], (method, m, where, "host"), args, "regular")
                assert np.all(out[k:] == dtype(42.0)), (method, m, where)
                got, guards, err = _dev_eval(it, x)
                assert err is not None and str(err) == "Unrepresentable number" and err.first_bad_index == k, (method, m, where, err)
                assert _form(it)[1] == ppl
                assert guards
                _assert_bits(got[:k], want[:k], x[:k], (method, m, where, "device"), args, "regular")
                wantc, badc = R.eval(method, "regular", dtype, True, clean, **args)
                got, guards, err = _dev_eval(it, clean)
                assert err is None and badc is None and guards
                _assert_bits(got, wantc, clean, (method, m, where, "clean device"), args, "regular")
                out = np.full(m, 42.0, dtype=dtype)
                it.eval_host([clean], out)
                _assert_bits(out, wantc, clean, (method, m, where, "clean host"), args, "regular")
                it.close()


# -- regular grids: the cell index next to knots ------------------------------------------------------------------------

def _ulp_walk(v, j):
    """v moved by j ulps (j < 0: down), elementwise."""
    to = v.dtype.type(np.inf if j > 0 else -np.inf)
    for _ in range(abs(j)):
        v = np.nextafter(v, to)
    return v


def knot_points(dtype, start, step, n, rng, ncells=2000, extra_cells=()):
    """Points around knots of the regular grid (start, step, n): for a sample of knots k (always the first 3 and the
    last 3, f32: both sides of 2^24 where the grid reaches it) the knot as the reference forms it, T(start + step T(k)),
    the same knot formed in wider arithmetic and rounded once, each of them moved by 0 .. 4 ulps both ways, and points
    at quotient offsets of +-2^-22, 2^-21, 2^-20, 2^-19, 2^-10 cells (f32: also those offsets times |k| + 1, as its
    admission margin grows with the quotient), x_k + step delta formed wide and rounded once.
    Returns (x, k): the points and the knot each belongs to."""
    dtype = np.dtype(dtype)
    T = dtype.type
    wide = np.longdouble if dtype == np.float64 else np.float64
    fixed = [0, 1, 2, n - 3, n - 2, n - 1] + list(extra_cells)
    if dtype == np.float32 and n > 2**24 + 4:
        fixed += list(range(2**24 - 3, 2**24 + 4))
    k = np.unique(np.concatenate([np.array([c for c in fixed if 0 <= c < n], dtype=np.int64), rng.integers(0, n, ncells)]))
    with np.errstate(all="ignore"):
        x_ref = (T(start) + T(step) * k.astype(dtype)).astype(dtype)
        x_wide = wide(T(start)) + wide(T(step)) * k.astype(wide)
        xs, ks = [], []
        for base in (x_ref, x_wide.astype(dtype)):
            for j in range(-4, 5):
                xs.append(_ulp_walk(base, j))
                ks.append(k)
        scales = [np.ones(len(k), dtype=wide)] + ([(np.abs(k) + 1).astype(wide)] if dtype == np.float32 else [])
        for sc in scales:
            for e in (-22, -21, -20, -19, -10):
                for sgn in (1, -1):
                    xs.append((x_wide + wide(T(step)) * (sc * wide(sgn * 2.0**e))).astype(dtype))
                    ks.append(k)
    return np.concatenate(xs), np.concatenate(ks)


def step_limits(dtype):
    """StepCellRange<T> (interpn_device.h): the steps the host admits to the divide-free cell index."""
    return (2.0**-128, 2.0**128) if np.dtype(dtype) == np.float64 else (2.0**-16, 2.0**16)


def fast_path_model(dtype, a0, step):
    """numpy model of od_eval's choice (k_one_dim.hip, interpn_device.h::floor_quotient_fast) for a0 = x - start:
    (admitted, floor(a0 * RN(1 / step)), floor(a0 / step)), all in T."""
    dtype = np.dtype(dtype)
    T = dtype.type
    with np.errstate(all="ignore"):
        qt = (a0 * (T(1) / T(step))).astype(dtype)
        d = qt - np.floor(qt)
        if dtype == np.float64:
            ok = (np.abs(d - 0.5) < 0.5 - 2.0**-20) & (np.abs(qt) < 2.0**31)
        else:  # the margin is one fused operation in f32: exact in f64, rounded once
            margin = (np.abs(qt).astype(np.float64) * 2.0**-21 + 2.0**-21).astype(np.float32)
            ok = (np.abs(d - T(0.5)) + margin).astype(np.float32) < T(0.5)
        lo, hi = step_limits(dtype)
        ok &= bool(lo <= float(step) <= hi)
        return ok, np.floor(qt), np.floor((a0 / T(step)).astype(dtype))


def _limit_steps(dtype):
    T = np.dtype(dtype).type
    lo, hi = (T(v) for v in step_limits(dtype))
    up, down = T(np.inf), T(0)
    return {"lo": lo, "lo_in": np.nextafter(lo, up), "lo_out": np.nextafter(lo, down),
            "hi": hi, "hi_in": np.nextafter(hi, down), "hi_out": np.nextafter(hi, up)}


# The (dtype, step) families of the CPU self-check (tests/test_one_dim_cpu.py): non-dyadic steps inside the admitted range
TEETH_FAMILIES = [
    ("f64-0.0731", np.float64, -1.25, 0.0731, 1_000_003),
    ("f64-third", np.float64, -1.25, 1.0 / 3.0, 1_000_003),
    ("f64-2.5/(n-1)", np.float64, -1.25, 2.5 / (2**22 - 1), 2**22),
    ("f32-0.0731", np.float32, -1.25, 0.0731, 2**20 + 2**18),
    ("f32-third", np.float32, -1.25, 1.0 / 3.0, 2**20 + 2**18),
    ("f32-2.5/(n-1)", np.float32, -1.25, 2.5 / 65535, 65536),
]


def regular_families():
    """label -> (dtype, start, step, n) of test_regular_cell_index_next_to_knots."""
    fam = {lab: (dt, dt(st), dt(sp), n) for lab, dt, st, sp, n in TEETH_FAMILIES}
    for dt, tag in ((np.float64, "f64"), (np.float32, "f32")):
        for nm, s in _limit_steps(dt).items():
            fam[f"{tag}-step-{nm}"] = (dt, dt(0), s, 1000)
        fam[f"{tag}-pow2"] = (dt, dt(-1.25), dt(2.0**-3), 100_003)
        fam[f"{tag}-pow2-start0"] = (dt, dt(0), dt(2.0**5), 70_001)
        fam[f"{tag}-start0"] = (dt, dt(0), dt(0.0731), 50_001)
    fam["f64-start1e6"] = (np.float64, np.float64(1e6), np.float64(1e-6), 1_000_003)  # span ~ 1: x - start cancels
    fam["f32-start1e6"] = (np.float32, np.float32(1e6), np.float32(0.25), 4099)
    fam["f32-past-2^24"] = (np.float32, np.float32(-3.0), np.float32(2.0**-16 * 1.37), 2**24 + 2**12)
    return fam


def _far_points(dtype, start, step):
    """Valid points far outside: quotients around the fast path's limits (2^20 in f32, 2^31) and below the isize limit."""
    wide = np.float64
    q = np.array([s * (2.0**e + d) for e in (20, 24, 31, 40, 62) for d in (-3.5, -1.0, -0.5, 0.0, 0.5, 1.0, 3.5) for s in (1, -1)])
    with np.errstate(all="ignore"):
        x = (wide(start) + wide(step) * q).astype(dtype)
    return x[np.isfinite(x)]


def family_points(family, ncells=2000, bulk=20):
    """The point set of a regular family: knot_points, _far_points, and `bulk` points spread over the grid (two cells of
    margin) for every point next to a knot.  The bulk is where the divide-free form runs at every cell index (the ulp
    neighbours mostly hand over to the division); it is also what keeps the points whose rounded quotient and exact
    knot comparison disagree, which exist only next to knots, a small share of the family
    (tests/test_one_dim_cpu.py::test_exact_cell_share_left_out).  Finite points only."""
    dtype, start, step, n = regular_families()[family]
    rng = np.random.default_rng(sum(map(ord, family)))
    x, _ = knot_points(dtype, start, step, n, rng, ncells=ncells)
    with np.errstate(all="ignore"):
        u = (np.float64(start) + np.float64(step) * rng.uniform(-2.0, n + 1.0, bulk * len(x))).astype(dtype)
    x = np.concatenate([x, _far_points(dtype, start, step), u])
    return x[np.isfinite(x)], rng


@pytest.mark.parametrize("family", list(regular_families()))
def test_regular_cell_index_next_to_knots(family):
    """od_eval's cell index where a reciprocal-multiply floor and floor(RN(a0 / step)) part: knots, their ulp neighbours
    and the admission threshold of floor_quotient_fast, on non-dyadic and power-of-two steps, steps at / inside /
    outside the admitted range (outside: the division path, same bits), starts 0, -1.25 and one that cancels, f32 up to
    and beyond the cell (2^20) where its margin reaches 0.5.  tests/test_one_dim_cpu.py shows these inputs have teeth."""
    dtype, start, step, n = regular_families()[family]
    x, rng = family_points(family)
    vals = rng.normal(size=n).astype(dtype)
    args = dict(start=start, step=step, vals=vals)
    i, *_rest, bad = R.grid_at("regular", dtype, x, **args)
    x = x[~bad]
    rng.shuffle(x)
    for method, fma in METHOD_FLAVOURS:
        want, bad = R.eval(method, "regular", dtype, fma, x, **args)
        assert bad is None
        it = _create(method, "regular", args, dtype, fma)
        host, dev = _eval_both(it, x)
        _assert_bits(dev, want, x, (family, method, fma, "device"), args, "regular")
        _assert_bits(host[:8000], want[:8000], x[:8000], (family, method, fma, "host"), args, "regular")
        it.set_option("ppl", 1)
        got, guards, err = _dev_eval(it, x[:30_001])
        assert err is None and guards and _form(it)[1] == 1
        _assert_bits(got, want[:30_001], x[:30_001], (family, method, fma, "ppl1"), args, "regular")
        it.close()


def test_regular_cell_index_on_a_large_f64_grid():
    """f64 cells up to 2^26 for a hold, a linear and the nearest method (test_regular_cell_index_at_2_30_cells goes to
    2^30 with Left1D alone)."""
    dtype = np.float64
    n = 2**26 + 3
    rng = np.random.default_rng(26)
    vals = rng.standard_normal(n)
    start, step = np.float64(-1.25), np.float64(0.0731)
    args = dict(start=start, step=step, vals=vals)
    x, _ = knot_points(dtype, start, step, n, rng, ncells=3000, extra_cells=range(n - 40, n))
    x = np.concatenate([x, _far_points(dtype, start, step)])
    rng.shuffle(x)
    for method, fma in (("Left1D", False), ("Linear1D", True), ("Nearest1D", False)):
        want, bad = R.eval(method, "regular", dtype, fma, x, **args)
        assert bad is None
        it = _create(method, "regular", args, dtype, fma)
        host, dev = _eval_both(it, x)
        assert _form(it)[0] is False
        _assert_bits(dev, want, x, (method, "device"), args, "regular")
        it.close()


def test_regular_cell_index_at_2_30_cells():
    """f64, Left1D (16 bytes per cell: a 16 GiB table), 2^30 + 2 cells: inside the grid the fast path's quotient comes
    within a factor 2 of its 2^31 limit.  The values are made on the device and borrowed by the handle."""
    import torch

    dtype = np.float64
    n = 2**30 + 3
    rng = np.random.default_rng(30)
    gen = torch.Generator(device="cuda:0").manual_seed(30)
    dvals = torch.randn(n, dtype=torch.float64, device="cuda:0", generator=gen)
    vals = dvals.cpu().numpy()
    start, step = np.float64(-1.25), np.float64(0.0731)
    args = dict(start=start, step=step, vals=vals)
    x, _ = knot_points(dtype, start, step, n, rng, ncells=3000, extra_cells=range(n - 40, n))
    x = np.concatenate([x, _far_points(dtype, start, step)])
    rng.shuffle(x)
    i = R.grid_at("regular", dtype, x, **args)[0]
    assert (i > 2**29).sum() > 10_000
    want, bad = R.eval("Left1D", "regular", dtype, False, x, **args)
    assert bad is None
    from interpn_amd import Interpolator

    it = Interpolator.grid1d_regular("Left1D", start, step, dvals, device=0, dtype=dtype)
    host, dev = _eval_both(it, x)
    assert _form(it)[0] is False
    _assert_bits(dev, want, x, "device", args, "regular")
    _assert_bits(host, want, x, "host", args, "regular")
    it.close()


# -- rectilinear axes: the bucket table where it is stressed -----------------------------------------------------------

def stressed_axes(dtype):
    """name -> strictly increasing axis (some with infinite ends) for test_rectilinear_stressed_axes."""
    dtype = np.dtype(dtype)
    T = dtype.type
    fi = np.finfo(dtype)

    def ulps(v0, m):  # m consecutive floats from v0 upwards
        out = np.empty(m, dtype=dtype)
        v = T(v0)
        for j in range(m):
            out[j] = v
            v = np.nextafter(v, T(np.inf))
        return out

    big = T(0.9) * fi.max
    tiny = T(fi.smallest_subnormal)
    ax = {}
    # all interior knots inside one bucket's width (M = 2 n buckets over the span): the scan of axis_partition_point
    ax["clustered"] = np.concatenate([[T(0)], ulps(5e5, 4094), [T(4e6)]]).astype(dtype)
    ax["two_clusters"] = np.concatenate([ulps(1.0, 2048), ulps(1e6, 2048)]).astype(dtype)
    wide_axis = np.linspace(-100.0, 100.0, 201).astype(dtype)
    ax["ulp_run"] = np.unique(np.concatenate([wide_axis, ulps(3.14159, 64)])).astype(dtype)
    ax["n2"] = np.array([-1.5, 2.25], dtype=dtype)
    ax["n3_mid_low"] = np.array([1.0, np.nextafter(T(1), T(2)), 7.0], dtype=dtype)
    ax["n3_mid_high"] = np.array([1.0, np.nextafter(T(7), T(0)), 7.0], dtype=dtype)
    ax["span_overflow"] = np.array([-big, -1.0, 0.0, 1.0, big], dtype=dtype)
    ax["span_overflow_n2"] = np.array([-big, big], dtype=dtype)  # f32: M / span is a subnormal
    ax["span_huge"] = np.array([0.0, 1.0, big], dtype=dtype)
    ax["span_tiny_scale_inf"] = (np.arange(10) * float(tiny)).astype(dtype)  # entirely subnormal; M / span = inf
    ax["span_tiny"] = ulps(1.0, 3)
    ax["subnormal"] = (np.arange(-20, 21) * 3 * float(tiny)).astype(dtype)
    ax["neg_inf_first"] = np.array([-np.inf, -1.0, 0.5, 2.0], dtype=dtype)
    ax["pos_inf_last"] = np.array([-1.0, 0.5, 2.0, np.inf], dtype=dtype)
    ax["both_inf"] = np.array([-np.inf, -1.0, 0.5, 2.0, np.inf], dtype=dtype)
    ax["neg_zero_knot"] = np.array([-1.0, -float(tiny), -0.0, float(tiny), 1.0], dtype=dtype)
    ax["pos_zero_knot"] = np.array([-float(fi.tiny), 0.0, float(fi.tiny), 3.0], dtype=dtype)
    ax["negative"] = (-np.cumsum(np.linspace(0.1, 1.0, 500))[::-1]).astype(dtype)
    for name, g in ax.items():
        assert np.all(g[1:] > g[:-1]), name
    return ax


AXIS_NAMES = list(stressed_axes(np.float64))


def axis_points(g):
    dtype = g.dtype
    fi = np.finfo(dtype)
    with np.errstate(all="ignore"):
        mids = (g[:-1].astype(np.float64) / 2 + g[1:].astype(np.float64) / 2).astype(dtype)
        pts = [_ulp_walk(g, j) for j in (-2, -1, 0, 1, 2)] + [mids]
        pts.append(np.array([0.0, -0.0, np.nan, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny,
                             fi.smallest_subnormal, -fi.smallest_subnormal, 1.0, -1.0], dtype=dtype))
    return np.concatenate(pts)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("axis", AXIS_NAMES)
def test_rectilinear_stressed_axes(axis, dtype):
    """create_one_dim's bucket table (M = 2 n buckets, scale = T(M / span)) and its fall-backs: many knots in one bucket,
    knots 1 ulp apart, n = 2 and 3, a span that overflows, M / span subnormal or infinite, infinite end knots, -0.0 and
    subnormal knots; points on every knot, +-1 and +-2 ulp, mid-points, +-0, NaN, +-inf, +-max.  Whether a table exists is
    not observable: only the bits are asserted, for the staged and the cached form and both PPL."""
    g = stressed_axes(dtype)[axis]
    rng = np.random.default_rng(len(g) + sum(map(ord, axis)))
    vals = rng.normal(size=len(g)).astype(dtype)
    args = dict(grid=g, vals=vals)
    x = axis_points(g)
    rng.shuffle(x)
    for method, fma in METHOD_FLAVOURS:
        want, bad = R.eval(method, "rectilinear", dtype, fma, x, **args)
        assert bad is None
        it = _create(method, "rectilinear", args, dtype, fma)
        host, dev = _eval_both(it, x)
        _assert_bits(dev, want, x, (axis, method, fma, "device"), args, "rectilinear")
        _assert_bits(host, want, x, (axis, method, fma, "host"), args, "rectilinear")
        it.set_option("axis_lds_kb", 0)
        it.set_option("ppl", 1)
        got, guards, err = _dev_eval(it, x)
        assert err is None and guards and _form(it) == (False, 1)
        _assert_bits(got, want, x, (axis, method, fma, "nolds ppl1"), args, "rectilinear")
        it.close()


# -- the staged host pipeline and its chunk seams ----------------------------------------------------------------------

@pytest.mark.parametrize("npts,chunk", [(8192, 0), (8193, 0), (50_001, 0), (50, 1), (50_001, 333), (50_001, 4096)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,fma", [("Linear1D", True), ("Left1D", False)], ids=["Linear1D-fma", "Left1D"])
def test_host_pipeline_against_restatement(monkeypatch, method, fma, kind, dtype, npts, chunk):
    """Host batches at and past the zero-copy limit (abi_host.hip: 8192 points) and forced chunk seams, against the
    restatement over ALL points (its fused step is vectorised: one_dim_restatement.fma_vec)."""
    if chunk:
        monkeypatch.setenv("INTERPN_HIP_HOST_CHUNK", str(chunk))  # latched per handle at creation
    rng = np.random.default_rng(npts + chunk)
    args, start, stop, knots = _grid(kind, 1000, dtype, rng)
    x = _points(kind, dtype, start, stop, knots, rng, m=npts)[:npts]
    assert len(x) == npts
    want, bad = R.eval(method, kind, dtype, fma, x, **args)
    assert bad is None
    it = _create(method, kind, args, dtype, fma)
    buf = np.full(npts + 4, SENTINEL, dtype=dtype)
    it.eval_host([x], buf[2:2 + npts])
    assert np.all(buf[:2] == SENTINEL) and np.all(buf[-2:] == SENTINEL)
    _assert_bits(buf[2:2 + npts], want, x, (method, kind, npts, chunk), args, kind)
    it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("chunk,npts", [(333, 5000), (0, 20_000)])
def test_host_abort_across_chunk_seams(monkeypatch, dtype, chunk, npts):
    """The abort contract of the host path with the bad point at chunk - 1, chunk, chunk + 1 and later chunks failing
    too: out[:k] has the restatement's bits, out[k:] is untouched, the index is k."""
    from interpn_amd import eval_host_sharded

    if chunk:
        monkeypatch.setenv("INTERPN_HIP_HOST_CHUNK", str(chunk))
    seam = chunk or 8192
    rng = np.random.default_rng(9)
    args, start, stop, knots = _grid("regular", 100, dtype, rng)
    clean = rng.uniform(-2, 2, size=npts).astype(dtype)
    for k in (seam - 1, seam, seam + 1, 2 * seam, 0):
        x = clean.copy()
        x[k] = np.nan
        x[k + 2 * seam + 3::seam] = np.inf  # later chunks fail too
        for method, fma in (("Linear1D", True), ("Right1D", False)):
            want, bad = R.eval(method, "regular", dtype, fma, x, **args)
            assert bad == k
            it = _create(method, "regular", args, dtype, fma)
            out = np.full(npts, 42.0, dtype=dtype)
            with pytest.raises(AssertionError, match="^Unrepresentable number$") as ei:
                eval_host_sharded([it], [x], out)
            assert ei.value.first_bad_index == k
            _assert_bits(out[:k], want[:k], x[:k], (method, chunk, k), args, "regular")
            assert np.all(out[k:] == dtype(42.0)), (method, chunk, k)
            out = np.full(npts, 42.0, dtype=dtype)
            with pytest.raises(AssertionError, match="^Unrepresentable number$"):
                it.eval_host([x], out)
            _assert_bits(out[:k], want[:k], x[:k], (method, chunk, k, "eval_host"), args, "regular")
            assert np.all(out[k:] == dtype(42.0)), (method, chunk, k)
            wantc, _ = R.eval(method, "regular", dtype, fma, clean, **args)
            it.eval_host([clean], out)
            _assert_bits(out, wantc, clean, (method, chunk, k, "clean"), args, "regular")
            it.close()


# -- something that is not the restatement -----------------------------------------------------------------------------

def test_kernels_within_exact_bound():
    """The kernels against one_dim_restatement.exact (rational arithmetic, cells by exact comparison with the knots):
    the linear pair within K u scale (K derived in tests/test_one_dim_cpu.py::EXACT_K), the selecting methods bit for
    bit, on samples of the regular families and the stressed axes, device entry."""
    import torch

    from tests.test_one_dim_cpu import EXACT_K, check_against_exact

    def on_device(kind, dtype, args):
        def ev(method, fma, xs):
            it = _create(method, kind, args, dtype, fma)
            out = it.eval_tensors([torch.from_numpy(np.ascontiguousarray(xs)).to("cuda:0")])
            it.finish()
            it.close()
            return out.cpu().numpy()
        return ev

    worst = {}
    for label, (dtype, start, step, n) in regular_families().items():
        if n > 2**23:
            continue  # exact() lists every knot; f32 past 2^24 cells the knots coincide
        rng = np.random.default_rng(sum(map(ord, label)))
        args = dict(start=start, step=step, vals=rng.normal(size=n).astype(dtype))
        x, _ = knot_points(dtype, start, step, n, rng, ncells=40)
        x = np.concatenate([x, rng.uniform(float(start) - 3 * float(step), float(start) + float(step) * (n + 2), 300).astype(dtype)])
        for f, w in check_against_exact("regular", dtype, x, args, on_device("regular", dtype, args)).items():
            worst[(np.dtype(dtype).name, f)] = max(worst.get((np.dtype(dtype).name, f), 0.0), w)
    for dtype in (np.float64, np.float32):
        for name, g in stressed_axes(dtype).items():
            rng = np.random.default_rng(len(g))
            args = dict(grid=g, vals=rng.normal(size=len(g)).astype(dtype))
            x = axis_points(g)
            x = x[rng.permutation(len(x))[:1500]]
            for f, w in check_against_exact("rectilinear", dtype, x, args, on_device("rectilinear", dtype, args)).items():
                worst[(np.dtype(dtype).name, f)] = max(worst.get((np.dtype(dtype).name, f), 0.0), w)
    print("worst |kernel - exact| / (u scale):", worst)
    for (name, f), w in worst.items():
        assert 0 < w <= EXACT_K[f]


# -- the remaining paths ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["f32", "ppl1", "big_table"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_full_size_batch_other_forms(kind, form):
    """test_full_size_batch (1e8 points, sampled) in f32, with ppl = 1, and with a table too large for LDS (n = 1 000 003)."""
    import torch

    dtype = np.float32 if form == "f32" else np.float64
    n = 1_000_003 if form == "big_table" else 1000
    rng = np.random.default_rng(98)
    args, start, stop, knots = _grid(kind, n, dtype, rng)
    npts = 100_000_001
    span = float(stop) - float(start)
    gen = torch.Generator(device="cuda:0").manual_seed(4)
    x = torch.rand(npts, dtype=torch.float64, device="cuda:0", generator=gen) * (1.2 * span) + (float(start) - 0.1 * span)
    x = x.to(_tt(dtype))
    idx = np.concatenate([rng.integers(0, npts, 100_000), np.arange(npts - 1000, npts), np.arange(0, 1000)])
    tidx = torch.from_numpy(idx).to("cuda:0")
    xs = x[tidx].cpu().numpy()
    out = torch.empty_like(x)
    for method, fma in METHOD_FLAVOURS:
        want, bad = R.eval(method, kind, dtype, fma, xs, **args)
        assert bad is None
        it = _create(method, kind, args, dtype, fma)
        if form == "ppl1":
            it.set_option("ppl", 1)
        it.eval_tensors([x], out)
        it.finish()
        assert _form(it) == (form != "big_table", 1 if form == "ppl1" else 2), it.kernel_name()
        _assert_bits(out[tidx].cpu().numpy(), want, xs, (kind, form, method, fma), args, kind)
        it.close()


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_graph_capture_and_side_stream(kind):
    """One eval_tensors of a one_dim handle is one kernel: captured into a hipGraph (no parallel branches) and replayed
    three times on new data, and evaluated on a non-default stream, against the restatement."""
    import torch

    dtype = np.float64
    rng = np.random.default_rng(61)
    args, start, stop, knots = _grid(kind, 500, dtype, rng)
    P = 200_001
    span = float(stop) - float(start)
    new = lambda: rng.uniform(float(start) - 0.2 * span, float(stop) + 0.2 * span, P)
    for method, fma in (("Linear1D", True), ("Nearest1D", False)):
        it = _create(method, kind, args, dtype, fma)
        obs = torch.zeros(P, dtype=torch.float64, device="cuda:0")
        out = torch.zeros(P, dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        h = new()
        obs.copy_(torch.from_numpy(h))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            it.eval_tensors([obs], out)  # on the side stream (torch's current one); also the warm-up outside capture
        it.finish()
        _assert_bits(out.cpu().numpy(), R.eval(method, kind, dtype, fma, h, **args)[0], h, (method, "side stream"), args, kind)
        out.zero_()
        it.eval_tensors([obs], out, stream=side)  # the stream given explicitly
        it.finish(side)
        _assert_bits(out.cpu().numpy(), R.eval(method, kind, dtype, fma, h, **args)[0], h, (method, "stream="), args, kind)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            it.eval_tensors([obs], out)
        for rep in range(3):
            h = new()
            obs.copy_(torch.from_numpy(h))
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits(out.cpu().numpy(), R.eval(method, kind, dtype, fma, h, **args)[0], h, (method, "replay", rep), args, kind)
        it.finish()
        it.close()


def test_one_dim_fuzz_short():
    """A fixed-seed slice of tools/fuzz_parity.py::run_one_dim (random method / kind / dtype / flavour / n / step and axis
    families / ppl / axis_lds_kb / entry point / offset views / injected NaN and inf), every case bit-identical to the
    restatement; the same 12 s budget as tests/test_gpu_parity.py::test_differential_fuzz_short."""
    from tools.fuzz_parity import run_one_dim

    cases, failures = run_one_dim(budget=12.0, seed=20261016, max_cases=12_000)
    print("one_dim fuzz cases:", cases)
    assert cases > 100
    assert failures == 0
