"""Lattice evaluation on the GPU (interpn_hip_eval_lattice_*): every result is compared BIT FOR BIT, at the same fma flavour,
with (a) the oracle run on the `np.meshgrid(..., indexing="ij")`-expanded, ravelled points and (b) the same handle's
`eval` on those points — on the fused path (interpn::k_lattice_axes + interpn::k_lattice_rows) and on the expanded one.

Wall time of the whole file on one MI355X: see DESIGN.md, "Lattice evaluation".
"""

import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import run_oracle, synthetic_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS_KERNEL = "interpn::k_lattice_rows<"
SHAPES = {2: [37, 53], 3: [17, 12, 23]}
LATTICE = {2: [41, 67], 3: [11, 13, 71]}
CLASSES = ("outside_low", "inside_low", "none", "inside_high", "outside_high")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_bits(got, want, ctx):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (ctx, len(bad), bad[:5].tolist(), [(got[b], want[b]) for b in bad[:5]])


def _grid_case(method, kind, shape, dtype, seed, linearize=False):
    return synthetic_case(method, kind, len(shape), shape, 1, seed, dtype=dtype, linearize=linearize, specials=False)


def _axis(g, m, rng, dtype):
    """`m` coordinates for the grid axis `g`: beyond both ends, in the first, the last and a middle interval (with the two
    ends: all five cubic saturation classes), exact knots, a repeated value, the rest random; shuffled."""
    n = g.size
    g = g.astype(np.float64)
    span = g[-1] - g[0]
    base = [g[0] - 0.11 * span, g[-1] + 0.09 * span, 0.5 * (g[0] + g[1]), 0.5 * (g[-2] + g[-1]),
            0.5 * (g[n // 2 - 1] + g[n // 2]), g[0], g[-1], g[1], g[-2], g[n // 2]]
    x = rng.uniform(g[0] - 0.05 * span, g[-1] + 0.05 * span, m)
    k = min(m, len(base))
    x[:k] = base[:k]
    if m >= len(base) + 2:
        x[len(base)] = x[len(base) + 1] = x[4]
    x = x.astype(dtype)
    rng.shuffle(x)
    return x


def _axes(case, lens, seed):
    rng = np.random.default_rng(seed)
    return [_axis(case.grids[d], lens[d], rng, case.vals.dtype) for d in range(len(lens))]


def _expand(axes):
    return [np.ascontiguousarray(m.ravel()) for m in np.meshgrid(*axes, indexing="ij")]


def _classes(case, d, x):
    """Saturation class of every coordinate of axis d, from the oracle side's cell computation: the regular grid's
    floor((x - start) / step) in the element type, the rectilinear grid's partition point."""
    g = case.grids[d]
    n = g.size
    dtype = case.vals.dtype.type
    if case.kind == "regular":
        floc = np.floor((x.astype(dtype) - dtype(case.starts[d])) / dtype(case.steps[d]))
        sel = [floc < 0, floc == 0, (floc > 0) & (floc < n - 2), floc == n - 2, floc > n - 2]
    else:
        iloc = np.searchsorted(g, x, side="left") - 2  # partition_point(|v| v < x) - 2
        sel = [iloc == -2, iloc == -1, (iloc > -1) & (iloc < n - 3), iloc == n - 3, iloc == n - 2]
    return {name for name, s in zip(CLASSES, sel) if s.any()}


def _make(case, fma=None):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, case.vals,
                                                linearize_extrapolation=case.linearize, dtype=case.vals.dtype, fma=fma)
    return interpn_amd.Interpolator.rectilinear(case.method, case.grids, case.vals, linearize_extrapolation=case.linearize,
                                                dtype=case.vals.dtype, fma=fma)


def _tensors(arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def _want(oracle, case, points, fma=True):
    c = dataclasses.replace(case, obs=points)
    return run_oracle(oracle, c, fma=fma, out=np.zeros(points[0].size, dtype=case.vals.dtype))


def _eval_points(it, points):
    res = it.eval_tensors(_tensors(points))
    it.finish()
    return res.cpu().numpy()


def _eval_lattice(it, axes, **kw):
    res = it.eval_lattice_tensors(_tensors(axes), **kw)
    it.finish()
    return res.cpu().numpy()


def _kernel(dtype, method, n, kind, fma):
    return (f"{ROWS_KERNEL}{'double' if dtype == np.float64 else 'float'}, {0 if method == 'linear' else 1}, {n}, "
            f"{'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>")


FUSED = [("linear", False), ("cubic", False), ("cubic", True)]


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("method,linearize", FUSED, ids=["linear", "cubic-nolin", "cubic-lin"])
def test_fused_instantiations(oracle, method, linearize, n, kind, dtype, fma):
    case = _grid_case(method, kind, SHAPES[n], dtype, seed=3 * n + len(method), linearize=linearize)
    axes = _axes(case, LATTICE[n], seed=100 + n)
    if method == "cubic":
        for d in range(n):
            assert _classes(case, d, axes[d]) == set(CLASSES), (d, _classes(case, d, axes[d]))
    points = _expand(axes)
    want = _want(oracle, case, points, fma)
    it = _make(case, fma)
    try:
        it.set_option("lattice", 1)
        dev = _eval_lattice(it, axes)
        assert dev.shape == tuple(LATTICE[n])
        assert it.last_lattice_path == "fused"
        assert it.kernel_name() == _kernel(dtype, method, n, kind, fma), it.kernel_name()
        host = it.eval_lattice_host(axes)
        assert host.shape == tuple(LATTICE[n]) and it.last_lattice_path == "fused"
        _assert_bits(dev, want, ("fused device vs oracle", method, n, kind))
        _assert_bits(host, want, ("fused host vs oracle", method, n, kind))
        _assert_bits(dev, _eval_points(it, points), ("fused vs eval", method, n, kind))
    finally:
        it.close()


LENGTH_CASES = [("linear", "regular", 3, np.float64), ("cubic", "rectilinear", 2, np.float32)]


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "expanded"])
@pytest.mark.parametrize("other", [1, 2, 7])
@pytest.mark.parametrize("last", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("method,kind,n,dtype", LENGTH_CASES, ids=["linear3-regular-f64", "cubic2-rectilinear-f32"])
def test_axis_lengths_and_guards(oracle, method, kind, n, dtype, last, other, mode):
    import torch

    case = _grid_case(method, kind, SHAPES[n], dtype, seed=11, linearize=True)
    lens = [other] * (n - 1) + [last]
    axes = _axes(case, lens, seed=last + other)
    points = _expand(axes)
    want = _want(oracle, case, points)
    count, guard, sentinel = want.size, 3, -12345.5
    it = _make(case)
    try:
        it.set_option("lattice", mode)
        big = torch.full((count + 2 * guard,), sentinel, dtype=torch.float64 if dtype == np.float64 else torch.float32,
                         device="cuda:0")
        it.eval_lattice_tensors(_tensors(axes), out=big[guard:guard + count])
        it.finish()
        assert it.last_lattice_path == ("fused" if mode else "expanded")
        got = big.cpu().numpy()
        assert (got[:guard] == sentinel).all() and (got[guard + count:] == sentinel).all()
        _assert_bits(got[guard:guard + count], want, ("lengths", lens, mode))
    finally:
        it.close()


@pytest.mark.parametrize("method,kind,n,dtype", LENGTH_CASES + [("cubic", "regular", 3, np.float64), ("linear", "rectilinear", 2, np.float32)],
                         ids=["linear3-regular-f64", "cubic2-rectilinear-f32", "cubic3-regular-f64", "linear2-rectilinear-f32"])
def test_three_lattice_settings(oracle, method, kind, n, dtype):
    import interpn_amd

    case = _grid_case(method, kind, SHAPES[n], dtype, seed=5)
    it = _make(case)
    try:
        # a lattice with a row for every wave of the device, and one without: the automatic rule tells them apart
        for lens in ([40, 30, 50] if n == 3 else [1100, 50], [3, 3, 50][3 - n:]):
            axes = _axes(case, lens, seed=sum(lens))
            points = _expand(axes)
            want = _want(oracle, case, points)
            results = {}
            for mode in (0, 1, -1):
                it.set_option("lattice", mode)
                results[mode] = _eval_lattice(it, axes)
                rows = it.kernel_name().startswith(ROWS_KERNEL)
                planned = interpn_amd.lattice_plan(dtype, method, SHAPES[n], lens)[0]
                expect = {0: "expanded", 1: "fused", -1: planned}[mode]
                assert it.last_lattice_path == expect and rows == (expect == "fused"), (mode, lens, it.last_lattice_path, it.kernel_name())
                _assert_bits(results[mode], want, ("setting", mode, lens))
            nrows = int(np.prod(lens[:-1]))
            assert interpn_amd.lattice_plan(dtype, method, SHAPES[n], lens)[0] == ("fused" if nrows >= 4 * it.get_option("dev_num_cus") else "expanded")
            assert results[0].tobytes() == results[1].tobytes() == results[-1].tobytes()
    finally:
        it.close()


EXPANDED = [("nearest", [301], [777]), ("nearest", [9, 11], [13, 17]), ("nearest", [9, 7, 11], [6, 5, 9]),
            ("linear", [301], [1500]), ("linear", [5, 4, 6, 7], [4, 3, 5, 6]), ("linear", [3, 2, 4, 3, 2], [3, 2, 3, 4, 5]),
            ("linear", [3, 2, 4, 3, 2, 3, 4], [2, 3, 2, 2, 3, 2, 3]),
            ("cubic", [301], [1500]), ("cubic", [5, 4, 6, 7], [4, 3, 5, 6]), ("cubic", [4, 5, 4, 4, 5], [3, 2, 3, 2, 5])]


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,shape,lens", EXPANDED, ids=[f"{m}-N{len(s)}" for m, s, _ in EXPANDED])
def test_expanded_path(oracle, method, shape, lens, kind):
    case = _grid_case(method, kind, shape, np.float64, seed=17 + len(shape), linearize=method == "cubic")
    axes = _axes(case, lens, seed=len(shape))
    points = _expand(axes)
    it = _make(case)
    try:
        it.set_option("lattice", 1)  # "wherever covered": none of these is
        dev = _eval_lattice(it, axes)
        assert dev.shape == tuple(lens) and it.last_lattice_path == "expanded"
        assert not it.kernel_name().startswith(ROWS_KERNEL)
        host = it.eval_lattice_host(axes)
        _assert_bits(dev, _eval_points(it, points), ("expanded vs eval", method, shape))
        _assert_bits(dev, _want(oracle, case, points), ("expanded vs oracle", method, shape))
        _assert_bits(host, dev, ("expanded host", method, shape))
    finally:
        it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_last_axis_at_the_lds_budget(oracle, dtype):
    """Four lines of n_{N-1} elements must fit the budget (option axis_lds_kb): the boundary, computed from the option."""
    kb = 1
    inside = kb * 1024 // (4 * np.dtype(dtype).itemsize)
    for n_last, path in ((inside, "fused"), (inside + 1, "expanded")):
        shape = [5, 6, n_last]
        case = _grid_case("linear", "regular", shape, dtype, seed=n_last)
        axes = _axes(case, [4, 5, 90], seed=n_last)
        points = _expand(axes)
        it = _make(case)
        try:
            it.set_option("axis_lds_kb", kb)
            it.set_option("lattice", 1)
            got = _eval_lattice(it, axes)
            assert it.last_lattice_path == path, (n_last, it.last_lattice_path)
            _assert_bits(got, _want(oracle, case, points), ("lds boundary", n_last))
            _assert_bits(got, _eval_points(it, points), ("lds boundary vs eval", n_last))
        finally:
            it.close()


def _formula(lens, bad):
    """min over bad (d, j) of j * prod(lens[e], e > d)."""
    return min(j * int(np.prod(lens[d + 1:], dtype=object)) for d, j in bad)


BAD_SETS = [[(0, 5)], [(1, 3)], [(2, 7)], [(0, 6), (2, 2)], [(1, 0), (2, 40)], [(2, 0)]]
FAILING = [("linear", [17, 12, 23], 1), ("cubic", [17, 12, 23], 1), ("nearest", [9, 7, 11], 1), ("linear", [17, 12, 23], 0)]


@pytest.mark.parametrize("value", [np.nan, np.inf, 1e300], ids=["nan", "inf", "1e300"])
@pytest.mark.parametrize("bad", BAD_SETS, ids=["axis0", "middle", "last", "two", "two-b", "first-point"])
@pytest.mark.parametrize("method,shape,mode", FAILING, ids=["linear-fused", "cubic-fused", "nearest-expanded", "linear-expanded"])
def test_failing_points_on_regular_grids(oracle, method, shape, mode, bad, value):
    lens = [9, 8, 45]
    case = _grid_case(method, "regular", shape, np.float64, seed=23)
    clean = _axes(case, lens, seed=9)
    axes = [a.copy() for a in clean]
    for d, j in bad:
        axes[d][j] = value
    first = _formula(lens, bad)
    want = _want(oracle, case, _expand(clean))
    # the oracle's own loop agrees on the index
    with pytest.raises(AssertionError) as oe:
        _want(oracle, case, _expand(axes))
    assert oe.value.first_bad == first
    it = _make(case)
    try:
        it.set_option("lattice", mode)
        it.eval_lattice_tensors(_tensors(axes))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
            it.finish()
        assert e.value.first_bad_index == first, (e.value.first_bad_index, first)
        assert it.last_lattice_path == ("fused" if mode and method != "nearest" else "expanded")
        # host form: exactly the prefix, the rest of `out` as it was
        sentinel = -777.25
        out = np.full(lens, sentinel)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
            it.eval_lattice_host(axes, out)
        assert e.value.first_bad_index == first
        flat = out.ravel()
        _assert_bits(flat[:first], want.ravel()[:first], ("prefix", bad))
        assert (flat[first:] == sentinel).all()
        # the status word is cleared: a clean lattice afterwards is clean
        _assert_bits(_eval_lattice(it, clean), want, ("clean after failure", bad))
    finally:
        it.close()


def test_first_failure_behind_the_first_expanded_slice(oracle):
    """Two slices of the expanded path (64 MiB of coordinates each): the reported index is the lattice's, not the slice's."""
    lens = [180, 180, 180]
    case = _grid_case("nearest", "regular", [9, 7, 11], np.float32, seed=2)
    axes = _axes(case, lens, seed=3)
    axes[0][179] = np.nan
    it = _make(case)
    try:
        it.eval_lattice_tensors(_tensors(axes))
        with pytest.raises(AssertionError) as e:
            it.finish()
        assert it.last_lattice_path == "expanded"
        assert e.value.first_bad_index == 179 * 180 * 180 > 64 * 2**20 // (3 * 4)
        axes[0][179] = 0.25
        points = _expand(axes)
        _assert_bits(_eval_lattice(it, axes), _eval_points(it, points), "two slices")
    finally:
        it.close()


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "expanded"])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_rectilinear_grids_propagate_nan(oracle, method, mode):
    lens = [9, 8, 45]
    case = _grid_case(method, "rectilinear", [17, 12, 23], np.float64, seed=29)
    axes = _axes(case, lens, seed=4)
    axes[0][2] = np.nan
    axes[2][31] = np.nan
    points = _expand(axes)
    it = _make(case)
    try:
        it.set_option("lattice", mode)
        got = _eval_lattice(it, axes)  # finish() inside: no failure reported
        host = it.eval_lattice_host(axes)
        expect_nan = np.zeros(lens, dtype=bool)
        expect_nan[2, :, :] = True
        expect_nan[:, :, 31] = True
        assert np.array_equal(np.isnan(got), expect_nan)
        ref = _eval_points(it, points).reshape(lens)
        assert np.array_equal(np.isnan(ref), expect_nan)
        _assert_bits(got[~expect_nan], ref[~expect_nan], "beside the NaN planes")
        _assert_bits(got[~expect_nan], _want(oracle, case, points).reshape(lens)[~expect_nan], "beside the NaN planes, oracle")
        assert np.array_equal(np.isnan(host), expect_nan)
        _assert_bits(host[~expect_nan], got[~expect_nan], "host")
    finally:
        it.close()


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "expanded"])
def test_streams_reserve_and_capture(oracle, mode):
    import torch

    import interpn_amd

    lens = [12, 9, 130]
    case = _grid_case("linear", "rectilinear", SHAPES[3], np.float64, seed=31)
    axes = _axes(case, lens, seed=6)
    want = _want(oracle, case, _expand(axes))
    # no_alloc without a reserved block: an error, not a silent allocation
    it = _make(case)
    try:
        it.set_option("lattice", mode)
        with pytest.raises(interpn_amd._lib.InterpnHipError):
            it.eval_lattice_tensors(_tensors(axes), no_alloc=True)
        it.reserve_lattice(lens, 1)
        allocs = it.get_option("scratch_allocs")
        assert allocs >= 1
        got = _eval_lattice(it, axes, no_alloc=True)
        assert it.get_option("scratch_allocs") == allocs
        _assert_bits(got, want, "no_alloc after reserve")
        _assert_bits(it.eval_lattice_host(axes), want, "host form")
        # a side stream, as torch's current one and given explicitly
        ax_t = _tensors(axes)
        out = torch.zeros(lens, dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            it.eval_lattice_tensors(ax_t, out)
        it.finish()
        _assert_bits(out.cpu().numpy(), want, "side stream")
        out.zero_()
        torch.cuda.synchronize()
        it.eval_lattice_tensors(ax_t, out, stream=side)
        it.finish(side)
        _assert_bits(out.cpu().numpy(), want, "stream=")
        # capture on a single stream, replay on new coordinates
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            it.eval_lattice_tensors(ax_t, out)
        assert it.last_lattice_path == ("fused" if mode else "expanded")
        for rep in range(2):
            fresh = _axes(case, lens, seed=50 + rep)
            for d in range(3):
                ax_t[d].copy_(torch.from_numpy(fresh[d]))
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits(out.cpu().numpy(), _want(oracle, case, _expand(fresh)), ("replay", rep))
        it.finish()
    finally:
        it.close()


def _exact_grids(kind, shape, rng):
    grids = []
    for d, n in enumerate(shape):
        g = -1.0 + 0.125 * np.arange(n)  # exactly equal spacings: `interpn` takes the grid for regular
        if kind == "rectilinear":
            g[1:-1] += rng.uniform(-0.03, 0.03, n - 2)
        grids.append(g)
    return grids


@pytest.mark.parametrize("method", ["linear", "cubic", "nearest"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_interpn_lattice_entry_point(kind, method):
    import torch

    import interpn_amd

    rng = np.random.default_rng(41)
    shape = [9, 12, 17]
    grids = _exact_grids(kind, shape, rng)
    assert interpn_amd._check_regular(grids) == (kind == "regular")
    vals = rng.uniform(-1, 1, shape)
    lens = [6, 5, 70]
    inside = [np.sort(rng.uniform(g[0], g[-1], m)) for g, m in zip(grids, lens)]
    beyond = [a.copy() for a in inside]
    beyond[1][2] = grids[1][-1] + 0.5
    for axes in (inside, beyond):
        mesh = np.meshgrid(*axes, indexing="ij")
        want = interpn_amd.interpn(mesh, grids, vals, method=method)
        got = interpn_amd.interpn_lattice(axes, grids, vals, method=method)
        assert got.shape == tuple(lens)
        _assert_bits(got, want, ("interpn_lattice", kind, method))
        out = np.zeros(lens)
        assert interpn_amd.interpn_lattice(axes, grids, vals, method=method, out=out) is out
        _assert_bits(out, want, "out=")
        got_t = interpn_amd.interpn_lattice(_tensors(axes), grids, vals, method=method)
        assert isinstance(got_t, torch.Tensor) and tuple(got_t.shape) == tuple(lens)
        _assert_bits(got_t.cpu().numpy(), want, "torch input")
    _assert_bits(interpn_amd.interpn_lattice(inside, grids, vals, method=method, check_bounds=True),
                 interpn_amd.interpn(np.meshgrid(*inside, indexing="ij"), grids, vals, method=method), "check_bounds, inside")
    with pytest.raises(ValueError, match="Observation points violate interpolator bounds"):
        interpn_amd.interpn_lattice(beyond, grids, vals, method=method, check_bounds=True)
    with pytest.raises(ValueError, match="Observation points violate interpolator bounds"):
        interpn_amd.interpn_lattice(_tensors(beyond), grids, vals, method=method, check_bounds=True)


def test_classes_eval_lattice():
    import interpn_amd

    rng = np.random.default_rng(43)
    shape = [9, 12, 17]
    lens = [6, 5, 70]
    for kind in ("regular", "rectilinear"):
        grids = _exact_grids(kind, shape, rng)
        vals = rng.uniform(-1, 1, int(np.prod(shape)))
        axes = [rng.uniform(g[0] - 0.1, g[-1] + 0.1, m) for g, m in zip(grids, lens)]
        points = _expand(axes)
        dims = shape
        starts = np.array([g[0] for g in grids])
        steps = np.array([g[1] - g[0] for g in grids])
        if kind == "regular":
            objs = [interpn_amd.MultilinearRegular.new(dims, starts, steps, vals), interpn_amd.MulticubicRegular.new(dims, starts, steps, vals),
                    interpn_amd.NearestRegular.new(dims, starts, steps, vals)]
        else:
            objs = [interpn_amd.MultilinearRectilinear.new(grids, vals), interpn_amd.MulticubicRectilinear.new(grids, vals),
                    interpn_amd.NearestRectilinear.new(grids, vals)]
        for obj in objs:
            want = obj.eval(points)
            got = obj.eval_lattice(axes)
            assert got.shape == tuple(lens)
            _assert_bits(got, want, (type(obj).__name__, "numpy"))
            got_t = obj.eval_lattice(_tensors(axes))
            _assert_bits(got_t.cpu().numpy(), want, (type(obj).__name__, "torch"))


FULL = [("linear", 464), ("cubic", 216)]


@pytest.mark.parametrize("method,m", FULL, ids=["linear-464", "cubic-216"])
def test_full_size_regrid(oracle, method, m):
    """64^3 -> m^3 in f64 on a regular grid: the fused result equals the handle's eval_tensors on device-expanded points over
    the whole batch, and 5e5 sampled points equal the oracle."""
    import torch

    case = _grid_case(method, "regular", [64, 64, 64], np.float64, seed=47)
    rng = np.random.default_rng(48)
    axes = []
    for d in range(3):
        g = case.grids[d]
        a = np.linspace(g[0] - 0.02, g[-1] + 0.02, m)
        a[rng.integers(0, m, 8)] = g[rng.integers(0, 64, 8)]  # exact knots
        axes.append(a)
    it = _make(case)
    try:
        it.set_option("lattice", 1)
        ax_t = _tensors(axes)
        got = it.eval_lattice_tensors(ax_t)
        it.finish()
        assert it.last_lattice_path == "fused" and tuple(got.shape) == (m, m, m)
        mesh = [t.reshape(-1).contiguous() for t in torch.meshgrid(*ax_t, indexing="ij")]
        ref = it.eval_tensors(mesh)
        it.finish()
        assert torch.equal(got.reshape(-1).view(torch.int64), ref.view(torch.int64))
        del mesh, ref
        idx = rng.integers(0, m**3, 500_000)
        i, j, k = np.unravel_index(idx, (m, m, m))
        sample = [axes[0][i], axes[1][j], axes[2][k]]
        _assert_bits(got.reshape(-1)[torch.from_numpy(idx).to("cuda:0")].cpu().numpy(), _want(oracle, case, sample), ("sampled", method))
    finally:
        it.close()


def test_argument_errors_with_a_handle():
    """The wrong number of coordinate vectors takes the arm of `interp` on the wrong number of arrays: "Dimension
    mismatch" for linear and nearest, the flattened cubic arm's panic for multicubic N <= 4.  one_dim handles have no
    lattice form; an empty axis means no points."""
    import torch

    import interpn_amd

    lin = _make(_grid_case("linear", "regular", SHAPES[3], np.float64, seed=1))
    cub = _make(_grid_case("cubic", "rectilinear", SHAPES[3], np.float64, seed=1))
    one = interpn_amd.Interpolator.grid1d_regular("Linear1D", 0.0, 1.0, np.arange(5.0))
    try:
        two = [np.zeros(3), np.zeros(4)]
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            lin.eval_lattice_host(two)
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            lin.eval_lattice_tensors(_tensors(two))
        with pytest.raises(interpn_amd._lib.ReferencePanic):
            cub.eval_lattice_host(two)
        with pytest.raises(interpn_amd._lib.ReferencePanic):
            cub.reserve_lattice([3, 4])
        with pytest.raises(interpn_amd._lib.InterpnHipError):
            one.eval_lattice_host([np.zeros(3)])
        empty = lin.eval_lattice_host([np.zeros(3), np.zeros(0), np.zeros(4)])
        assert empty.shape == (3, 0, 4) and lin.last_lattice_path is None
        out = torch.full((5,), 7.0, dtype=torch.float64, device="cuda:0")
        res = lin.eval_lattice_tensors(_tensors([np.zeros(0), np.zeros(3), np.zeros(4)]))
        lin.finish()
        assert tuple(res.shape) == (0, 3, 4) and (out == 7.0).all()
    finally:
        lin.close()
        cub.close()
        one.close()
