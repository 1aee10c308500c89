"""Gradients on a lattice on the GPU (interpn_hip_eval_lattice_grad_*): everything is compared BIT FOR BIT, at the handle's
fma flavour, with
  (a) the gradient definitions restated in numpy (tests/grad_restatement.py, tests/cubic_grad_restatement.py) on the
      `np.meshgrid(..., indexing="ij")`-expanded points,
  (b) the oracle for the value, and
  (c) the same handle's `eval_grad_tensors` / `eval_cubic_grad_tensors` on the expanded points,
on the fused path (interpn::k_lattice_axes + interpn::k_lattice_grad_rows) and on the expanded one.

Wall time of the whole file on one MI355X: see DESIGN.md, "Gradients on a lattice".
"""

import contextlib
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cubic_grad_restatement, grad_restatement  # noqa: E402
from tests.test_lattice_gpu import (CLASSES, FUSED, LATTICE, SHAPES, _assert_bits, _axes, _classes, _exact_grids, _expand,  # noqa: E402
                                    _formula, _grid_case, _make, _tensors, _want)

pytestmark = pytest.mark.gpu

ROWS_KERNEL = "interpn::k_lattice_grad_rows<"
LENGTH_CASES = [("linear", "regular", 3, np.float64), ("cubic", "rectilinear", 2, np.float32)]


def _restated(case, points, fma=True):
    """Reference (a): (value, gradient (N, n)) of the definition on the expanded points."""
    c = dataclasses.replace(case, obs=points)
    mod = cubic_grad_restatement if case.method == "cubic" else grad_restatement
    out, grad, _ok = mod.eval_grad_case(c, fma=fma)
    return out, grad


def _product(it, case, points):
    """Reference (c): the per-point gradient kernels of the same handle on the expanded points."""
    call = it.eval_cubic_grad_tensors if case.method == "cubic" else it.eval_grad_tensors
    out, grad = call(_tensors(points))
    it.finish()
    return out.cpu().numpy(), grad.cpu().numpy()


def _eval(it, axes, **kw):
    out, grad = it.eval_lattice_grad_tensors(_tensors(axes), **kw)
    it.finish()
    return out.cpu().numpy(), grad.cpu().numpy()


def _kernel(dtype, method, n, kind, fma):
    return (f"{ROWS_KERNEL}{'double' if dtype == np.float64 else 'float'}, {0 if method == 'linear' else 1}, {n}, "
            f"{'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>")


def _assert_all(got, want_out, want_grad, ctx):
    out, grad = got
    _assert_bits(out, want_out, (ctx, "value"))
    n = grad.shape[0]
    for d in range(n):
        _assert_bits(grad[d], np.asarray(want_grad)[d], (ctx, "component", d))


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("method,linearize", FUSED, ids=["linear", "cubic-nolin", "cubic-lin"])
def test_fused_instantiations(oracle, method, linearize, n, kind, dtype, fma):
    case = _grid_case(method, kind, SHAPES[n], dtype, seed=3 * n + len(method), linearize=linearize)
    lens = LATTICE[n]
    axes = _axes(case, lens, seed=100 + n)
    for d in range(n):
        assert _classes(case, d, axes[d]) == set(CLASSES), (d, _classes(case, d, axes[d]))
    points = _expand(axes)
    want_out, want_grad = _restated(case, points, fma)
    _assert_bits(want_out, _want(oracle, case, points, fma), ("restated value vs oracle", method, n, kind))
    it = _make(case, fma)
    try:
        it.set_option("lattice", 1)
        dev = _eval(it, axes)
        assert dev[0].shape == tuple(lens) and dev[1].shape == (n,) + tuple(lens)
        assert it.last_lattice_path == "fused"
        assert it.kernel_name() == _kernel(dtype, method, n, kind, fma), it.kernel_name()
        host = it.eval_lattice_grad_host(axes)
        assert host[0].shape == tuple(lens) and host[1].shape == (n,) + tuple(lens) and it.last_lattice_path == "fused"
        _assert_all(dev, want_out, want_grad, ("fused device vs definition", method, n, kind))
        _assert_all(host, want_out, want_grad, ("fused host vs definition", method, n, kind))
        prod_out, prod_grad = _product(it, case, points)
        _assert_all(dev, prod_out, prod_grad, ("fused device vs per-point kernels", method, n, kind))
        value = it.eval_lattice_tensors(_tensors(axes))
        it.finish()
        _assert_bits(dev[0], value.cpu().numpy(), ("fused value vs eval_lattice", method, n, kind))
    finally:
        it.close()


def _guarded(shape, n, dtype, sentinel, guard):
    import torch

    count = int(np.prod(shape))
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    big_out = torch.full((count + 2 * guard,), sentinel, dtype=tdt, device="cuda:0")
    big_grad = torch.full((n, count + 2 * guard), sentinel, dtype=tdt, device="cuda:0")
    return big_out, big_grad, big_out[guard:guard + count].view(shape), big_grad[:, guard:guard + count].view((n,) + tuple(shape))


def _check_guarded(it, case, axes, mode, ctx):
    """One evaluation into sentinel-filled buffers: guards intact, bits those of the definition and of the product path."""
    lens = [a.size for a in axes]
    n = len(lens)
    dtype = case.vals.dtype.type
    points = _expand(axes)
    want_out, want_grad = _restated(case, points)
    count, guard, sentinel = want_out.size, 3, -12345.5
    big_out, big_grad, out, grad = _guarded(lens, n, dtype, sentinel, guard)
    it.set_option("lattice", mode)
    it.eval_lattice_grad_tensors(_tensors(axes), out=out, grad=grad)
    it.finish()
    assert it.last_lattice_path == ("fused" if mode else "expanded"), ctx
    got_out, got_grad = big_out.cpu().numpy(), big_grad.cpu().numpy()
    assert (got_out[:guard] == sentinel).all() and (got_out[guard + count:] == sentinel).all(), ctx
    assert (got_grad[:, :guard] == sentinel).all() and (got_grad[:, guard + count:] == sentinel).all(), ctx
    got = (got_out[guard:guard + count], got_grad[:, guard:guard + count])
    _assert_all(got, want_out, want_grad, (ctx, "definition"))
    prod_out, prod_grad = _product(it, case, points)
    _assert_all(got, prod_out, prod_grad, (ctx, "per-point kernels"))
    return got


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "expanded"])
@pytest.mark.parametrize("other", [1, 2, 7])
@pytest.mark.parametrize("last", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("method,kind,n,dtype", LENGTH_CASES, ids=["linear3-regular-f64", "cubic2-rectilinear-f32"])
def test_axis_lengths_and_guards(oracle, method, kind, n, dtype, last, other, mode):
    case = _grid_case(method, kind, SHAPES[n], dtype, seed=11, linearize=True)
    lens = [other] * (n - 1) + [last]
    axes = _axes(case, lens, seed=last + other)
    it = _make(case)
    try:
        got = _check_guarded(it, case, axes, mode, ("lengths", lens, mode))
        _assert_bits(got[0], _want(oracle, case, _expand(axes)), ("lengths, oracle", lens, mode))
    finally:
        it.close()


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "expanded"])
@pytest.mark.parametrize("n_last", ["min", 65])
@pytest.mark.parametrize("method,kind,n,dtype", LENGTH_CASES, ids=["linear3-regular-f64", "cubic2-rectilinear-f32"])
def test_last_grid_axis_lengths(oracle, method, kind, n, dtype, n_last, mode):
    """The method's minimum (multilinear 2: the difference line has ONE entry; multicubic 4) and 65, the second trip of the
    lane loop over the grid columns."""
    if n_last == "min":
        n_last = 2 if method == "linear" else 4
    shape = SHAPES[n][:-1] + [n_last]
    case = _grid_case(method, kind, shape, dtype, seed=13, linearize=True)
    lens = [5] * (n - 1) + [70]
    axes = _axes(case, lens, seed=n_last)
    it = _make(case)
    try:
        got = _check_guarded(it, case, axes, mode, ("last grid axis", shape, mode))
        _assert_bits(got[0], _want(oracle, case, _expand(axes)), ("last grid axis, oracle", shape, mode))
    finally:
        it.close()


@pytest.mark.parametrize("method,kind", [("linear", "regular"), ("cubic", "rectilinear")])
def test_a_wave_takes_more_than_one_row(oracle, method, kind):
    case = _grid_case(method, kind, [9, 11], np.float64, seed=7, linearize=True)
    it = _make(case)
    try:
        slots = 4 * it.get_option("dev_num_cus") * it.get_option("blocks_per_cu")  # rows of one pass of the persistent grid
        rows = max(8200, slots + 8)
        assert rows > slots
        axes = _axes(case, [rows, 3], seed=5)
        points = _expand(axes)
        it.set_option("lattice", 1)
        got = _eval(it, axes)
        assert it.last_lattice_path == "fused"
        _assert_all(got, *_restated(case, points), ("rows", method))
        _assert_all(got, *_product(it, case, points), ("rows, per-point kernels", method))
        _assert_bits(got[0], _want(oracle, case, points), ("rows, oracle", method))
    finally:
        it.close()


@pytest.mark.parametrize("method,dtype", [("linear", np.float64), ("linear", np.float32), ("cubic", np.float64), ("cubic", np.float32)],
                         ids=["linear-f64", "linear-f32", "cubic-f64", "cubic-f32"])
def test_last_axis_at_the_lds_budget(oracle, method, dtype):
    """4 waves x round16(L lines x n_last elements) against the budget (option axis_lds_kb): the boundary, computed from
    the option, with the same bits on both sides of it where the lattices coincide."""
    kb, n = 1, 3
    lines = n + 1 if method == "linear" else n
    inside = kb * 1024 // (4 * lines * np.dtype(dtype).itemsize)
    assert 4 * ((lines * inside * np.dtype(dtype).itemsize + 15) // 16 * 16) <= kb * 1024
    assert 4 * ((lines * (inside + 1) * np.dtype(dtype).itemsize + 15) // 16 * 16) > kb * 1024
    for n_last, path in ((inside, "fused"), (inside + 1, "expanded")):
        shape = [5, 6, n_last]
        case = _grid_case(method, "regular", shape, dtype, seed=n_last, linearize=True)
        axes = _axes(case, [4, 5, 90], seed=n_last)
        points = _expand(axes)
        it = _make(case)
        try:
            it.set_option("axis_lds_kb", kb)
            it.set_option("lattice", 1)
            got = _eval(it, axes)
            assert it.last_lattice_path == path, (n_last, it.last_lattice_path)
            assert it.kernel_name().startswith(ROWS_KERNEL) == (path == "fused")
            _assert_all(got, *_restated(case, points), ("lds boundary", n_last))
            _assert_all(got, *_product(it, case, points), ("lds boundary vs per-point kernels", n_last))
            _assert_bits(got[0], _want(oracle, case, points), ("lds boundary, oracle", n_last))
        finally:
            it.close()


EXPANDED = [("linear", [301], [1500], {}), ("cubic", [301], [1500], {}),
            ("linear", [5, 4, 6, 7], [4, 3, 5, 6], {}), ("cubic", [5, 4, 6, 7], [4, 3, 5, 6], {}),
            ("linear", [17, 12, 23], [11, 13, 71], {"lattice": 0}), ("cubic", [37, 53], [41, 67], {"lattice": 0}),
            ("linear", [17, 12, 23], [11, 13, 71], {"force_generic": 1}), ("cubic", [37, 53], [41, 67], {"force_generic": 1}),
            ("linear", [5, 6, 700], [4, 5, 90], {"axis_lds_kb": 1}), ("cubic", [6, 700], [40, 90], {"axis_lds_kb": 1})]


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,shape,lens,options", EXPANDED,
                         ids=[f"{m}-N{len(s)}-{'-'.join(o) or 'uncovered'}" for m, s, _, o in EXPANDED])
def test_expanded_path(oracle, method, shape, lens, options, kind):
    case = _grid_case(method, kind, shape, np.float64, seed=17 + len(shape), linearize=method == "cubic")
    axes = _axes(case, lens, seed=len(shape))
    points = _expand(axes)
    it = _make(case)
    try:
        it.set_option("lattice", 1)  # "wherever covered and fitting": none of these is
        for name, value in options.items():
            it.set_option(name, value)
        dev = _eval(it, axes)
        assert dev[0].shape == tuple(lens) and it.last_lattice_path == "expanded"
        assert not it.kernel_name().startswith(ROWS_KERNEL)
        host = it.eval_lattice_grad_host(axes)
        _assert_all(dev, *_restated(case, points), ("expanded vs definition", method, shape))
        _assert_all(dev, *_product(it, case, points), ("expanded vs per-point kernels", method, shape))
        _assert_bits(dev[0], _want(oracle, case, points), ("expanded vs oracle", method, shape))
        _assert_all(host, dev[0], dev[1], ("expanded host", method, shape))
    finally:
        it.close()


def test_several_expanded_slices(oracle):
    """Two slices of the expanded path (64 MiB of coordinates each), as in
    test_lattice_gpu.py::test_first_failure_behind_the_first_expanded_slice: every component lands at its slice's offset,
    and the reported failing index is the lattice's, not the slice's."""
    lens = [180, 180, 180]
    case = _grid_case("linear", "regular", [9, 7, 11], np.float32, seed=2)
    axes = _axes(case, lens, seed=3)
    assert int(np.prod(lens)) > 64 * 2**20 // (3 * 4)
    it = _make(case)
    try:
        it.set_option("lattice", 0)
        points = _expand(axes)
        got = _eval(it, axes)
        assert it.last_lattice_path == "expanded"
        _assert_all(got, *_product(it, case, points), "two slices")
        it.set_option("lattice", 1)
        fused = _eval(it, axes)
        assert it.last_lattice_path == "fused"
        _assert_all(fused, got[0], got[1], "two slices vs fused")
        it.set_option("lattice", 0)
        axes[0][179] = np.nan
        it.eval_lattice_grad_tensors(_tensors(axes))
        with pytest.raises(AssertionError) as e:
            it.finish()
        assert e.value.first_bad_index == 179 * 180 * 180
    finally:
        it.close()


BAD_SETS = [[(0, 5)], [(1, 3)], [(2, 7)], [(0, 6), (2, 2)]]
FAILING = [("linear", 1), ("cubic", 1), ("linear", 0), ("cubic", 0)]
_CLEAN = {}


def _clean_reference(oracle, method):
    """The failing-point tests share one lattice per method: its definition and oracle value, computed once."""
    if method not in _CLEAN:
        case = _grid_case(method, "regular", [17, 12, 23], np.float64, seed=23)
        lens = [9, 8, 45]
        clean = _axes(case, lens, seed=9)
        points = _expand(clean)
        want_out, want_grad = _restated(case, points)
        _assert_bits(want_out, _want(oracle, case, points), "restated value vs oracle")
        _CLEAN[method] = (case, lens, clean, want_out, want_grad)
    return _CLEAN[method]


@pytest.mark.parametrize("value", [np.nan, np.inf, 1e300], ids=["nan", "inf", "1e300"])
@pytest.mark.parametrize("bad", BAD_SETS, ids=["axis0", "middle", "last", "two"])
@pytest.mark.parametrize("method,mode", FAILING, ids=["linear-fused", "cubic-fused", "linear-expanded", "cubic-expanded"])
def test_failing_points_on_regular_grids(oracle, method, mode, bad, value):
    case, lens, clean, want_out, want_grad = _clean_reference(oracle, method)
    axes = [a.copy() for a in clean]
    for d, j in bad:
        axes[d][j] = value
    first = _formula(lens, bad)
    it = _make(case)
    try:
        it.set_option("lattice", mode)
        it.eval_lattice_grad_tensors(_tensors(axes))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
            it.finish()
        assert e.value.first_bad_index == first, (e.value.first_bad_index, first)
        assert it.last_lattice_path == ("fused" if mode else "expanded")
        # host form, in one chunk and with the failure behind the first chunk: exactly the prefix, the rest as it was
        sentinel = -777.25
        per0 = lens[1] * lens[2]
        for chunk in (0, 2 * per0):
            if chunk:
                if first < chunk:
                    continue
                it.set_option("host_chunk", chunk)
            out, grad = np.full(lens, sentinel), np.full([3] + lens, sentinel)
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
                it.eval_lattice_grad_host(axes, out, grad)
            assert e.value.first_bad_index == first, (chunk, e.value.first_bad_index, first)
            _assert_bits(out.ravel()[:first], want_out[:first], ("prefix", bad, chunk))
            assert (out.ravel()[first:] == sentinel).all()
            for d in range(3):
                _assert_bits(grad[d].ravel()[:first], want_grad[d][:first], ("prefix", bad, chunk, d))
                assert (grad[d].ravel()[first:] == sentinel).all()
        # the status word is cleared: a clean lattice afterwards is clean, in chunks as in one piece
        _assert_all(_eval(it, clean), want_out, want_grad, ("clean after failure", bad))
        _assert_all(it.eval_lattice_grad_host(clean), want_out, want_grad, ("clean host after failure", bad))
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
        got = _eval(it, axes)  # finish() inside: no failure reported
        host = it.eval_lattice_grad_host(axes)
        prod_out, prod_grad = _product(it, case, points)
        expect_nan = np.zeros(lens, dtype=bool)
        expect_nan[2, :, :] = True
        expect_nan[:, :, 31] = True
        assert np.array_equal(np.isnan(got[0]), expect_nan) and np.array_equal(np.isnan(host[0]), expect_nan)
        want_out, want_grad = _restated(case, points)
        keep = ~expect_nan.ravel()
        _assert_bits(got[0].ravel()[keep], want_out[keep], "beside the NaN planes")
        _assert_bits(host[0].ravel()[keep], want_out[keep], "beside the NaN planes, host")
        for d in range(3):
            # a component is NaN exactly where the per-point kernels' is (component d does not use coordinate d's t)
            nan_d = np.isnan(prod_grad[d])
            assert nan_d[~keep].any()
            assert np.array_equal(np.isnan(got[1][d].ravel()), nan_d) and np.array_equal(np.isnan(host[1][d].ravel()), nan_d)
            _assert_bits(got[1][d].ravel()[keep], want_grad[d][keep], ("beside the NaN planes", d))
            _assert_bits(got[1][d].ravel()[~nan_d], prod_grad[d][~nan_d], ("wherever a number, per-point kernels", d))
            _assert_bits(host[1][d].ravel()[~nan_d], prod_grad[d][~nan_d], ("wherever a number, host", d))
    finally:
        it.close()


@contextlib.contextmanager
def _side_streams(count):
    """`count` non-blocking streams made by the HIP runtime itself and destroyed afterwards, wrapped for torch.  Not
    `torch.cuda.Stream()`: that hands out the next stream of torch's fixed pool, so every call here would move the pair of
    pool streams that each later test of the process draws (tests/test_step_commands_gpu.py needs two that run side by
    side)."""
    import torch

    import interpn_amd

    hip = interpn_amd._lib.load()  # the library's handle resolves the symbols of the HIP runtime it is bound to
    raws = []
    try:
        for _ in range(count):
            raw = ctypes.c_void_p()
            assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), ctypes.c_uint(1)) == 0  # hipStreamNonBlocking
            raws.append(raw)
        yield [torch.cuda.ExternalStream(raw.value) for raw in raws]
    finally:
        torch.cuda.synchronize()
        for raw in raws:
            hip.hipStreamDestroy(raw)


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "expanded"])
def test_streams_reserve_and_capture(oracle, mode):
    import torch

    import interpn_amd

    lens = [12, 9, 130]
    case = _grid_case("linear", "rectilinear", SHAPES[3], np.float64, seed=31)
    axes = _axes(case, lens, seed=6)
    want_out, want_grad = _restated(case, _expand(axes))
    with _side_streams(2) as (side, other):  # destroyed after the handle that has used them is closed
        it = _make(case)
        try:
            it.set_option("lattice", mode)
            # no_alloc without a reserved block: an error, not a silent allocation
            with pytest.raises(interpn_amd._lib.InterpnHipError):
                it.eval_lattice_grad_tensors(_tensors(axes), no_alloc=True)
            it.reserve_lattice(lens, 1)  # the value call's reserve serves gradient calls
            allocs = it.get_option("scratch_allocs")
            assert allocs >= 1
            got = _eval(it, axes, no_alloc=True)
            assert it.get_option("scratch_allocs") == allocs
            _assert_all(got, want_out, want_grad, "no_alloc after reserve")
            # two side streams: torch's current one, and one given explicitly
            ax_t = _tensors(axes)
            out = torch.zeros(lens, dtype=torch.float64, device="cuda:0")
            grad = torch.zeros([3] + lens, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                it.eval_lattice_grad_tensors(ax_t, out, grad)
            it.finish()
            _assert_all((out.cpu().numpy(), grad.cpu().numpy()), want_out, want_grad, "side stream")
            out.zero_()
            grad.zero_()
            torch.cuda.synchronize()
            it.eval_lattice_grad_tensors(ax_t, out, grad, stream=other)
            it.finish(other)
            _assert_all((out.cpu().numpy(), grad.cpu().numpy()), want_out, want_grad, "stream=")
            if mode:
                # one fused evaluation captured on a single stream after the reserve, replayed twice on new coordinates
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    it.eval_lattice_grad_tensors(ax_t, out, grad)
                assert it.last_lattice_path == "fused"
                for rep in range(2):
                    fresh = _axes(case, lens, seed=50 + rep)
                    for d in range(3):
                        ax_t[d].copy_(torch.from_numpy(fresh[d]))
                    out.zero_()
                    grad.zero_()
                    graph.replay()
                    torch.cuda.synchronize()
                    _assert_all((out.cpu().numpy(), grad.cpu().numpy()), *_restated(case, _expand(fresh)), ("replay", rep))
                it.finish()
        finally:
            it.close()


def test_unsupported_handles_and_null_gradient():
    import interpn_amd

    case = _grid_case("nearest", "regular", [9, 7, 11], np.float64, seed=1)
    axes = _axes(case, [4, 5, 6], seed=1)
    it = _make(case)
    try:
        with pytest.raises(interpn_amd._lib.InterpnHipError, match="(?i)unsupported"):
            it.eval_lattice_grad_host(axes)
        with pytest.raises(interpn_amd._lib.InterpnHipError, match="(?i)unsupported"):
            it.eval_lattice_grad_tensors(_tensors(axes))
    finally:
        it.close()
    case = _grid_case("linear", "regular", [9, 7, 11], np.float64, seed=1)
    it = _make(case)
    try:
        out, grad = it.eval_lattice_grad_host([axes[0], axes[1][:0], axes[2]])  # an empty axis: nothing to do
        assert out.shape == (4, 0, 6) and grad.shape == (3, 4, 0, 6)
        with pytest.raises(AssertionError):  # two vectors for three axes
            it.eval_lattice_grad_host(axes[:2])
    finally:
        it.close()


@pytest.mark.parametrize("method", ["linear", "cubic"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_python_surface(kind, method):
    import torch

    import interpn_amd

    rng = np.random.default_rng(41)
    shape = [9, 12, 17]
    grids = _exact_grids(kind, shape, rng)
    vals = rng.uniform(-1, 1, shape)
    lens = [6, 5, 70]
    axes = [rng.uniform(g[0] - 0.1, g[-1] + 0.1, m) for g, m in zip(grids, lens)]
    mesh = np.meshgrid(*axes, indexing="ij")
    want_out, want_grad = interpn_amd.interpn_grad(mesh, grids, vals, method=method)
    got = interpn_amd.interpn_lattice_grad(axes, grids, vals, method=method)
    assert got[0].shape == tuple(lens) and got[1].shape == (3,) + tuple(lens)
    _assert_all(got, want_out, want_grad, ("interpn_lattice_grad", kind, method))
    _assert_bits(got[0], interpn_amd.interpn_lattice(axes, grids, vals, method=method), "value vs interpn_lattice")
    got_t = interpn_amd.interpn_lattice_grad(_tensors(axes), grids, vals, method=method)
    assert all(isinstance(t, torch.Tensor) for t in got_t)
    _assert_all((got_t[0].cpu().numpy(), got_t[1].cpu().numpy()), want_out, want_grad, "torch input")
    with pytest.raises(ValueError, match="Observation points violate interpolator bounds"):
        interpn_amd.interpn_lattice_grad(axes, grids, vals, method=method, check_bounds=True)
    # the classes
    flat = vals.ravel()
    starts = np.array([g[0] for g in grids])
    steps = np.array([g[1] - g[0] for g in grids])
    if kind == "regular":
        cls = interpn_amd.MultilinearRegular if method == "linear" else interpn_amd.MulticubicRegular
        obj = cls.new(shape, starts, steps, flat)
    else:
        cls = interpn_amd.MultilinearRectilinear if method == "linear" else interpn_amd.MulticubicRectilinear
        obj = cls.new(grids, flat)
    points = _expand(axes)
    ref = obj.eval_grad(points) if method == "linear" else obj.eval_cubic_grad(points)
    res = obj.eval_lattice_grad(axes)
    _assert_all(res, ref[0], ref[1], (cls.__name__, "numpy"))
    out = np.zeros(lens)
    grad = np.zeros([3] + lens)
    back = obj.eval_lattice_grad(axes, out, grad)
    assert back[0] is out and back[1] is grad
    _assert_all(back, ref[0], ref[1], (cls.__name__, "numpy out="))
    res_t = obj.eval_lattice_grad(_tensors(axes))
    _assert_all((res_t[0].cpu().numpy(), res_t[1].cpu().numpy()), ref[0], ref[1], (cls.__name__, "torch"))
    out_t = torch.zeros(lens, dtype=torch.float64, device="cuda:0")
    grad_t = torch.zeros([3] + lens, dtype=torch.float64, device="cuda:0")
    back_t = obj.eval_lattice_grad(_tensors(axes), out_t, grad_t)
    assert back_t[0] is out_t and back_t[1] is grad_t
    _assert_all((out_t.cpu().numpy(), grad_t.cpu().numpy()), ref[0], ref[1], (cls.__name__, "torch out="))


@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_autograd_interp_lattice(method):
    """A table of small integers on a unit-step grid, axes at dyadic fractions inside it: every product and sum of the
    forward and the backward pass is exact, so the sum over the other lattice dimensions cannot depend on its order."""
    import torch

    import interpn_amd
    from interpn_amd import autograd

    rng = np.random.default_rng(3)
    shape = [6, 7, 9]
    vals = rng.integers(-4, 5, shape).astype(np.float64)
    it = interpn_amd.Interpolator.regular(method, shape, np.zeros(3), np.ones(3), vals.ravel(), dtype=np.float64)
    try:
        lens = [5, 4, 70]
        axes = [torch.from_numpy(rng.integers(8, 8 * (n - 2), m) / 8.0).to("cuda:0").requires_grad_(True) for n, m in zip(shape, lens)]
        mesh = [a.detach().clone().requires_grad_(True) for a in axes]
        weights = torch.from_numpy(rng.integers(-3, 4, lens).astype(np.float64)).to("cuda:0")
        res = autograd.interp_lattice(it, axes)
        assert tuple(res.shape) == tuple(lens)
        (res * weights).sum().backward()
        expanded = torch.meshgrid(*mesh, indexing="ij")
        ref = autograd.interp(it, expanded)
        (ref * weights).sum().backward()
        assert torch.equal(res.detach(), ref.detach())
        for d in range(3):
            assert axes[d].grad is not None and axes[d].grad.shape == axes[d].shape
            assert torch.equal(axes[d].grad, mesh[d].grad), (d, axes[d].grad, mesh[d].grad)
        assert any(bool((a.grad != 0).any()) for a in axes)
    finally:
        it.close()
