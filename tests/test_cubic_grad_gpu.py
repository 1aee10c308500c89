"""Multicubic value and gradient on the GPU (interpn_hip_eval_cubic_grad_*, Interpolator.eval_cubic_grad_*,
interpn_grad(method="cubic"), the classes' eval_cubic_grad, interpn_amd.autograd on a cubic handle) against the numpy
restatement of the definition (tests/cubic_grad_restatement.py, pinned on the CPU by tests/test_cubic_grad_cpu.py).  Every
comparison is bit for bit at the same fma flavour; a NaN need only be a NaN on both sides.  The value is compared with
`eval` as well."""

import functools
import itertools
from ctypes import c_size_t, c_void_p

import numpy as np
import pytest

from tests import cubic_grad_restatement as cg

pytestmark = pytest.mark.gpu

OK, DIM_MISMATCH, REFERENCE_PANIC, INVALID, UNSUPPORTED = 0, 1, 9, 32, 33
FUSED, GENERIC = "interpn::k_cubic_grad<", "interpn::k_cubic_grad_n<"
LAYOUTS = ["44", "24", "22", "14", "11"]  # every tile-step pair a cubic handle can have; "11" gathers by LDS-DMA
SHAPES = {2: [(4, 4), (5, 5), (6, 6), (7, 7), (4, 7)], 3: [(4, 4, 4), (5, 5, 5), (6, 6, 6), (7, 7, 7), (4, 7, 5)]}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_BRICKS", "INTERPN_HIP_FORCE_GENERIC", "INTERPN_HIP_HOST_CHUNK", "INTERPN_HIP_BLOCKS_PER_CU"):
        monkeypatch.delenv(name, raising=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist(), got[~same][:4], want[~same][:4])


# ---- workloads: dyadic regular axes (start -1, step 1/2: knots are exact), rectilinear ones with jittered interior knots
def _axis(kind, n, d, dtype):
    g = -1.0 + 0.5 * np.arange(n)
    if kind == "rectilinear":
        j = (np.random.default_rng(1000 + 10 * n + d).random(n) - 0.5) * 0.25
        j[0] = j[-1] = 0.0
        g = g + j
    return g.astype(dtype)


def _axis_coords(g):
    """One coordinate per class and per boundary of the cell rule: more than one cell below the grid, just below it, inside
    the first cell, exactly on knots 0, 1, n - 2, n - 1, interior, inside the last cell, just above the grid, more than one
    cell above."""
    g = g.astype(np.float64)
    n = g.size
    h0, h1 = g[1] - g[0], g[-1] - g[-2]
    mid = (n - 1) // 2
    c = [g[0] - 1.625 * h0, g[0] - 0.25 * h0, g[0] + 0.375 * h0, g[0], g[1], g[-2], g[-1], g[mid] + 0.3 * (g[mid + 1] - g[mid]),
         g[1] + 0.71 * (g[2] - g[1]), g[-1] - 0.375 * h1, g[-1] + 0.25 * h1, g[-1] + 2.125 * h1]
    return np.array(c)


@functools.lru_cache(maxsize=None)
def _workload(kind, shape, dtype_name, fill):
    """(grids, vals, obs): the full cross product of the axes' coordinate sets, then random points over the grid widened by
    40 % up to `fill` points in all (not a multiple of 256)."""
    dtype = np.dtype(dtype_name)
    n = len(shape)
    rng = np.random.default_rng(4000 + sum((d + 1) * s for d, s in enumerate(shape)) + (kind == "regular"))
    grids = [_axis(kind, shape[d], d, dtype) for d in range(n)]
    vals = rng.uniform(-1.0, 1.0, int(np.prod(shape))).astype(dtype)
    cross = np.array(list(itertools.product(*[_axis_coords(g) for g in grids]))).T  # (n, 12^n)
    assert cross.shape[1] < fill and fill % 256 != 0
    obs = []
    for d in range(n):
        lo, hi = float(grids[d][0]), float(grids[d][-1])
        w = 0.4 * (hi - lo)
        obs.append(np.concatenate([cross[d], rng.uniform(lo - w, hi + w, fill - cross.shape[1])]).astype(dtype))
    return grids, vals, obs


def _grid_args(kind, grids, dtype):
    if kind == "regular":
        return ([g.size for g in grids], np.array([g[0] for g in grids], dtype=dtype), np.array([g[1] - g[0] for g in grids], dtype=dtype))
    return [np.asarray(g, dtype=dtype) for g in grids]


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, dtype_name, fill, linearize, fma):
    """The restatement of one workload: computed once, shared by every layout and test that evaluates it."""
    grids, vals, obs = _workload(kind, shape, dtype_name, fill)
    out, grad, ok = cg.eval_grad(kind, _grid_args(kind, grids, np.dtype(dtype_name)), vals, obs, linearize=linearize, fma=fma,
                                 dtype=np.dtype(dtype_name))
    assert ok.all()
    out.setflags(write=False)
    grad.setflags(write=False)
    return out, grad


def _handle(kind, grids, vals, linearize=True, fma=True, method="cubic"):
    import interpn_amd

    dt = vals.dtype
    if kind == "regular":
        dims, starts, steps = _grid_args(kind, grids, dt)
        return interpn_amd.Interpolator.regular(method, dims, starts, steps, vals, linearize_extrapolation=linearize, dtype=dt, fma=fma)
    return interpn_amd.Interpolator.rectilinear(method, [np.asarray(g) for g in grids], vals, linearize_extrapolation=linearize,
                                                dtype=dt, fma=fma)


def _device(it, obs, out=None, grad=None, stream=None):
    import torch

    out_t, grad_t = it.eval_cubic_grad_tensors([torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in obs], out, grad, stream)
    it.finish()
    return out_t.cpu().numpy(), grad_t.cpu().numpy()


def _kernel_args(name):
    return [a.strip() for a in name[name.index("<") + 1:-1].split(",")]


FILL = {2: 700, 3: 2000}  # 144 / 1728 cross-product points + random fill: 3 and 8 workgroups, ragged tails


# ---- the fused kernel: every tile-step pair, grid shape, class, flavour
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", ["float64", "float32"], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [2, 3])
def test_fused_kernel_matches_the_restatement(n, kind, dtype, layout, monkeypatch):
    monkeypatch.setenv("INTERPN_HIP_BRICKS", layout)
    for shape in SHAPES[n]:
        grids, vals, obs = _workload(kind, shape, dtype, FILL[n])
        for linearize in (True, False):
            it = _handle(kind, grids, vals, linearize)
            try:
                assert it.table_layout()[0] > 0
                plain = it.eval_host(obs, np.zeros_like(obs[0]))
                for fma in (True, False):
                    it.set_option("fma", int(fma))
                    want_out, want_grad = _reference(kind, shape, dtype, FILL[n], linearize, fma)
                    out, grad = _device(it, obs)
                    name = it.kernel_name()
                    assert name.startswith(FUSED), name
                    args = _kernel_args(name)  # T, N, RECT, FMA, SI, SJ
                    assert args[1] == str(n) and args[2] == ("true" if kind == "rectilinear" else "false"), name
                    assert args[3] == ("true" if fma else "false") and args[4:6] == [layout[0], layout[1]], name
                    what = (shape, linearize, fma)
                    _assert_same(out, want_out, (what, "out"))
                    _assert_same(grad, want_grad, (what, "grad"))
                    if fma:
                        _assert_same(out, plain, (what, "value against eval"))
            finally:
                it.close()


@pytest.mark.parametrize("layout", ["24", "11"])
@pytest.mark.parametrize("dtype", ["float64", "float32"], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [2, 3])
def test_call_sizes_host_form_and_grid_stride(n, kind, dtype, layout, monkeypatch):
    """Calls of 1, 63, 64, 65 and 257 points (dead tail lanes take part in the gathers' exchanges), the host form, and a launch
    whose grid-stride loop iterates several times (one workgroup per CU, fewer workgroups than the call needs)."""
    monkeypatch.setenv("INTERPN_HIP_BRICKS", layout)
    shape = SHAPES[n][4]
    grids, vals, obs = _workload(kind, shape, dtype, FILL[n])
    want_out, want_grad = _reference(kind, shape, dtype, FILL[n], True, True)
    it = _handle(kind, grids, vals, True)
    try:
        for count in (0, 1, 63, 64, 65, 257):
            sub = [np.ascontiguousarray(o[:count]) for o in obs]
            out, grad = _device(it, sub)
            assert out.shape == (count,) and grad.shape == (n, count)
            _assert_same(out, want_out[:count], ("device", count))
            _assert_same(grad, want_grad[:, :count], ("device", count))
            hout, hgrad = it.eval_cubic_grad_host(sub)
            _assert_same(hout, want_out[:count], ("host", count))
            _assert_same(hgrad, want_grad[:, :count], ("host", count))
        # several trips of the grid-stride loop: the points repeated until they outnumber one workgroup per CU
        import torch

        cus = torch.cuda.get_device_properties(0).multi_processor_count
        reps = (2 * cus * 256) // obs[0].size + 2
        big = [np.tile(o, reps)[:-3] for o in obs]  # ragged
        it.set_blocks_per_cu(1)
        assert big[0].size > 2 * cus * 256
        out, grad = _device(it, big)
        assert it.kernel_name().startswith(FUSED)
        _assert_same(out, np.tile(want_out, reps)[:-3], "grid stride out")
        _assert_same(grad, np.tile(want_grad, (1, reps))[:, :-3], "grid stride grad")
        it.set_option("host_chunk", 40_000)
        hout, hgrad = it.eval_cubic_grad_host(big)
        _assert_same(hout, np.tile(want_out, reps)[:-3], "chunked host out")
        _assert_same(hgrad, np.tile(want_grad, (1, reps))[:, :-3], "chunked host grad")
    finally:
        it.close()


# ---- the runtime-N kernel
N_SHAPES = {1: (6,), 4: (4, 5, 6, 4), 5: (4, 5, 4, 4, 5)}


@functools.lru_cache(maxsize=None)
def _n_workload(kind, n, dtype_name):
    dtype = np.dtype(dtype_name)
    shape = N_SHAPES[n]
    rng = np.random.default_rng(5000 + n + (kind == "regular"))
    grids = [_axis(kind, shape[d], d, dtype) for d in range(n)]
    vals = rng.uniform(-1.0, 1.0, int(np.prod(shape))).astype(dtype)
    npts = 403
    obs = []
    for d in range(n):
        lo, hi = float(grids[d][0]), float(grids[d][-1])
        w = 0.4 * (hi - lo)
        o = rng.uniform(lo - w, hi + w, npts)
        c = _axis_coords(grids[d])
        o[:c.size] = np.roll(c, 5 * d)  # every class of every axis, de-correlated across the axes
        obs.append(o.astype(dtype))
    return grids, vals, obs


@pytest.mark.parametrize("linearize", [True, False], ids=["lin", "quad"])
@pytest.mark.parametrize("dtype", ["float64", "float32"], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 4, 5])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_runtime_n_kernel_matches_the_restatement(kind, n, dtype, linearize):
    grids, vals, obs = _n_workload(kind, n, dtype)
    it = _handle(kind, grids, vals, linearize)
    try:
        plain = it.eval_host(obs, np.zeros_like(obs[0]))
        for fma in (True, False):
            it.set_option("fma", int(fma))
            want_out, want_grad, ok = cg.eval_grad(kind, _grid_args(kind, grids, np.dtype(dtype)), vals, obs, linearize=linearize,
                                                   fma=fma, dtype=np.dtype(dtype))
            assert ok.all()
            out, grad = _device(it, obs)
            assert it.kernel_name().startswith(GENERIC), it.kernel_name()
            _assert_same(out, want_out, (fma, "device out"))
            _assert_same(grad, want_grad, (fma, "device grad"))
            hout, hgrad = it.eval_cubic_grad_host(obs)
            _assert_same(hout, want_out, (fma, "host out"))
            _assert_same(hgrad, want_grad, (fma, "host grad"))
            if fma:
                _assert_same(out, plain, "value against eval")
    finally:
        it.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_force_generic_and_no_table_give_the_fused_kernels_bits(kind, n, dtype, monkeypatch):
    shape = SHAPES[n][4]
    grids, vals, obs = _workload(kind, shape, dtype, FILL[n])
    want_out, want_grad = _reference(kind, shape, dtype, FILL[n], True, True)
    monkeypatch.setenv("INTERPN_HIP_BRICKS", "22")
    it = _handle(kind, grids, vals, True)
    try:
        out, grad = _device(it, obs)
        assert it.kernel_name().startswith(FUSED)
        it.set_option("force_generic", 1)
        gout, ggrad = _device(it, obs)
        assert it.kernel_name().startswith(GENERIC), it.kernel_name()
        for a, b, c in ((out, gout, want_out), (grad, ggrad, want_grad)):
            _assert_same(a, c, "fused")
            _assert_same(b, c, "force_generic")
    finally:
        it.close()
    monkeypatch.setenv("INTERPN_HIP_BRICKS", "off")
    it = _handle(kind, grids, vals, True)
    try:
        assert it.table_layout()[0] == 0
        oout, ograd = _device(it, obs)
        assert it.kernel_name().startswith(GENERIC), it.kernel_name()
        _assert_same(oout, want_out, "no table")
        _assert_same(ograd, want_grad, "no table")
    finally:
        it.close()


# ---- special values
@pytest.mark.parametrize("dtype", ["float64", "float32"], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_non_finite_inputs_propagate(kind, n, dtype, monkeypatch):
    if n in (2, 3):
        monkeypatch.setenv("INTERPN_HIP_BRICKS", "11" if n == 2 else "24")
        grids, vals, obs = _workload(kind, SHAPES[n][3], dtype, FILL[n])
    else:
        grids, vals, obs = _n_workload(kind, n, dtype)
    vals = vals.copy()
    obs = [o.copy() for o in obs]
    rng = np.random.default_rng(99)
    for v in (np.nan, np.inf, -np.inf):
        vals[rng.integers(0, vals.size, max(2, vals.size // 40))] = v
    if kind == "rectilinear":  # a regular grid cannot evaluate such a coordinate at all (next test)
        for d in range(n):
            for v in (np.nan, np.inf, -np.inf):
                obs[d][rng.integers(0, obs[d].size, 4)] = v
    for linearize in (True, False):
        want_out, want_grad, ok = cg.eval_grad(kind, _grid_args(kind, grids, np.dtype(dtype)), vals, obs, linearize=linearize,
                                               fma=True, dtype=np.dtype(dtype))
        assert ok.all() and np.isnan(want_grad).any()
        it = _handle(kind, grids, vals, linearize)
        try:
            out, grad = _device(it, obs)
            _assert_same(out, want_out, "device out")
            _assert_same(grad, want_grad, "device grad")
            _assert_same(out, it.eval_host(obs, np.zeros_like(obs[0])), "eval")
            hout, hgrad = it.eval_cubic_grad_host(obs)
            _assert_same(hout, want_out, "host out")
            _assert_same(hgrad, want_grad, "host grad")
        finally:
            it.close()


@pytest.mark.parametrize("n,chunk", [(1, 0), (2, 0), (3, 0), (3, 500), (4, 300)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e300])
def test_unrepresentable_coordinate_contract(n, chunk, bad, monkeypatch):
    """A coordinate whose cell index does not convert to isize on a regular grid.  Host: out[0..i) and grad[d][0..i) written,
    nothing at or beyond i — also when the call is cut into small chunks.  Device: i through finish()."""
    import torch

    if n in (2, 3):
        monkeypatch.setenv("INTERPN_HIP_BRICKS", "14")
        grids, vals, obs = _workload("regular", SHAPES[n][2], "float64", FILL[n])
        good_out, good_grad = _reference("regular", SHAPES[n][2], "float64", FILL[n], True, True)
    else:
        grids, vals, obs = _n_workload("regular", n, "float64")
        good_out, good_grad, _ = cg.eval_grad("regular", _grid_args("regular", grids, np.dtype("float64")), vals, obs)
    obs = [o.copy() for o in obs]
    npts = obs[0].size
    k = (2 * npts) // 3 + 1
    obs[n - 1][k] = bad
    obs[0][k + 40] = np.nan  # a later failure must not win
    _, _, ok = cg.eval_grad("regular", _grid_args("regular", grids, np.dtype("float64")), vals, obs)
    assert int(np.argmin(ok)) == k and not ok[k]
    it = _handle("regular", grids, vals, True)
    try:
        if chunk:
            it.set_option("host_chunk", chunk)
        out = np.full(npts, -7.0)
        grad = np.full((n, npts), -7.0)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
            it.eval_cubic_grad_host(obs, out, grad)
        _assert_same(out[:k], good_out[:k], "host out in front")
        _assert_same(grad[:, :k], good_grad[:, :k], "host grad in front")
        assert (out[k:] == -7.0).all() and (grad[:, k:] == -7.0).all()
        it.eval_cubic_grad_tensors([torch.from_numpy(o).cuda() for o in obs])
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
            it.finish()
        assert ei.value.first_bad_index == k
        # the word is clean again afterwards
        obs[n - 1][k] = 0.0
        obs[0][k + 40] = 0.0
        _device(it, obs)
    finally:
        it.close()


# ---- ABI: which handles, which arguments
def test_other_methods_are_unsupported_and_argument_checks():
    import interpn_amd
    from interpn_amd import _lib

    lib = _lib.load()
    grids, vals, obs = _workload("regular", (6, 6), "float64", FILL[2])
    rgrids = _workload("rectilinear", (6, 6), "float64", FILL[2])[0]
    dims, starts, steps = _grid_args("regular", grids, np.dtype("float64"))
    n = 64
    obs = [np.ascontiguousarray(o[:n]) for o in obs]
    out = np.zeros(n)
    grad = np.zeros((2, n))
    handles = [interpn_amd.Interpolator.regular("linear", dims, starts, steps, vals),
               interpn_amd.Interpolator.rectilinear("linear", list(rgrids), vals),
               interpn_amd.Interpolator.regular("nearest", dims, starts, steps, vals),
               interpn_amd.Interpolator.rectilinear("nearest", list(rgrids), vals),
               interpn_amd.Interpolator.grid1d_regular("Linear1D", 0.0, 0.5, vals[:9].copy()),
               interpn_amd.Interpolator.grid1d_rectilinear("Left1D", np.asarray(rgrids[0]), vals[:6].copy())]
    try:
        for it in handles:
            with pytest.raises(_lib.InterpnHipError, match="unsupported"):
                it.eval_cubic_grad_host(obs[:it.ndims()], out, grad[:it.ndims()])
            vp = (c_void_p * 2)(*[o.ctypes.data for o in obs])
            gp = (c_void_p * 2)(grad[0].ctypes.data, grad[1].ctypes.data)
            lens = (c_size_t * 2)(n, n)
            # before any device work: the (host) pointers are never dereferenced
            assert lib.interpn_hip_eval_cubic_grad_device(it._h, vp, it.ndims(), c_void_p(out.ctypes.data), gp, n, None) == UNSUPPORTED
            assert lib.interpn_hip_eval_cubic_grad_host(it._h, vp, lens, it.ndims(), c_void_p(out.ctypes.data), n, gp) == UNSUPPORTED
        assert not out.any() and not grad.any()
    finally:
        for it in handles:
            it.close()
    for cls in (interpn_amd.MultilinearRegular, interpn_amd.MultilinearRectilinear, interpn_amd.NearestRegular):
        assert not hasattr(cls, "eval_cubic_grad")
    it = _handle("regular", grids, vals)
    try:
        vp = (c_void_p * 3)(*[o.ctypes.data for o in obs], obs[0].ctypes.data)
        gp = (c_void_p * 3)(grad[0].ctypes.data, grad[1].ctypes.data, grad[1].ctypes.data)
        lens = (c_size_t * 3)(n, n, n)
        # a wrong number of coordinate arrays: the status `eval` gives on the same handle (the shared check of
        # interpn_hip_eval_host: on a multicubic handle of at most 4 dimensions the reference panics, beyond that it
        # reports "Dimension mismatch" like the multilinear namesakes)
        for nobs in (1, 3):
            want = lib.interpn_hip_eval_host(it._h, vp, lens, nobs, c_void_p(out.ctypes.data), n)
            assert want == REFERENCE_PANIC
            assert lib.interpn_hip_eval_cubic_grad_host(it._h, vp, lens, nobs, c_void_p(out.ctypes.data), n, gp) == want
            assert lib.interpn_hip_eval_cubic_grad_device(it._h, vp, nobs, c_void_p(out.ctypes.data), gp, n, None) == want
        with pytest.raises(_lib.ReferencePanic):
            it.eval_cubic_grad_host(obs[:1], out, grad[:1])
        g5, v5, o5 = _n_workload("regular", 5, "float64")
        it5 = _handle("regular", g5, v5)
        try:
            p5 = (c_void_p * 6)(*[o5[d % 5].ctypes.data for d in range(6)])
            l5 = (c_size_t * 6)(*[n] * 6)
            for nobs in (4, 6):
                assert lib.interpn_hip_eval_cubic_grad_host(it5._h, p5, l5, nobs, c_void_p(out.ctypes.data), n, p5) == DIM_MISMATCH
                assert lib.interpn_hip_eval_cubic_grad_device(it5._h, p5, nobs, c_void_p(out.ctypes.data), p5, n, None) == DIM_MISMATCH
            with pytest.raises(AssertionError, match="Dimension mismatch"):
                it5.eval_cubic_grad_host([o[:n] for o in o5[:4]], out, np.zeros((4, n)))
        finally:
            it5.close()
        short = (c_size_t * 2)(n, n - 1)
        assert lib.interpn_hip_eval_cubic_grad_host(it._h, vp, short, 2, c_void_p(out.ctypes.data), n, gp) == DIM_MISMATCH
        null1 = (c_void_p * 2)(grad[0].ctypes.data, None)
        for o, g_ in ((None, gp), (c_void_p(out.ctypes.data), None), (c_void_p(out.ctypes.data), null1)):
            assert lib.interpn_hip_eval_cubic_grad_host(it._h, vp, lens, 2, o, n, g_) == INVALID
            assert lib.interpn_hip_eval_cubic_grad_device(it._h, vp, 2, o, g_, n, None) == INVALID
        assert lib.interpn_hip_eval_cubic_grad_host(it._h, null1, lens, 2, c_void_p(out.ctypes.data), n, gp) == INVALID
        assert lib.interpn_hip_eval_cubic_grad_host(it._h, vp, None, 2, c_void_p(out.ctypes.data), n, gp) == INVALID
        # no points: nothing to do, whatever the other pointers are
        assert lib.interpn_hip_eval_cubic_grad_host(it._h, vp, (c_size_t * 2)(0, 0), 2, None, 0, None) == OK
        assert not out.any() and not grad.any()
        # and the multilinear pair keeps refusing a cubic handle
        assert lib.interpn_hip_eval_grad_host(it._h, vp, lens, 2, c_void_p(out.ctypes.data), n, gp) == UNSUPPORTED
    finally:
        it.close()


# ---- the device form: caller's arrays, a side stream, graph capture
@pytest.mark.parametrize("kind,n,layout", [("regular", 3, "11"), ("rectilinear", 3, "44"), ("rectilinear", 2, "11"), ("regular", 4, "")])
def test_callers_arrays_side_stream_and_graph_capture(kind, n, layout, monkeypatch):
    """Caller-supplied `out` / `grad` (views one element into their buffers), a non-default stream, and one capture-and-replay
    of a single call: one kernel node, no parallel branches, replayed once on new coordinates."""
    import torch

    if layout:
        monkeypatch.setenv("INTERPN_HIP_BRICKS", layout)
    if n == 4:
        grids, vals, obs = _n_workload(kind, n, "float64")
        want_out, want_grad, _ = cg.eval_grad(kind, _grid_args(kind, grids, np.dtype("float64")), vals, obs)
    else:
        grids, vals, obs = _workload(kind, SHAPES[n][3], "float64", FILL[n])
        want_out, want_grad = _reference(kind, SHAPES[n][3], "float64", FILL[n], True, True)
    npts = obs[0].size
    it = _handle(kind, grids, vals, True)
    try:
        obs_t = [torch.from_numpy(o).cuda() for o in obs]
        out_b = torch.full((npts + 1,), -7.0, dtype=torch.float64, device="cuda")
        grad_b = torch.full((n, npts + 2), -7.0, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        it.eval_cubic_grad_tensors(obs_t, out_b[1:], grad_b[:, 1:npts + 1], stream=side)
        it.finish()
        assert float(out_b[0]) == -7.0 and bool((grad_b[:, 0] == -7.0).all()) and bool((grad_b[:, -1] == -7.0).all())
        _assert_same(out_b[1:].cpu().numpy(), want_out, "side stream out")
        _assert_same(grad_b[:, 1:npts + 1].cpu().numpy(), want_grad, "side stream grad")
        # capture one call, replay it on the points in reverse order
        out = torch.zeros(npts, dtype=torch.float64, device="cuda")
        grad = torch.zeros((n, npts), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            it.eval_cubic_grad_tensors(obs_t, out, grad)
        for d in range(n):
            obs_t[d].copy_(torch.from_numpy(obs[d][::-1].copy()))
        out.zero_()
        grad.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        it.finish()
        _assert_same(out.cpu().numpy(), want_out[::-1], "replay out")
        _assert_same(grad.cpu().numpy(), want_grad[:, ::-1], "replay grad")
    finally:
        it.close()


# ---- the Python layer
def test_entry_points_interpn_grad_and_classes():
    import torch

    import interpn_amd

    for kind in ("regular", "rectilinear"):
        for dtype in ("float64", "float32"):
            shape3 = SHAPES[3][3]
            grids, vals, obs = _workload(kind, shape3, dtype, FILL[3])
            for linearize in (True, False):
                want_out, want_grad = _reference(kind, shape3, dtype, FILL[3], linearize, True)
                shape = (50, 40)
                obs2 = [o.reshape(shape) for o in obs]
                vals3 = vals.reshape(shape3)
                kw = dict(method="cubic", linearize_extrapolation=linearize, assume_regular=(kind == "regular"))
                out, grad = interpn_amd.interpn_grad(obs2, grids, vals3, **kw)
                assert out.shape == shape and grad.shape == (3,) + shape
                _assert_same(out.ravel(), want_out, "interpn_grad numpy")
                _assert_same(grad.reshape(3, -1), want_grad, "interpn_grad numpy")
                tout, tgrad = interpn_amd.interpn_grad([torch.from_numpy(o).cuda() for o in obs2], grids, vals3, **kw)
                assert tout.is_cuda and tuple(tout.shape) == shape and tuple(tgrad.shape) == (3,) + shape
                _assert_same(tout.cpu().numpy().ravel(), want_out, "interpn_grad tensors")
                _assert_same(tgrad.cpu().numpy().reshape(3, -1), want_grad, "interpn_grad tensors")
                if kind == "regular":
                    dims, starts, steps = _grid_args(kind, grids, np.dtype(dtype))
                    cls = interpn_amd.MulticubicRegular.new(dims, starts, steps, vals.copy(), linearize_extrapolation=linearize)
                else:
                    cls = interpn_amd.MulticubicRectilinear.new([np.array(g) for g in grids], vals.copy(), linearize_extrapolation=linearize)
                out, grad = cls.eval_cubic_grad(obs2)
                assert out.shape == shape and grad.shape == (3,) + shape
                _assert_same(out.ravel(), want_out, "class numpy")
                _assert_same(grad.reshape(3, -1), want_grad, "class numpy")
                tout, tgrad = cls.eval_cubic_grad([torch.from_numpy(o).cuda() for o in obs2])
                _assert_same(tout.cpu().numpy().ravel(), want_out, "class tensors")
                _assert_same(tgrad.cpu().numpy().reshape(3, -1), want_grad, "class tensors")
            # the default is today's: linear, and linearize_extrapolation has no effect on it
            lin_out, lin_grad = interpn_amd.interpn_grad(obs, grids, vals.reshape(shape3), assume_regular=(kind == "regular"))
            ref_out, ref_grad = interpn_amd.interpn_grad(obs, grids, vals.reshape(shape3), assume_regular=(kind == "regular"),
                                                         method="linear", linearize_extrapolation=False)
            _assert_same(lin_out, ref_out, "default method")
            _assert_same(lin_grad, ref_grad, "default method")
            with pytest.raises(ValueError, match="violate interpolator bounds"):
                interpn_amd.interpn_grad(obs, grids, vals.reshape(shape3), method="cubic", assume_regular=(kind == "regular"), check_bounds=True)


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_autograd_gradcheck_and_backward(kind, n):
    """The cubic is C1, and smooth strictly inside a cell: gradcheck at a quarter and three quarters of randomly chosen cells,
    far from every knot relative to its step (1e-6)."""
    import torch

    from interpn_amd import autograd

    shape = SHAPES[n][3] if n < 4 else N_SHAPES[4]
    rng = np.random.default_rng(17 + n)
    grids = [_axis(kind, shape[d], d, np.float64) for d in range(n)]
    vals = rng.uniform(-1.0, 1.0, int(np.prod(shape)))
    pts = []
    for d in range(n):
        g = grids[d]
        c = rng.integers(0, g.size - 1, 24)
        frac = np.where(rng.random(24) < 0.5, 0.25, 0.75)
        pts.append(g[c] + frac * (g[c + 1] - g[c]))
    it = _handle(kind, grids, vals, True)
    try:
        inputs = [torch.from_numpy(p).cuda().requires_grad_(True) for p in pts]
        assert torch.autograd.gradcheck(lambda *o: autograd.interp(it, o), inputs, eps=1e-6, atol=1e-6, rtol=1e-5)
        out, grad = it.eval_cubic_grad_tensors([t.detach() for t in inputs])
        it.finish()
        y = autograd.interp(it, inputs)
        assert bool((y.detach() == out).all())
        y.sum().backward()
        for d in range(n):
            assert bool((inputs[d].grad == grad[d]).all()), d
            inputs[d].grad = None
        w = torch.from_numpy(rng.uniform(-2, 2, 24)).cuda()
        (autograd.interp(it, inputs) * w).sum().backward()
        for d in range(n):
            assert bool((inputs[d].grad == w * grad[d]).all()), d
        a = inputs[0].detach().reshape(4, 6).requires_grad_(True)
        rest = [t.detach().reshape(4, 6) for t in inputs[1:]]
        y2 = autograd.interp(it, [a] + rest)
        assert tuple(y2.shape) == (4, 6)
        y2.sum().backward()
        assert bool((a.grad.reshape(-1) == grad[0]).all())
    finally:
        it.close()
