"""Multilinear value and gradient on the GPU (interpn_hip_eval_grad_*, Interpolator.eval_grad_*, interpn_grad, the classes'
eval_grad, interpn_amd.autograd) against the numpy restatement of the definition (tests/grad_restatement.py, pinned on the CPU
by tests/test_grad_cpu.py).  Every comparison is bit for bit at the same fma flavour; a NaN need only be a NaN on both sides."""

from ctypes import c_size_t, c_void_p

import numpy as np
import pytest

from tests import grad_restatement as gr
from tests.helpers import synthetic_case

pytestmark = pytest.mark.gpu

OK, DIM_MISMATCH, INVALID, UNSUPPORTED = 0, 1, 32, 33
FUSED, GENERIC = "interpn::k_linear_grad<", "interpn::k_linear_grad_n<"

# points per axis: N = 2, 3 beyond the 16 KiB below which a handle keeps no re-laid table; N = 7, 8 on 3-point axes
AXES = {1: [300], 2: [70, 90], 3: [20, 18, 22], 4: [7, 6, 8, 5], 5: [5, 4, 6, 3, 4], 6: [3, 4, 3, 5, 2, 4], 7: [3] * 7, 8: [3] * 8}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_BRICKS", "INTERPN_HIP_FORCE_GENERIC", "INTERPN_HIP_AXIS_REGS", "INTERPN_HIP_PPL"):
        monkeypatch.delenv(name, raising=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist(), got[~same][:4], want[~same][:4])


def _handle(case, fma=True):
    import interpn_amd

    dt = case.vals.dtype
    if case.kind == "regular":
        return interpn_amd.Interpolator.regular("linear", case.dims, case.starts, case.steps, case.vals, dtype=dt, fma=fma)
    return interpn_amd.Interpolator.rectilinear("linear", case.grids, case.vals, dtype=dt, fma=fma)


def _device(it, obs, out=None, grad=None, stream=None):
    import torch

    out_t, grad_t = it.eval_grad_tensors([torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in obs], out, grad, stream)
    it.finish()
    return out_t.cpu().numpy(), grad_t.cpu().numpy()


def _case(kind, n, dtype, nobs=1500, seed=0, axes=None):
    return synthetic_case("linear", kind, n, axes or AXES[n], nobs, 8800 + 17 * n + seed + (kind == "regular"), dtype=dtype,
                          specials=True)


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_device_and_host_match_the_restatement(kind, n, dtype, fma):
    case = _case(kind, n, dtype, nobs=1500 if n <= 6 else 400)
    want_out, want_grad, ok = gr.eval_grad_case(case, fma=fma)
    assert ok.all()
    it = _handle(case, fma)
    try:
        out, grad = _device(it, case.obs)
        name = it.kernel_name()
        assert name.startswith(FUSED if n in (2, 3) else GENERIC), name
        _assert_same(out, want_out, "device out")
        _assert_same(grad, want_grad, "device grad")
        plain = it.eval_host(case.obs, np.zeros_like(case.obs[0]))
        _assert_same(out, plain, "value against eval")
        hout, hgrad = it.eval_grad_host(case.obs)
        _assert_same(hout, want_out, "host out")
        _assert_same(hgrad, want_grad, "host grad")
    finally:
        it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_runtime_n_kernel_gives_the_fused_kernels_bits(kind, n, dtype, monkeypatch):
    case = _case(kind, n, dtype, seed=3)
    want_out, want_grad, _ = gr.eval_grad_case(case, fma=True)
    it = _handle(case)
    try:
        out, grad = _device(it, case.obs)
        assert it.kernel_name().startswith(FUSED)
        it.set_option("force_generic", 1)
        gout, ggrad = _device(it, case.obs)
        assert it.kernel_name().startswith(GENERIC), it.kernel_name()
        for a, b, c in ((out, gout, want_out), (grad, ggrad, want_grad)):
            _assert_same(a, c, "fused")
            _assert_same(b, c, "force_generic")
    finally:
        it.close()
    monkeypatch.setenv("INTERPN_HIP_BRICKS", "off")
    it = _handle(case)
    try:
        assert it.table_layout()[0] == 0
        oout, ograd = _device(it, case.obs)
        assert it.kernel_name().startswith(GENERIC), it.kernel_name()
        _assert_same(oout, want_out, "bricks off")
        _assert_same(ograd, want_grad, "bricks off")
    finally:
        it.close()


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("layout,dtype", [("11", np.float64), ("12", np.float64), ("22", np.float64), ("11", np.float32),
                                          ("12", np.float32), ("22", np.float32), ("j4", np.float32)])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_3d_under_every_brick_layout(kind, layout, dtype, fma, monkeypatch):
    """N = 3 gathers from whichever table the handle has: steps (1,1), (1,2), (2,2) and the f32 2 x 4 x 4 bricks; with two
    points per lane and with one (option ppl = 1)."""
    monkeypatch.setenv("INTERPN_HIP_BRICKS", layout)
    case = _case(kind, 3, dtype, seed=11, axes=[21, 19, 23])
    want_out, want_grad, _ = gr.eval_grad_case(case, fma=fma)
    it = _handle(case, fma)
    try:
        for ppl in (0, 1):
            it.set_option("ppl", ppl)
            out, grad = _device(it, case.obs)
            name = it.kernel_name()
            assert name.startswith(FUSED), name
            args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]  # T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL
            assert args[1] == "3" and args[2] == ("true" if kind == "rectilinear" else "false") and args[3] == ("true" if fma else "false")
            if layout == "j4":
                assert args[4:6] == ["1", "1"] and args[8] == "2", name
            else:
                assert args[4:6] == [layout[0], layout[1]] and args[8] == "0", name
            assert args[6] == ("1" if ppl == 1 else "2"), name
            _assert_same(out, want_out, (layout, ppl, "out"))
            _assert_same(grad, want_grad, (layout, ppl, "grad"))
    finally:
        it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,axes", [(2, [40, 33]), (2, [300, 41]), (3, [20, 18, 22]), (3, [70, 12, 66])])
def test_rectilinear_axis_search_forms(n, axes, dtype, monkeypatch):
    """The fused kernel searches rectilinear axes like the value kernels: across lanes (axes of at most 64 coordinates:
    the lane table, the probe sequence) or in LDS / through L2 (option axis_regs = 0, longer axes, axis_lds_kb = 0)."""
    if n == 2:
        monkeypatch.setenv("INTERPN_HIP_BRICKS", "on")  # a 2-D grid of 64 x 64 f32 values at most is L1-sized: no table by itself
    case = _case("rectilinear", n, dtype, seed=23, axes=axes)
    want_out, want_grad, _ = gr.eval_grad_case(case, fma=True)
    it = _handle(case)
    seen = set()
    try:
        assert it.table_layout()[0] > 0
        for regs, lds_kb in ((-1, -1), (1, -1), (0, -1), (0, 0)):
            it.set_option("axis_regs", regs)
            it.set_option("axis_lds_kb", lds_kb)
            out, grad = _device(it, case.obs)
            name = it.kernel_name()
            assert name.startswith(FUSED), name
            seen.add(name)
            _assert_same(out, want_out, (regs, lds_kb, "out"))
            _assert_same(grad, want_grad, (regs, lds_kb, "grad"))
    finally:
        it.close()
    if max(axes) <= 64:
        assert len(seen) >= 2, seen  # lanes and LDS forms both ran


def test_entry_points_interpn_grad_and_classes():
    import torch

    import interpn_amd

    for kind in ("regular", "rectilinear"):
        for dtype in (np.float64, np.float32):
            case = _case(kind, 3, dtype, nobs=2000, seed=31)
            want_out, want_grad, _ = gr.eval_grad_case(case, fma=True)
            shape = (50, 40)
            obs2 = [o.reshape(shape) for o in case.obs]
            vals3 = case.vals.reshape(case.dims)
            # interpn_grad on numpy arrays and on CUDA tensors
            out, grad = interpn_amd.interpn_grad(obs2, case.grids, vals3, assume_regular=(kind == "regular"))
            assert out.shape == shape and grad.shape == (3,) + shape
            _assert_same(out.ravel(), want_out, "interpn_grad numpy")
            _assert_same(grad.reshape(3, -1), want_grad, "interpn_grad numpy")
            tout, tgrad = interpn_amd.interpn_grad([torch.from_numpy(o).cuda() for o in obs2], case.grids, vals3,
                                                   assume_regular=(kind == "regular"))
            assert tout.is_cuda and tuple(tout.shape) == shape and tuple(tgrad.shape) == (3,) + shape
            _assert_same(tout.cpu().numpy().ravel(), want_out, "interpn_grad tensors")
            _assert_same(tgrad.cpu().numpy().reshape(3, -1), want_grad, "interpn_grad tensors")
            with pytest.raises(ValueError, match="violate interpolator bounds"):
                interpn_amd.interpn_grad(obs2, case.grids, vals3, assume_regular=(kind == "regular"), check_bounds=True)
            # the classes
            if kind == "regular":
                cls = interpn_amd.MultilinearRegular.new(case.dims, case.starts, case.steps, case.vals)
            else:
                cls = interpn_amd.MultilinearRectilinear.new(case.grids, case.vals)
            out, grad = cls.eval_grad(obs2)
            assert out.shape == shape and grad.shape == (3,) + shape
            _assert_same(out.ravel(), want_out, "class numpy")
            _assert_same(grad.reshape(3, -1), want_grad, "class numpy")
            tout, tgrad = cls.eval_grad([torch.from_numpy(o).cuda() for o in obs2])
            _assert_same(tout.cpu().numpy().ravel(), want_out, "class tensors")
            _assert_same(tgrad.cpu().numpy().reshape(3, -1), want_grad, "class tensors")


@pytest.mark.parametrize("kind,n,dtype", [("regular", 3, np.float64), ("rectilinear", 3, np.float32), ("regular", 2, np.float32),
                                          ("rectilinear", 2, np.float64), ("regular", 4, np.float64), ("rectilinear", 1, np.float32)])
def test_batch_shapes_offset_views_and_host_chunks(kind, n, dtype):
    import torch

    big = 100_003
    case = _case(kind, n, dtype, nobs=big + 1, seed=41)
    want_out, want_grad, _ = gr.eval_grad_case(case, fma=True)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    it = _handle(case)
    try:
        for count in (0, 1, 255, 257, big):
            obs = [np.ascontiguousarray(o[:count]) for o in case.obs]
            out, grad = _device(it, obs)
            assert out.shape == (count,) and grad.shape == (n, count)
            _assert_same(out, want_out[:count], ("device", count))
            _assert_same(grad, want_grad[:, :count], ("device", count))
            hout, hgrad = it.eval_grad_host(obs)
            _assert_same(hout, want_out[:count], ("host", count))
            _assert_same(hgrad, want_grad[:, :count], ("host", count))
        # views one element into their buffers: coordinates, out and grad rows lose the 2-element alignment
        for count in (257, big):
            obs_t = [torch.from_numpy(case.obs[d]).cuda()[1:count + 1] for d in range(n)]
            out_b = torch.full((count + 1,), -7.0, dtype=tdt, device="cuda")
            grad_b = torch.full((n, count + 2), -7.0, dtype=tdt, device="cuda")
            it.eval_grad_tensors(obs_t, out_b[1:], grad_b[:, 1:count + 1])
            it.finish()
            assert float(out_b[0]) == -7.0 and bool((grad_b[:, 0] == -7.0).all()) and bool((grad_b[:, -1] == -7.0).all())
            _assert_same(out_b[1:].cpu().numpy(), want_out[1:count + 1], ("offset", count))
            _assert_same(grad_b[:, 1:count + 1].cpu().numpy(), want_grad[:, 1:count + 1], ("offset", count))
            hout_b = np.full(count + 1, -7.0, dtype=dtype)
            hgrad_b = np.full((n, count + 2), -7.0, dtype=dtype)
            it.eval_grad_host([case.obs[d][1:count + 1] for d in range(n)], hout_b[1:], hgrad_b[:, 1:count + 1])
            assert hout_b[0] == -7.0 and (hgrad_b[:, 0] == -7.0).all() and (hgrad_b[:, -1] == -7.0).all()
            _assert_same(hout_b[1:], want_out[1:count + 1], ("host offset", count))
            _assert_same(hgrad_b[:, 1:count + 1], want_grad[:, 1:count + 1], ("host offset", count))
        # a host batch of several chunks
        it.set_option("host_chunk", 30_000)
        obs = [np.ascontiguousarray(o[:big]) for o in case.obs]
        hout, hgrad = it.eval_grad_host(obs)
        _assert_same(hout, want_out[:big], "chunked host")
        _assert_same(hgrad, want_grad[:, :big], "chunked host")
    finally:
        it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_non_finite_inputs_propagate(kind, n, dtype):
    case = _case(kind, n, dtype, nobs=600, seed=53)
    rng = np.random.default_rng(99)
    # NaN / +-inf in the table
    for v in (np.nan, np.inf, -np.inf):
        case.vals[rng.integers(0, case.vals.size, max(3, case.vals.size // 50))] = v
    if kind == "rectilinear":  # a regular grid cannot evaluate such a coordinate at all (next test)
        for d in range(n):
            for v in (np.nan, np.inf, -np.inf):
                case.obs[d][rng.integers(100, 600, 4)] = v
    want_out, want_grad, ok = gr.eval_grad_case(case, fma=True)
    assert ok.all()
    assert np.isnan(want_grad).any()
    it = _handle(case)
    try:
        out, grad = _device(it, case.obs)
        _assert_same(out, want_out, "device")
        _assert_same(grad, want_grad, "device")
        _assert_same(out, it.eval_host(case.obs, np.zeros_like(case.obs[0])), "eval")
        hout, hgrad = it.eval_grad_host(case.obs)
        _assert_same(hout, want_out, "host")
        _assert_same(hgrad, want_grad, "host")
    finally:
        it.close()


@pytest.mark.parametrize("n,chunk", [(1, 0), (2, 0), (3, 0), (3, 1000), (5, 700)])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e300])
def test_unrepresentable_coordinate_contract(n, chunk, bad):
    """The inputs the parity tests use for `eval`: a coordinate whose cell index does not convert to isize on a regular grid.
    Host: out[0..i) and grad[d][0..i) written, nothing at or beyond i.  Device: i through finish()."""
    import torch

    case = _case("regular", n, np.float64, nobs=4000, seed=61)
    k = 2517
    good_out, good_grad, _ = gr.eval_grad_case(case, fma=True)
    case.obs[n - 1][k] = bad
    case.obs[0][k + 300] = np.nan  # a later failure must not win
    _, _, ok = gr.eval_grad_case(case, fma=True)
    assert int(np.argmin(ok)) == k and not ok[k]
    it = _handle(case)
    try:
        if chunk:
            it.set_option("host_chunk", chunk)
        out = np.full(4000, -7.0)
        grad = np.full((n, 4000), -7.0)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
            it.eval_grad_host(case.obs, out, grad)
        _assert_same(out[:k], good_out[:k], "host out in front")
        _assert_same(grad[:, :k], good_grad[:, :k], "host grad in front")
        assert (out[k:] == -7.0).all() and (grad[:, k:] == -7.0).all()
        it.eval_grad_tensors([torch.from_numpy(o).cuda() for o in case.obs])
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
            it.finish()
        assert ei.value.first_bad_index == k
        # the word is clean again afterwards
        case.obs[n - 1][k] = 0.0
        case.obs[0][k + 300] = 0.0
        _device(it, case.obs)
    finally:
        it.close()


def test_other_methods_are_unsupported_and_argument_checks():
    import interpn_amd
    from interpn_amd import _lib

    lib = _lib.load()
    case = _case("regular", 2, np.float64, nobs=64, seed=71, axes=[9, 8])
    n = 64
    out = np.zeros(n)
    grad = np.zeros((2, n))
    handles = [interpn_amd.Interpolator.regular("cubic", case.dims, case.starts, case.steps, case.vals),
               interpn_amd.Interpolator.rectilinear("cubic", case.grids, case.vals),
               interpn_amd.Interpolator.regular("nearest", case.dims, case.starts, case.steps, case.vals),
               interpn_amd.Interpolator.rectilinear("nearest", case.grids, case.vals),
               interpn_amd.Interpolator.grid1d_regular("Linear1D", 0.0, 0.5, case.vals[:9].copy()),
               interpn_amd.Interpolator.grid1d_rectilinear("Left1D", case.grids[0], case.vals[:9].copy())]
    try:
        for it in handles:
            obs = case.obs[:it.ndims()]
            with pytest.raises(_lib.InterpnHipError, match="unsupported"):
                it.eval_grad_host(obs, out, grad[:it.ndims()])
            vp = (c_void_p * 2)(*[o.ctypes.data for o in case.obs])
            gp = (c_void_p * 2)(grad[0].ctypes.data, grad[1].ctypes.data)
            lens = (c_size_t * 2)(n, n)
            # before any device work: the (host) pointers are never dereferenced
            assert lib.interpn_hip_eval_grad_device(it._h, vp, it.ndims(), c_void_p(out.ctypes.data), gp, n, None) == UNSUPPORTED
            assert lib.interpn_hip_eval_grad_host(it._h, vp, lens, it.ndims(), c_void_p(out.ctypes.data), n, gp) == UNSUPPORTED
        assert not out.any() and not grad.any()
    finally:
        for it in handles:
            it.close()
    for cls, args in ((interpn_amd.MulticubicRegular, (case.dims, case.starts, case.steps, case.vals)),
                      (interpn_amd.MulticubicRectilinear, (case.grids, case.vals)),
                      (interpn_amd.NearestRegular, (case.dims, case.starts, case.steps, case.vals)),
                      (interpn_amd.NearestRectilinear, (case.grids, case.vals))):
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            cls.new(*args).eval_grad(case.obs)
    it = _handle(case)
    try:
        vp = (c_void_p * 3)(*[o.ctypes.data for o in case.obs], case.obs[0].ctypes.data)
        gp = (c_void_p * 3)(grad[0].ctypes.data, grad[1].ctypes.data, grad[1].ctypes.data)
        lens = (c_size_t * 3)(n, n, n)
        for nobs in (1, 3):
            assert lib.interpn_hip_eval_grad_host(it._h, vp, lens, nobs, c_void_p(out.ctypes.data), n, gp) == DIM_MISMATCH
            assert lib.interpn_hip_eval_grad_device(it._h, vp, nobs, c_void_p(out.ctypes.data), gp, n, None) == DIM_MISMATCH
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            it.eval_grad_host(case.obs[:1], out, grad[:1])
        short = (c_size_t * 2)(n, n - 1)
        assert lib.interpn_hip_eval_grad_host(it._h, vp, short, 2, c_void_p(out.ctypes.data), n, gp) == DIM_MISMATCH
        null1 = (c_void_p * 2)(grad[0].ctypes.data, None)
        for o, g_ in ((None, gp), (c_void_p(out.ctypes.data), None), (c_void_p(out.ctypes.data), null1)):
            assert lib.interpn_hip_eval_grad_host(it._h, vp, lens, 2, o, n, g_) == INVALID
            assert lib.interpn_hip_eval_grad_device(it._h, vp, 2, o, g_, n, None) == INVALID
        assert lib.interpn_hip_eval_grad_host(it._h, null1, lens, 2, c_void_p(out.ctypes.data), n, gp) == INVALID
        assert lib.interpn_hip_eval_grad_host(it._h, vp, None, 2, c_void_p(out.ctypes.data), n, gp) == INVALID
        # no points: nothing to do, whatever the other pointers are
        assert lib.interpn_hip_eval_grad_host(it._h, vp, (c_size_t * 2)(0, 0), 2, None, 0, None) == OK
        assert not out.any() and not grad.any()
    finally:
        it.close()


@pytest.mark.parametrize("kind,n", [("regular", 3), ("rectilinear", 2), ("regular", 5)])
def test_graph_capture_of_one_kernel(kind, n):
    """The device form is one kernel: captured on a side stream (a single node, no parallel branches) and replayed once on
    new coordinates."""
    import torch

    case = _case(kind, n, np.float64, nobs=5000, seed=83)
    fresh = _case(kind, n, np.float64, nobs=5000, seed=84)
    it = _handle(case)
    try:
        obs_t = [torch.from_numpy(o).cuda() for o in case.obs]
        out = torch.zeros(5000, dtype=torch.float64, device="cuda")
        grad = torch.zeros((n, 5000), dtype=torch.float64, device="cuda")
        it.eval_grad_tensors(obs_t, out, grad)  # warm: nothing is left to allocate or build
        it.finish()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            it.eval_grad_tensors(obs_t, out, grad)
        for d in range(n):
            obs_t[d].copy_(torch.from_numpy(fresh.obs[d]))
        out.zero_()
        grad.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        it.finish()
        want_out, want_grad, _ = gr.eval_grad(kind, (case.dims, case.starts, case.steps) if kind == "regular" else case.grids,
                                              case.vals, fresh.obs, fma=True)
        _assert_same(out.cpu().numpy(), want_out, "replay out")
        _assert_same(grad.cpu().numpy(), want_grad, "replay grad")
    finally:
        it.close()


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_autograd_gradcheck_and_backward(kind, n):
    import torch

    from interpn_amd import autograd

    case = _case(kind, n, np.float64, nobs=64, seed=91)
    rng = np.random.default_rng(17)
    # a quarter and three quarters of randomly chosen cells: far from every knot relative to gradcheck's step (1e-6)
    pts = []
    for d in range(n):
        g = case.grids[d]
        c = rng.integers(0, g.size - 1, 24)
        frac = np.where(rng.random(24) < 0.5, 0.25, 0.75)
        pts.append(g[c] + frac * (g[c + 1] - g[c]))
    it = _handle(case)
    try:
        inputs = [torch.from_numpy(p).cuda().requires_grad_(True) for p in pts]
        assert torch.autograd.gradcheck(lambda *o: autograd.interp(it, o), inputs, eps=1e-6, atol=1e-6, rtol=1e-5)
        # backward through a sum reproduces grad exactly; a weighted sum scales it
        out, grad = it.eval_grad_tensors([t.detach() for t in inputs])
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
        # only the coordinates that ask for it get a gradient; shapes other than 1-D keep their shape
        a = inputs[0].detach().reshape(4, 6).requires_grad_(True)
        rest = [t.detach().reshape(4, 6) for t in inputs[1:]]
        y2 = autograd.interp(it, [a] + rest)
        assert tuple(y2.shape) == (4, 6)
        y2.sum().backward()
        assert bool((a.grad.reshape(-1) == grad[0]).all())
    finally:
        it.close()
