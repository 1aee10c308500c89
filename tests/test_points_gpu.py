"""Point-major observation points on the GPU (interpn_hip_eval_points_*, Interpolator.eval_points_*, interpn_points, the
classes' eval_points): the points as ONE array of shape (n, N).  The yardstick is `eval_tensors` of the same handle on the
de-interleaved columns (the existing kernels, themselves pinned to the oracle by tests/test_gpu_parity.py); one case per
method and kind is compared with the oracle as well.  Every comparison is bit for bit, a NaN need only be a NaN on both
sides."""

from ctypes import c_int, c_void_p

import numpy as np
import pytest

from tests.helpers import run_oracle, synthetic_case
from tests.test_grad_gpu import AXES

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, 32, 33
FUSED = "interpn::k_linear_points<"
NPTS = 1501  # odd: the two-points-per-lane form has a tail; 3 workgroups, 11 full waves and a ragged one

# multicubic needs four points per axis: the gradient tests' shapes where they have them, 4 per axis beyond
CUBIC_AXES = {**AXES, 5: [5, 4, 6, 4, 4], 6: [4] * 6, 7: [4] * 7, 8: [4] * 8}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_BRICKS", "INTERPN_HIP_FORCE_GENERIC", "INTERPN_HIP_AXIS_REGS", "INTERPN_HIP_PPL",
                 "INTERPN_HIP_POINTS_PATH", "INTERPN_HIP_POINTS_LOAD", "INTERPN_HIP_POINTS_SLICE"):
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
        return interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, case.vals, dtype=dt, fma=fma)
    return interpn_amd.Interpolator.rectilinear(case.method, case.grids, case.vals, dtype=dt, fma=fma)


def _case(method, kind, n, dtype, nobs=NPTS, seed=0, axes=None):
    axes = axes or (CUBIC_AXES if method == "cubic" else AXES)[n]
    return synthetic_case(method, kind, n, axes, nobs, 9900 + 17 * n + seed + (kind == "regular"), dtype=dtype, specials=True)


def _columns(it, obs):
    """The yardstick: the handle's ordinary evaluation of the coordinate arrays."""
    import torch

    out = it.eval_tensors([torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in obs])
    it.finish()
    return out.cpu().numpy()


def _rows(obs):
    return np.ascontiguousarray(np.stack(obs, axis=1))


def _device(it, pts_t, out=None, **kw):
    out = it.eval_points_tensors(pts_t, out, **kw)
    it.finish()
    return out.cpu().numpy()


def _expected_path(method, n):
    return "fused" if method == "linear" and n in (2, 3) else ("direct" if n == 1 else "split")


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("method,n", [(m, n) for m in ("linear", "cubic", "nearest") for n in range(1, 9) if m != "nearest" or n <= 6])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_device_and_host_match_the_columns(oracle, kind, method, n, dtype, fma):
    import torch

    case = _case(method, kind, n, dtype)
    it = _handle(case, fma)
    try:
        want = _columns(it, case.obs)
        if n == 3 and dtype == np.float64 and fma:  # one case per method and kind: the yardstick itself against the oracle
            _assert_same(want, run_oracle(oracle, case, fma=True), "columns against the oracle")
        pts = _rows(case.obs)
        got = _device(it, torch.from_numpy(pts).cuda())
        name = it.kernel_name()
        assert name.startswith(FUSED) == (method == "linear" and n in (2, 3)), name
        assert it.last_points_path() == _expected_path(method, n)
        _assert_same(got, want, "device")
        _assert_same(it.eval_points_host(pts), want, "host")
    finally:
        it.close()


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("layout,dtype", [("11", np.float64), ("12", np.float64), ("22", np.float64), ("11", np.float32),
                                          ("12", np.float32), ("22", np.float32), ("j4", np.float32)])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_3d_under_every_brick_layout(kind, layout, dtype, fma, monkeypatch):
    import torch

    monkeypatch.setenv("INTERPN_HIP_BRICKS", layout)
    case = _case("linear", kind, 3, dtype, seed=11, axes=[21, 19, 23])
    it = _handle(case, fma)
    try:
        want = _columns(it, case.obs)
        pts_t = torch.from_numpy(_rows(case.obs)).cuda()
        for ppl in (0, 1):
            it.set_option("ppl", ppl)
            got = _device(it, pts_t)
            name = it.kernel_name()
            assert name.startswith(FUSED), name
            args = [a.strip() for a in name[name.index("<") + 1:-1].split(",")]  # T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL
            assert args[1] == "3" and args[2] == ("true" if kind == "rectilinear" else "false") and args[3] == ("true" if fma else "false")
            if layout == "j4":
                assert args[4:6] == ["1", "1"] and args[8] == "2", name
            else:
                assert args[4:6] == [layout[0], layout[1]] and args[8] == "0", name
            assert args[6] == ("1" if ppl == 1 else "2"), name
            _assert_same(got, want, (layout, ppl))
    finally:
        it.close()


@pytest.mark.parametrize("kind,n,dtype", [("regular", 3, np.float64), ("rectilinear", 3, np.float32), ("regular", 2, np.float32),
                                          ("rectilinear", 2, np.float64)])
def test_one_point_per_lane_from_the_environment(kind, n, dtype, monkeypatch):
    import torch

    monkeypatch.setenv("INTERPN_HIP_PPL", "1")
    case = _case("linear", kind, n, dtype, seed=13)
    it = _handle(case)
    try:
        want = _columns(it, case.obs)
        got = _device(it, torch.from_numpy(_rows(case.obs)).cuda())
        name = it.kernel_name()
        assert name.startswith(FUSED) and name.split(",")[6].strip() == "1", name
        _assert_same(got, want, "ppl = 1")
    finally:
        it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,axes", [(2, [40, 33]), (2, [300, 41]), (3, [20, 18, 22]), (3, [70, 12, 66])])
def test_rectilinear_axis_search_forms(n, axes, dtype, monkeypatch):
    """The axis searches of the value kernels: across lanes (lane table, probe sequence), in LDS, through L2."""
    import torch

    if n == 2:
        monkeypatch.setenv("INTERPN_HIP_BRICKS", "on")  # a 2-D grid of 64 x 64 f32 values at most is L1-sized: no table by itself
    case = _case("linear", "rectilinear", n, dtype, seed=23, axes=axes)
    it = _handle(case)
    seen = set()
    try:
        assert it.table_layout()[0] > 0
        want = _columns(it, case.obs)
        pts_t = torch.from_numpy(_rows(case.obs)).cuda()
        for regs, lds_kb in ((-1, -1), (1, -1), (0, -1), (0, 0)):
            it.set_option("axis_regs", regs)
            it.set_option("axis_lds_kb", lds_kb)
            got = _device(it, pts_t)
            name = it.kernel_name()
            assert name.startswith(FUSED), name
            seen.add(name)
            _assert_same(got, want, (regs, lds_kb))
    finally:
        it.close()
    if max(axes) <= 64:
        assert len(seen) >= 2, seen  # lanes and LDS forms both ran


@pytest.mark.parametrize("kind,n,dtype", [("regular", 3, np.float64), ("rectilinear", 3, np.float64), ("regular", 3, np.float32),
                                          ("regular", 2, np.float64), ("rectilinear", 2, np.float32)])
def test_load_forms_strides_and_alignment(kind, n, dtype):
    """Packed rows, rows of a wider tensor (stride N + 1, N + 5), a base and an `out` one element off a 16-byte boundary, and
    the counts around a wave; every coordinate load form the kernel has (option points_load: 1 per-lane vectors, 2 the
    wave's span through LDS, 3 elements).  Untouched neighbours stay untouched."""
    import torch

    case = _case("linear", kind, n, dtype, seed=37)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    it = _handle(case)
    try:
        want = _columns(it, case.obs)
        pts = _rows(case.obs)
        for load in (0, 1, 2, 3):
            it.set_option("points_load", load)
            for count in (1, 63, 64, 65, NPTS):
                sub = np.ascontiguousarray(pts[:count])
                views = {"packed": torch.from_numpy(sub).cuda()}
                for extra in (1, 5):
                    wide = torch.full((count, n + extra), 1e30, dtype=tdt, device="cuda")  # a coordinate nobody may read
                    wide[:, :n] = views["packed"]
                    views[f"stride {n + extra}"] = wide[:, :n]
                big = torch.zeros(count * n + 3, dtype=tdt, device="cuda")
                big[1:1 + count * n] = views["packed"].reshape(-1)
                views["base + 1"] = big[1:1 + count * n].view(count, n)
                for what, v in views.items():
                    assert v.stride(1) == 1 or count * n == 1
                    _assert_same(_device(it, v), want[:count], (load, count, what))
                    assert it.kernel_name().startswith(FUSED) and it.last_points_path() == "fused"
                out_b = torch.full((count + 2,), -7.0, dtype=tdt, device="cuda")
                got = _device(it, views["packed"], out_b[1:count + 1])
                _assert_same(got, want[:count], (load, count, "out + 1"))
                assert float(out_b[0]) == -7.0 and float(out_b[-1]) == -7.0
                # the host form takes the row stride of a numpy view
                hwide = np.full((count, n + 1), 1e30, dtype=dtype)
                hwide[:, :n] = sub
                _assert_same(it.eval_points_host(hwide[:, :n]), want[:count], (load, count, "host stride"))
    finally:
        it.close()


@pytest.mark.parametrize("kind,method,n,dtype", [("regular", "cubic", 3, np.float64), ("rectilinear", "nearest", 2, np.float32),
                                                 ("regular", "linear", 5, np.float64), ("rectilinear", "linear", 1, np.float32)])
def test_split_path_strides_and_alignment(kind, method, n, dtype):
    import torch

    case = _case(method, kind, n, dtype, seed=39)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    it = _handle(case)
    try:
        want = _columns(it, case.obs)
        pts = _rows(case.obs)
        for count in (1, 255, 256, 257, NPTS):
            packed = torch.from_numpy(np.ascontiguousarray(pts[:count])).cuda()
            for extra in (1, 5, 40):  # 40: rows longer than the de-interleaving tile takes
                wide = torch.full((count, n + extra), 1e30, dtype=tdt, device="cuda")
                wide[:, :n] = packed
                # the last row's trailing elements are not part of the view's storage span: they must not be read
                _assert_same(_device(it, wide[:, :n]), want[:count], (count, extra))
                assert it.last_points_path() == ("direct" if n == 1 and count == 1 else "split")  # one point has no stride
            big = torch.zeros(count * n + 3, dtype=tdt, device="cuda")
            big[1:1 + count * n] = packed.reshape(-1)
            out_b = torch.full((count + 2,), -7.0, dtype=tdt, device="cuda")
            got = _device(it, big[1:1 + count * n].view(count, n), out_b[1:count + 1])
            _assert_same(got, want[:count], (count, "base + 1, out + 1"))
            assert float(out_b[0]) == -7.0 and float(out_b[-1]) == -7.0
            assert it.last_points_path() == ("direct" if n == 1 else "split")
    finally:
        it.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_fused_against_split_on_one_handle(kind, n, dtype, monkeypatch):
    import torch

    import interpn_amd

    case = _case("linear", kind, n, dtype, seed=43)
    pts_t = torch.from_numpy(_rows(case.obs)).cuda()
    it = _handle(case)
    try:
        want = _columns(it, case.obs)
        it.set_option("points_path", 1)
        fused = _device(it, pts_t)
        assert it.kernel_name().startswith(FUSED) and it.last_points_path() == "fused"
        it.set_option("points_path", 2)
        split = _device(it, pts_t)
        assert not it.kernel_name().startswith(FUSED) and it.last_points_path() == "split"
        _assert_same(fused, want, "fused")
        _assert_same(split, want, "split")
        it.set_option("points_path", 0)
        it.set_option("force_generic", 1)
        _assert_same(_device(it, pts_t), want, "force_generic")
        assert it.last_points_path() == "split" and not it.kernel_name().startswith(FUSED)
    finally:
        it.close()
    monkeypatch.setenv("INTERPN_HIP_BRICKS", "off")
    it = _handle(case)
    try:
        assert it.table_layout()[0] == 0
        _assert_same(_device(it, pts_t), want, "bricks off")
        assert it.last_points_path() == "split"
        it.set_option("points_path", 1)
        with pytest.raises(interpn_amd._lib.InterpnHipError, match="unsupported"):
            it.eval_points_tensors(pts_t)
    finally:
        it.close()


def test_fused_only_is_unsupported_where_no_fused_kernel_exists():
    import torch

    import interpn_amd

    for method, n in (("cubic", 3), ("nearest", 2), ("linear", 4), ("linear", 1)):
        case = _case(method, "regular", n, np.float64, nobs=64, seed=47)
        pts = _rows(case.obs)
        it = _handle(case)
        try:
            it.set_option("points_path", 1)
            with pytest.raises(interpn_amd._lib.InterpnHipError, match="unsupported"):
                it.eval_points_tensors(torch.from_numpy(pts).cuda())
            with pytest.raises(interpn_amd._lib.InterpnHipError, match="unsupported"):
                it.eval_points_host(pts)
        finally:
            it.close()


def test_argument_checks_before_any_device_work():
    """Host pointers that are never dereferenced."""
    from interpn_amd import _lib

    lib = _lib.load()
    case = _case("linear", "regular", 3, np.float64, nobs=64, seed=51)
    pts = _rows(case.obs)
    out = np.zeros(64)
    p, o = c_void_p(pts.ctypes.data), c_void_p(out.ctypes.data)
    import interpn_amd

    one = interpn_amd.Interpolator.grid1d_regular("Linear1D", 0.0, 0.5, case.vals[:9].copy())
    it = _handle(case)
    try:
        path = c_int(-5)
        for stride in (0, 1, 2):
            assert lib.interpn_hip_eval_points_device(it._h, p, stride, 64, o, None, 0, path) == INVALID
            assert lib.interpn_hip_eval_points_host(it._h, p, stride, 64, o) == INVALID
            assert lib.interpn_hip_eval_points_host(it._h, p, stride, 0, o) == INVALID
        assert lib.interpn_hip_eval_points_device(it._h, p, 3, 64, o, None, 2, path) == INVALID  # an unknown flag
        for pp, oo in ((None, o), (p, None), (None, None)):
            assert lib.interpn_hip_eval_points_device(it._h, pp, 3, 64, oo, None, 0, None) == INVALID
            assert lib.interpn_hip_eval_points_host(it._h, pp, 3, 64, oo) == INVALID
            # no points: nothing to do, whatever the other pointers are
            assert lib.interpn_hip_eval_points_device(it._h, pp, 3, 0, oo, None, 0, None) == OK
            assert lib.interpn_hip_eval_points_host(it._h, pp, 7, 0, oo) == OK
        assert lib.interpn_hip_eval_points_device(one._h, p, 0, 64, o, None, 0, None) == INVALID  # one_dim: stride >= 1
        assert lib.interpn_hip_eval_points_host(one._h, p, 0, 64, o) == INVALID
        assert lib.interpn_hip_reserve_points(it._h, 0, 1) == OK and lib.interpn_hip_reserve_points(it._h, 10, -1) == INVALID
        assert not out.any()
        assert it.last_points_path() is None
    finally:
        it.close()
        one.close()


@pytest.mark.parametrize("method", ["Linear1D", "Nearest1D"])
def test_one_dim_handles(method):
    import torch

    import interpn_amd

    rng = np.random.default_rng(5)
    vals = rng.uniform(-1, 1, 40)
    x = rng.uniform(0.0, 19.5, NPTS)
    it = interpn_amd.Interpolator.grid1d_regular(method, 0.0, 0.5, vals)
    try:
        want = _columns(it, [x])
        _assert_same(_device(it, torch.from_numpy(x).cuda().view(-1, 1)), want, "stride 1")
        assert it.last_points_path() == "direct"
        wide = torch.full((NPTS, 3), 1e30, dtype=torch.float64, device="cuda")
        wide[:, 1] = torch.from_numpy(x).cuda()
        _assert_same(_device(it, wide[:, 1:2]), want, "stride 3")
        assert it.last_points_path() == "split"
        _assert_same(it.eval_points_host(x.reshape(-1, 1)), want, "host")
    finally:
        it.close()


@pytest.mark.parametrize("kind,method,n,dtype", [("regular", "linear", 3, np.float64), ("rectilinear", "linear", 2, np.float32),
                                                 ("regular", "cubic", 3, np.float32), ("rectilinear", "nearest", 4, np.float64),
                                                 ("regular", "linear", 6, np.float64)])
def test_several_slices_and_host_chunks(kind, method, n, dtype):
    """Option points_slice forces several slices on the split path, host_chunk several chunks of the host form."""
    import torch

    case = _case(method, kind, n, dtype, seed=53)
    pts = _rows(case.obs)
    it = _handle(case)
    try:
        want = _columns(it, case.obs)
        it.set_option("points_path", 2)
        it.set_option("points_slice", 256)
        _assert_same(_device(it, torch.from_numpy(pts).cuda()), want, "six slices")
        assert it.last_points_path() == "split"
        it.set_option("host_chunk", 400)
        _assert_same(it.eval_points_host(pts), want, "host chunks of slices")
        it.set_option("points_path", 0)
        _assert_same(it.eval_points_host(pts), want, "host chunks")
    finally:
        it.close()


@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, 1e300])
def test_unrepresentable_coordinate_contract(path, bad):
    """A regular grid cannot evaluate such a coordinate: the first failing index (of the whole call, not of a slice or
    chunk) and what is written in front of it are those of `eval` on the columns."""
    import torch

    case = _case("linear", "regular", 3, np.float64, seed=61)
    k = 700  # in the third slice of 256 points, the second host chunk of 400
    case.obs[2][k] = bad
    case.obs[0][k + 300] = np.nan  # a later failure (another slice, another chunk) must not win
    case.obs[1][k + 600] = np.inf
    pts = _rows(case.obs)
    it = _handle(case)
    try:
        it.set_option("points_slice", 256)
        it.set_option("host_chunk", 400)
        # what eval does
        want = np.full(NPTS, -7.0)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
            it.eval_host(case.obs, want)
        assert (want[k:] == -7.0).all() and (want[:k] != -7.0).all()
        dev_want = it.eval_tensors([torch.from_numpy(o).cuda() for o in case.obs])
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
            it.finish()
        assert ei.value.first_bad_index == k
        it.set_option("points_path", 1 if path == "fused" else 2)
        out = np.full(NPTS, -7.0)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
            it.eval_points_host(pts, out)
        _assert_same(out, want, "host: prefix written, the rest untouched")
        got = it.eval_points_tensors(torch.from_numpy(pts).cuda())
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
            it.finish()
        assert ei.value.first_bad_index == k
        assert it.last_points_path() == path
        ok = np.ones(NPTS, dtype=bool)
        ok[[k, k + 300, k + 600]] = False
        _assert_same(got.cpu().numpy()[ok], dev_want.cpu().numpy()[ok], "device: every other point")
        # the word is clean again afterwards
        for d, i in ((2, k), (0, k + 300), (1, k + 600)):
            case.obs[d][i] = 0.0
        _assert_same(_device(it, torch.from_numpy(_rows(case.obs)).cuda()), _columns(it, case.obs), "clean again")
    finally:
        it.close()


def test_no_alloc_and_reserved_scratch():
    import torch

    import interpn_amd

    case = _case("cubic", "regular", 3, np.float64, seed=67)
    pts_t = torch.from_numpy(_rows(case.obs)).cuda()
    it = _handle(case)
    try:
        want = _columns(it, case.obs)
        # no_alloc without a reserved block: an error, not a silent allocation
        with pytest.raises(interpn_amd._lib.InterpnHipError):
            it.eval_points_tensors(pts_t, no_alloc=True)
        it.reserve_points(NPTS, 1)
        allocs = it.get_option("scratch_allocs")
        assert allocs >= 1
        _assert_same(_device(it, pts_t, no_alloc=True), want, "no_alloc after reserve")
        assert it.get_option("scratch_allocs") == allocs and it.last_points_path() == "split"
    finally:
        it.close()
    # the fused kernel takes no device memory
    case = _case("linear", "rectilinear", 3, np.float64, seed=67)
    it = _handle(case)
    try:
        want = _columns(it, case.obs)
        allocs = it.get_option("scratch_allocs")
        _assert_same(_device(it, torch.from_numpy(_rows(case.obs)).cuda(), no_alloc=True), want, "fused, no_alloc")
        assert it.get_option("scratch_allocs") == allocs and it.last_points_path() == "fused"
    finally:
        it.close()


@pytest.mark.parametrize("kind,n", [("regular", 3), ("rectilinear", 2)])
def test_graph_capture_of_one_kernel(kind, n):
    """The fused form is one kernel: captured on a side stream (a single node, no parallel branches) and replayed once on
    new points."""
    import torch

    case = _case("linear", kind, n, np.float64, nobs=5000, seed=83)
    fresh = _case("linear", kind, n, np.float64, nobs=5000, seed=84)
    it = _handle(case)
    try:
        want = _columns(it, fresh.obs)
        pts_t = torch.from_numpy(_rows(case.obs)).cuda()
        out = torch.zeros(5000, dtype=torch.float64, device="cuda")
        it.eval_points_tensors(pts_t, out)  # warm: nothing is left to allocate or build
        it.finish()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            it.eval_points_tensors(pts_t, out)
        pts_t.copy_(torch.from_numpy(_rows(fresh.obs)))
        out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        it.finish()
        _assert_same(out.cpu().numpy(), want, "replay")
    finally:
        it.close()


def test_entry_points_interpn_points_and_classes():
    import torch

    import interpn_amd

    for method, kind, n, dtype in (("linear", "regular", 3, np.float64), ("linear", "rectilinear", 2, np.float32),
                                   ("cubic", "rectilinear", 2, np.float64), ("nearest", "regular", 3, np.float32),
                                   ("cubic", "regular", 1, np.float64), ("nearest", "rectilinear", 4, np.float64)):
        case = _case(method, kind, n, dtype, nobs=77, seed=31)
        shape = (7, 11)
        cols = [o.reshape(shape) for o in case.obs]
        xi = np.stack(cols, axis=-1)
        assert xi.shape == shape + (n,)
        valsn = case.vals.reshape(case.dims)
        kw = dict(method=method, assume_regular=(kind == "regular"))
        want = interpn_amd.interpn(cols, case.grids, valsn, **kw)
        got = interpn_amd.interpn_points(xi, case.grids, valsn, **kw)
        assert isinstance(got, np.ndarray) and got.shape == shape
        _assert_same(got, want, "interpn_points numpy")
        tgot = interpn_amd.interpn_points(torch.from_numpy(xi).cuda(), case.grids, valsn, **kw)
        assert tgot.is_cuda and tuple(tgot.shape) == shape
        _assert_same(tgot.cpu().numpy(), want, "interpn_points tensor")
        out = np.full(shape, -7.0, dtype=dtype)
        assert interpn_amd.interpn_points(xi, case.grids, valsn, out=out, **kw).shape == shape
        _assert_same(out, want, "interpn_points out=")
        with pytest.raises(ValueError, match="violate interpolator bounds"):
            interpn_amd.interpn_points(xi, case.grids, valsn, check_bounds=True, **kw)
        with pytest.raises(ValueError, match="violate interpolator bounds"):
            interpn_amd.interpn_points(torch.from_numpy(xi).cuda(), case.grids, valsn, check_bounds=True, **kw)
        # the classes
        name = {"linear": "Multilinear", "cubic": "Multicubic", "nearest": "Nearest"}[method] + kind.capitalize()
        cls = getattr(interpn_amd, name)
        obj = cls.new(case.dims, case.starts, case.steps, case.vals) if kind == "regular" else cls.new(case.grids, case.vals)
        cwant = obj.eval(case.obs).reshape(shape)  # the classes' eval takes 1-D coordinate arrays
        _assert_same(obj.eval_points(xi), cwant, name)
        tres = obj.eval_points(torch.from_numpy(xi).cuda())
        assert tres.is_cuda and tuple(tres.shape) == shape
        _assert_same(tres.cpu().numpy(), cwant, name + " tensor")


def test_type_errors_and_existing_behaviour():
    import torch

    case = _case("linear", "regular", 3, np.float64, nobs=64, seed=71)
    pos = torch.from_numpy(_rows(case.obs)).cuda()
    it = _handle(case)
    try:
        with pytest.raises(TypeError, match="pts: expected a 2-D torch.float64 CUDA tensor"):
            it.eval_points_tensors(pos.float())
        with pytest.raises(TypeError, match="pts: expected a 2-D torch.float64 CUDA tensor"):
            it.eval_points_tensors(pos.reshape(-1))
        with pytest.raises(TypeError, match="stride\\(1\\) == 1"):
            it.eval_points_tensors(pos.T.contiguous().T)  # shape (n, 3), column-major
        with pytest.raises(TypeError):
            it.eval_points_tensors(pos.cpu())
        with pytest.raises(TypeError):
            it.eval_points_tensors(_rows(case.obs))
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            it.eval_points_tensors(pos[:, :2])
        with pytest.raises(TypeError):
            it.eval_points_host(_rows(case.obs).astype(np.float32))
        with pytest.raises(TypeError):
            it.eval_points_host(case.obs[0])
        with pytest.raises(ValueError, match="contiguous"):
            it.eval_points_host(np.asfortranarray(_rows(case.obs)))
        # existing behaviour stays: a column of a point-major tensor is not a coordinate array
        with pytest.raises(TypeError, match="expected a contiguous 1-D"):
            it.eval_tensors([pos[:, d] for d in range(3)])
    finally:
        it.close()
