"""Point-major gradients on the GPU (interpn_hip_eval_points_grad_*, Interpolator.eval_points_grad_*, interpn_points_grad, the
classes' eval_points_grad, autograd.interp_points): positions as ONE array of shape (n, N), the gradient in the same layout.
The yardstick is the same handle's `eval_grad_tensors` / `eval_cubic_grad_tensors` on the de-interleaved columns (pinned to the
restatements of the definitions by tests/test_grad_gpu.py and tests/test_cubic_grad_gpu.py); one case per method and kind is
compared with the restatement directly.  Every comparison is bit for bit, a NaN need only be a NaN on both sides."""

from ctypes import c_int, c_void_p

import numpy as np
import pytest

from tests import cubic_grad_restatement as cg
from tests import grad_restatement as gr
from tests.helpers import synthetic_case
from tests.test_grad_gpu import AXES
from tests.test_points_gpu import CUBIC_AXES

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, OUT_OF_MEMORY = 0, 32, 33, 35
FUSED = {"linear": "interpn::k_linear_points_grad<", "cubic": "interpn::k_cubic_points_grad<"}
NPTS = 1501  # odd: the two-points-per-lane form has a tail; 3 workgroups, 11 full waves and a ragged one
SENTINEL = -7.25
CUBIC_LAYOUTS = ["44", "24", "22", "14", "11"]  # every tile-step pair a cubic handle can have; "11" gathers by LDS-DMA


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_BRICKS", "INTERPN_HIP_FORCE_GENERIC", "INTERPN_HIP_AXIS_REGS", "INTERPN_HIP_PPL",
                 "INTERPN_HIP_POINTS_PATH", "INTERPN_HIP_POINTS_LOAD", "INTERPN_HIP_POINTS_STORE", "INTERPN_HIP_POINTS_SLICE"):
        monkeypatch.delenv(name, raising=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist(), got[~same][:4], want[~same][:4])


def _handle(case, fma=True, linearize=False):
    import interpn_amd

    dt = case.vals.dtype
    if case.kind == "regular":
        return interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, case.vals,
                                                linearize_extrapolation=linearize, dtype=dt, fma=fma)
    return interpn_amd.Interpolator.rectilinear(case.method, case.grids, case.vals, linearize_extrapolation=linearize, dtype=dt,
                                                fma=fma)


def _case(method, kind, n, dtype, nobs=NPTS, seed=0, axes=None):
    axes = axes or (CUBIC_AXES if method == "cubic" else AXES)[n]
    return synthetic_case(method, kind, n, axes, nobs, 7700 + 17 * n + seed + (kind == "regular"), dtype=dtype, specials=True)


def _columns(it, obs):
    """The yardstick: the handle's column-form value and gradient, the gradient turned to shape (n, N)."""
    import torch

    call = it.eval_cubic_grad_tensors if it.method == "cubic" else it.eval_grad_tensors
    out, grad = call([torch.from_numpy(np.ascontiguousarray(o)).cuda() for o in obs])
    it.finish()
    return out.cpu().numpy(), np.ascontiguousarray(grad.cpu().numpy().T)


def _rows(obs):
    return np.ascontiguousarray(np.stack(obs, axis=1))


def _device(it, pts_t, out=None, grad=None, **kw):
    out, grad = it.eval_points_grad_tensors(pts_t, out, grad, **kw)
    it.finish()
    return out.cpu().numpy(), grad.cpu().numpy()


def _expected_path(n):
    return "fused" if n in (2, 3) else ("direct" if n == 1 else "split")


def _kernel_args(name):
    return [a.strip() for a in name[name.index("<") + 1:-1].split(",")]


# ---- 1. device and host forms on every supported handle
_EVERY = [(m, n, lin) for m in ("linear", "cubic") for n in range(1, 9) for lin in ((False, True) if m == "cubic" and n in (2, 3) else (False,))]


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("method,n,linearize", _EVERY)
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_device_and_host_match_the_columns(kind, method, n, linearize, dtype, fma):
    import torch

    case = _case(method, kind, n, dtype, nobs=NPTS if n <= 6 else 400)
    it = _handle(case, fma, linearize)
    try:
        want_out, want_grad = _columns(it, case.obs)
        if n == 3 and dtype == np.float64 and fma and not linearize:  # one case per method and kind: the yardstick itself
            if method == "linear":
                r_out, r_grad, ok = gr.eval_grad_case(case, fma=True)
            else:
                args = (case.dims, case.starts, case.steps) if kind == "regular" else case.grids
                r_out, r_grad, ok = cg.eval_grad(kind, args, case.vals, case.obs, linearize=False, fma=True, dtype=np.dtype(dtype))
            assert ok.all()
            _assert_same(want_out, r_out, "columns against the restatement: out")
            _assert_same(want_grad, np.ascontiguousarray(np.asarray(r_grad).T), "columns against the restatement: grad")
        pts = _rows(case.obs)
        pts_t = torch.from_numpy(pts).cuda()
        out, grad = _device(it, pts_t)
        name = it.kernel_name()
        if n in (2, 3):
            assert name.startswith(FUSED[method]), name
        else:
            assert not name.startswith(FUSED[method]) and "points_grad" not in name, name
        assert it.last_points_path() == _expected_path(n)
        _assert_same(out, want_out, "device out")
        _assert_same(grad, want_grad, "device grad")
        plain = it.eval_points_tensors(pts_t)
        it.finish()
        _assert_same(out, plain.cpu().numpy(), "value against eval_points_tensors")
        hout, hgrad = it.eval_points_grad_host(pts)
        _assert_same(hout, want_out, "host out")
        _assert_same(hgrad, want_grad, "host grad")
    finally:
        it.close()


# ---- 2. every table layout and axis search
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("layout,dtype", [("11", np.float64), ("12", np.float64), ("22", np.float64), ("11", np.float32),
                                          ("12", np.float32), ("22", np.float32), ("j4", np.float32)])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_3d_multilinear_under_every_brick_layout(kind, layout, dtype, fma, monkeypatch):
    import torch

    monkeypatch.setenv("INTERPN_HIP_BRICKS", layout)
    case = _case("linear", kind, 3, dtype, seed=11, axes=[21, 19, 23])
    it = _handle(case, fma)
    try:
        want_out, want_grad = _columns(it, case.obs)
        pts_t = torch.from_numpy(_rows(case.obs)).cuda()
        for ppl in (0, 1):
            it.set_option("ppl", ppl)
            out, grad = _device(it, pts_t)
            name = it.kernel_name()
            assert name.startswith(FUSED["linear"]), name
            args = _kernel_args(name)  # T, N, RECT, FMA, SI, SJ, PPL, AXR, CELL
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
    """The axis searches of the multilinear kernels: across lanes (lane table, probe sequence), in LDS, through L2."""
    import torch

    if n == 2:
        monkeypatch.setenv("INTERPN_HIP_BRICKS", "on")  # a 2-D grid of 64 x 64 f32 values at most is L1-sized: no table by itself
    case = _case("linear", "rectilinear", n, dtype, seed=23, axes=axes)
    it = _handle(case)
    seen = set()
    try:
        assert it.table_layout()[0] > 0
        want_out, want_grad = _columns(it, case.obs)
        pts_t = torch.from_numpy(_rows(case.obs)).cuda()
        for regs, lds_kb in ((-1, -1), (1, -1), (0, -1), (0, 0)):
            it.set_option("axis_regs", regs)
            it.set_option("axis_lds_kb", lds_kb)
            out, grad = _device(it, pts_t)
            name = it.kernel_name()
            assert name.startswith(FUSED["linear"]), name
            seen.add(name)
            _assert_same(out, want_out, (regs, lds_kb, "out"))
            _assert_same(grad, want_grad, (regs, lds_kb, "grad"))
    finally:
        it.close()
    if max(axes) <= 64:
        assert len(seen) >= 2, seen  # lanes and LDS forms both ran


@pytest.mark.parametrize("layout", CUBIC_LAYOUTS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [2, 3])
def test_multicubic_under_every_tile_layout(n, kind, dtype, layout, monkeypatch):
    import torch

    monkeypatch.setenv("INTERPN_HIP_BRICKS", layout)
    case = _case("cubic", kind, n, dtype, seed=29, axes=[9, 7] if n == 2 else [7, 5, 6])
    pts_t = torch.from_numpy(_rows(case.obs)).cuda()
    for linearize in (True, False):
        it = _handle(case, True, linearize)
        try:
            assert it.table_layout()[0] > 0
            for fma in (True, False):
                it.set_option("fma", int(fma))
                want_out, want_grad = _columns(it, case.obs)
                assert it.kernel_name().startswith("interpn::k_cubic_grad<"), it.kernel_name()
                out, grad = _device(it, pts_t)
                name = it.kernel_name()
                assert name.startswith(FUSED["cubic"]), name
                args = _kernel_args(name)  # T, N, RECT, FMA, SI, SJ
                assert args[1] == str(n) and args[2] == ("true" if kind == "rectilinear" else "false"), name
                assert args[3] == ("true" if fma else "false") and args[4:6] == [layout[0], layout[1]], name
                _assert_same(out, want_out, (layout, linearize, fma, "out"))
                _assert_same(grad, want_grad, (layout, linearize, fma, "grad"))
        finally:
            it.close()


# ---- 3. load x store forms and block shapes
def _strided(flat, offset, count, n, stride):
    """A (count, n) view of the 1-D tensor `flat`: rows `stride` elements apart from element `offset` on; the last row ends
    with its n-th element."""
    import torch

    return torch.as_strided(flat, (count, n), (stride, 1), offset)


def _untouched(flat, offset, count, n, stride):
    """The elements of `flat` that are not part of the view still hold the sentinel."""
    keep = np.ones(flat.numel(), dtype=bool)
    for d in range(n):
        keep[offset + np.arange(count) * stride + d] = False
    return bool((flat.cpu().numpy()[keep] == SENTINEL).all())


@pytest.mark.parametrize("method,kind,n,dtype", [("linear", "regular", 3, np.float64), ("linear", "rectilinear", 3, np.float64),
                                                 ("linear", "regular", 3, np.float32), ("linear", "regular", 2, np.float64),
                                                 ("linear", "rectilinear", 2, np.float32), ("cubic", "regular", 2, np.float64),
                                                 ("cubic", "rectilinear", 3, np.float32), ("cubic", "regular", 2, np.float32)])
def test_load_and_store_forms_strides_and_alignment(method, kind, n, dtype):
    """Packed rows, rows of wider tensors (stride N + 1) on either side, bases and an `out` one element off a 16-byte
    boundary, the counts around a wave and a workgroup; every coordinate load form (option points_load: 1 per-lane vectors,
    2 the wave's span through LDS, 3 elements) times every gradient-row store form (option points_store, the same numbers).
    Nothing outside the blocks is written: the extra column of a strided gradient block, the elements behind the last row's
    N-th and behind out[n - 1] keep their sentinel."""
    import torch

    case = _case(method, kind, n, dtype, seed=37)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    it = _handle(case)
    try:
        want_out, want_grad = _columns(it, case.obs)
        pts = _rows(case.obs)
        forms = [(ld, st) for ld in (1, 2, 3) for st in (1, 2, 3)] if method == "linear" else [(0, 0)]
        for count in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, NPTS):
            packed = torch.from_numpy(np.ascontiguousarray(pts[:count])).cuda()
            wide = torch.full((count * (n + 1) + 2,), 1e30, dtype=tdt, device="cuda")  # coordinates nobody may read
            _strided(wide, 0, count, n, n + 1).copy_(packed)
            off1 = torch.full((count * n + 3,), 1e30, dtype=tdt, device="cuda")
            off1[1:1 + count * n] = packed.reshape(-1)
            # (points view, gradient offset, gradient stride, out offset)
            shapes = [("packed", packed, 0, n, 0), ("point stride N + 1", _strided(wide, 0, count, n, n + 1), 0, n, 0),
                      ("grad stride N + 1", packed, 0, n + 1, 0), ("bases + 1", _strided(off1, 1, count, n, n), 1, n, 0),
                      ("out + 1", packed, 0, n, 1), ("both strides N + 1, grad base + 2", _strided(wide, 0, count, n, n + 1), 2, n + 1, 0)]
            for load, store in forms:
                it.set_option("points_load", load)
                it.set_option("points_store", store)
                for what, view, goff, gstride, ooff in shapes:
                    gflat = torch.full((goff + (count - 1) * gstride + n + 2,), SENTINEL, dtype=tdt, device="cuda")
                    oflat = torch.full((ooff + count + 2,), SENTINEL, dtype=tdt, device="cuda")
                    out, grad = _device(it, view, oflat[ooff:ooff + count], _strided(gflat, goff, count, n, gstride))
                    tag = (load, store, count, what)
                    assert it.kernel_name().startswith(FUSED[method]) and it.last_points_path() == "fused", tag
                    if method == "linear":  # one point per lane exactly when `out` is off the two-element boundary
                        assert _kernel_args(it.kernel_name())[6] == ("1" if ooff else "2"), tag
                    _assert_same(out, want_out[:count], tag + ("out",))
                    _assert_same(grad, want_grad[:count], tag + ("grad",))
                    assert _untouched(gflat, goff, count, n, gstride), tag + ("gradient block's neighbours",)
                    assert _untouched(oflat, ooff, count, 1, 1), tag + ("out's neighbours",)
            # the host form takes the row strides of numpy views
            hwide = np.full((count, n + 1), 1e30, dtype=dtype)
            hwide[:, :n] = pts[:count]
            hg = np.full((count, n + 1), SENTINEL, dtype=dtype)
            hout, hgrad = it.eval_points_grad_host(hwide[:, :n], None, hg[:, :n])
            _assert_same(hout, want_out[:count], (count, "host out"))
            _assert_same(np.ascontiguousarray(hgrad), want_grad[:count], (count, "host grad"))
            assert (hg[:, n] == SENTINEL).all(), (count, "host: the extra column")
    finally:
        it.close()


# ---- 4. split path
@pytest.mark.parametrize("method,kind,n,dtype", [("linear", "regular", 3, np.float64), ("cubic", "rectilinear", 2, np.float32),
                                                 ("cubic", "regular", 3, np.float64), ("linear", "rectilinear", 2, np.float32)])
def test_split_gives_the_fused_bits(method, kind, n, dtype):
    """points_path = 2 with points_slice = 256 on 1501 points: six slices; packed and strided gradient rows."""
    import torch

    case = _case(method, kind, n, dtype, seed=43)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    pts_t = torch.from_numpy(_rows(case.obs)).cuda()
    it = _handle(case)
    try:
        want_out, want_grad = _columns(it, case.obs)
        it.set_option("points_path", 1)
        f_out, f_grad = _device(it, pts_t)
        assert it.kernel_name().startswith(FUSED[method]) and it.last_points_path() == "fused"
        it.set_option("points_path", 2)
        it.set_option("points_slice", 256)
        s_out, s_grad = _device(it, pts_t)
        assert "points_grad" not in it.kernel_name() and it.last_points_path() == "split"
        _assert_same(f_out, want_out, "fused out")
        _assert_same(f_grad, want_grad, "fused grad")
        _assert_same(s_out, f_out, "split out")
        _assert_same(s_grad, f_grad, "split grad")
        for gstride in (n + 1, 40):  # 40: rows longer than the interleaving tile takes
            gflat = torch.full(((NPTS - 1) * gstride + n + 2,), SENTINEL, dtype=tdt, device="cuda")
            _, g = _device(it, pts_t, None, _strided(gflat, 0, NPTS, n, gstride))
            _assert_same(g, f_grad, ("split, grad stride", gstride))
            assert _untouched(gflat, 0, NPTS, n, gstride), gstride
        it.set_option("points_path", 0)
        it.set_option("force_generic", 1)
        g_out, g_grad = _device(it, pts_t)
        assert it.last_points_path() == "split"
        _assert_same(g_out, want_out, "force_generic out")
        _assert_same(g_grad, want_grad, "force_generic grad")
    finally:
        it.close()


@pytest.mark.parametrize("method,kind,n,dtype", [("linear", "regular", 5, np.float64), ("cubic", "rectilinear", 4, np.float32),
                                                 ("linear", "rectilinear", 1, np.float32), ("cubic", "regular", 1, np.float64)])
def test_split_and_direct_paths_strides_and_alignment(method, kind, n, dtype):
    import torch

    case = _case(method, kind, n, dtype, seed=39)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    it = _handle(case)
    try:
        want_out, want_grad = _columns(it, case.obs)
        pts = _rows(case.obs)
        it.set_option("points_slice", 256)
        for count in (1, 255, 256, 257, NPTS):
            packed = torch.from_numpy(np.ascontiguousarray(pts[:count])).cuda()
            out, grad = _device(it, packed)
            assert it.last_points_path() == ("direct" if n == 1 else "split")
            _assert_same(out, want_out[:count], (count, "out"))
            _assert_same(grad, want_grad[:count], (count, "grad"))
            for extra in (1, 40):
                wide = torch.full(((count - 1) * (n + extra) + n + 1,), 1e30, dtype=tdt, device="cuda")
                _strided(wide, 0, count, n, n + extra).copy_(packed)
                gflat = torch.full((1 + (count - 1) * (n + extra) + n + 2,), SENTINEL, dtype=tdt, device="cuda")
                oflat = torch.full((count + 3,), SENTINEL, dtype=tdt, device="cuda")
                out, grad = _device(it, _strided(wide, 0, count, n, n + extra), oflat[1:1 + count],
                                    _strided(gflat, 1, count, n, n + extra))
                assert it.last_points_path() == ("direct" if n == 1 and count == 1 else "split")  # one point has no stride
                _assert_same(out, want_out[:count], (count, extra, "out"))
                _assert_same(grad, want_grad[:count], (count, extra, "grad"))
                assert _untouched(gflat, 1, count, n, n + extra) and _untouched(oflat, 1, count, 1, 1), (count, extra)
    finally:
        it.close()


def test_no_alloc_and_reserved_scratch():
    import torch

    import interpn_amd

    case = _case("linear", "regular", 4, np.float64, seed=67)
    pts_t = torch.from_numpy(_rows(case.obs)).cuda()
    it = _handle(case)
    try:
        want_out, want_grad = _columns(it, case.obs)
        # no_alloc without a reserved block: an error, not a silent allocation
        path = c_int(-5)
        st = interpn_amd._lib.load().interpn_hip_eval_points_grad_device(
            it._h, c_void_p(pts_t.data_ptr()), 4, NPTS, c_void_p(torch.empty(NPTS, dtype=torch.float64, device="cuda").data_ptr()),
            c_void_p(torch.empty((NPTS, 4), dtype=torch.float64, device="cuda").data_ptr()), 4, None, 1, path)
        assert st == OUT_OF_MEMORY
        with pytest.raises(interpn_amd._lib.InterpnHipError):
            it.eval_points_grad_tensors(pts_t, no_alloc=True)
        it.reserve_points(NPTS, 1)  # the value form's block is too small for N coordinate and N component arrays
        with pytest.raises(interpn_amd._lib.InterpnHipError):
            it.eval_points_grad_tensors(pts_t, no_alloc=True)
        it.reserve_points_grad(NPTS, 1)
        allocs = it.get_option("scratch_allocs")
        assert allocs >= 1
        out, grad = _device(it, pts_t, no_alloc=True)
        assert it.get_option("scratch_allocs") == allocs and it.last_points_path() == "split"
        _assert_same(out, want_out, "no_alloc after reserve: out")
        _assert_same(grad, want_grad, "no_alloc after reserve: grad")
    finally:
        it.close()
    # the fused kernels take no device memory
    for method in ("linear", "cubic"):
        case = _case(method, "rectilinear", 3, np.float64, seed=67)
        it = _handle(case)
        try:
            want_out, want_grad = _columns(it, case.obs)
            allocs = it.get_option("scratch_allocs")
            out, grad = _device(it, torch.from_numpy(_rows(case.obs)).cuda(), no_alloc=True)
            assert it.get_option("scratch_allocs") == allocs and it.last_points_path() == "fused"
            _assert_same(grad, want_grad, "fused, no_alloc")
        finally:
            it.close()


# ---- 5. failing points on regular grids
@pytest.mark.parametrize("bad", [np.nan, np.inf, 1e300])
@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_unrepresentable_coordinate_contract(method, path, bad):
    """The first failing index of the whole call (not of a slice or chunk) from `finish`; the host form writes exactly
    out[0..i) and gradient rows [0..i)."""
    import torch

    case = _case(method, "regular", 3, np.float64, seed=61)
    for k in (100, 700):  # in the first slice of 256 points and chunk of 400; in the third slice, the second chunk
        obs = [o.copy() for o in case.obs]
        obs[2][k] = bad
        obs[0][k + 300] = np.nan  # a later failure (another slice, another chunk) must not win
        obs[1][k + 600] = np.inf
        pts = _rows(obs)
        it = _handle(case)
        try:
            it.set_option("points_slice", 256)
            it.set_option("host_chunk", 400)
            clean_out, clean_grad = _columns(it, case.obs)
            it.set_option("points_path", 1 if path == "fused" else 2)
            out = np.full(NPTS, SENTINEL)
            grad = np.full((NPTS, 4), SENTINEL)
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
                it.eval_points_grad_host(pts, out, grad[:, :3])
            _assert_same(out[:k], clean_out[:k], "host: values in front")
            _assert_same(np.ascontiguousarray(grad[:k, :3]), clean_grad[:k], "host: rows in front")
            assert (out[k:] == SENTINEL).all() and (grad[k:] == SENTINEL).all() and (grad[:, 3] == SENTINEL).all()
            got_out, got_grad = it.eval_points_grad_tensors(torch.from_numpy(pts).cuda())
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
                it.finish()
            assert ei.value.first_bad_index == k
            assert it.last_points_path() == path
            ok = np.ones(NPTS, dtype=bool)
            ok[[k, k + 300, k + 600]] = False
            _assert_same(got_out.cpu().numpy()[ok], clean_out[ok], "device: every other point")
            _assert_same(got_grad.cpu().numpy()[ok], clean_grad[ok], "device: every other row")
            # the word is clean again afterwards
            o2, g2 = _device(it, torch.from_numpy(_rows(case.obs)).cuda())
            _assert_same(o2, clean_out, "clean again")
            _assert_same(g2, clean_grad, "clean again")
        finally:
            it.close()


# ---- 6. non-finite coordinates on rectilinear grids
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_non_finite_coordinates_propagate_as_in_the_column_form(method, n):
    import torch

    case = _case(method, "rectilinear", n, np.float64, seed=71)
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        for d in range(n):
            case.obs[d][10 + 7 * (i * n + d)] = v
    case.obs[0][900], case.obs[n - 1][900] = np.inf, np.nan
    it = _handle(case)
    try:
        want_out, want_grad = _columns(it, case.obs)
        out, grad = _device(it, torch.from_numpy(_rows(case.obs)).cuda())
        _assert_same(out, want_out, "out")
        _assert_same(grad, want_grad, "grad")
        assert np.isnan(want_out).any()
        hout, hgrad = it.eval_points_grad_host(_rows(case.obs))
        _assert_same(hout, want_out, "host out")
        _assert_same(hgrad, want_grad, "host grad")
    finally:
        it.close()


# ---- 7. what is unsupported, and the checks before any device work
def test_unsupported_handles_and_argument_checks():
    """Host pointers that are never dereferenced."""
    import torch

    import interpn_amd
    from interpn_amd import _lib

    lib = _lib.load()
    case = _case("linear", "regular", 3, np.float64, nobs=64, seed=51)
    pts = _rows(case.obs)
    out = np.zeros(64)
    grad = np.zeros((64, 3))
    p, o, g = c_void_p(pts.ctypes.data), c_void_p(out.ctypes.data), c_void_p(grad.ctypes.data)

    def dev(h, pp, stride, npts, oo, gg, gstride, flags=0):
        return lib.interpn_hip_eval_points_grad_device(h, pp, stride, npts, oo, gg, gstride, None, flags, c_int(-5))

    def host(h, pp, stride, npts, oo, gg, gstride):
        return lib.interpn_hip_eval_points_grad_host(h, pp, stride, npts, oo, gg, gstride)

    one = interpn_amd.Interpolator.grid1d_regular("Linear1D", 0.0, 0.5, case.vals[:9].copy())
    near = interpn_amd.Interpolator.regular("nearest", case.dims, case.starts, case.steps, case.vals, dtype=np.float64)
    it = _handle(case)
    try:
        # 2. neither multilinear nor multicubic: before the strides, the point count and the pointers are looked at
        for h in (one, near):
            for stride, npts, gg in ((3, 64, g), (0, 64, g), (3, 0, g), (3, 64, None)):
                assert dev(h._h, p, stride, npts, o, gg, 3) == UNSUPPORTED
                assert host(h._h, p, stride, npts, o, gg, 3) == UNSUPPORTED
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            near.eval_points_grad_tensors(torch.from_numpy(pts).cuda())
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            near.eval_points_grad_host(pts)
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            one.eval_points_grad_host(pts[:, :1])
        # 3. strides, before 4. no points
        for stride, gstride in ((0, 3), (2, 3), (3, 2), (3, 0)):
            for npts in (64, 0):
                assert dev(it._h, p, stride, npts, o, g, gstride) == INVALID
                assert host(it._h, p, stride, npts, o, g, gstride) == INVALID
        # 4. no points: nothing to do, whatever the pointers are; 5. NULL pointers
        for pp, oo, gg in ((None, o, g), (p, None, g), (p, o, None), (None, None, None)):
            assert dev(it._h, pp, 3, 64, oo, gg, 3) == INVALID
            assert host(it._h, pp, 3, 64, oo, gg, 4) == INVALID
            assert dev(it._h, pp, 3, 0, oo, gg, 3) == OK
            assert host(it._h, pp, 7, 0, oo, gg, 5) == OK
        # 6. a block whose bytes overflow size_t
        assert dev(it._h, p, 1 << 40, 1 << 40, o, g, 3) == INVALID
        assert host(it._h, p, 3, 1 << 40, o, g, 1 << 40) == INVALID
        assert dev(it._h, p, 3, 64, o, g, 3, flags=2) == INVALID  # an unknown flag
        assert lib.interpn_hip_reserve_points_grad(it._h, 0, 1) == OK and lib.interpn_hip_reserve_points_grad(it._h, 10, -1) == INVALID
        assert not out.any() and not grad.any()
        assert it.last_points_path() is None
    finally:
        it.close()
        one.close()
        near.close()
    # 7. fused only, where no fused form exists
    for method, n in (("linear", 4), ("cubic", 4), ("linear", 1)):
        case = _case(method, "regular", n, np.float64, nobs=64, seed=47)
        it = _handle(case)
        try:
            it.set_option("points_path", 1)
            with pytest.raises(_lib.InterpnHipError, match="unsupported"):
                it.eval_points_grad_tensors(torch.from_numpy(_rows(case.obs)).cuda())
            with pytest.raises(_lib.InterpnHipError, match="unsupported"):
                it.eval_points_grad_host(_rows(case.obs))
        finally:
            it.close()


def test_type_errors():
    import torch

    case = _case("linear", "regular", 3, np.float64, nobs=64, seed=71)
    pos = torch.from_numpy(_rows(case.obs)).cuda()
    it = _handle(case)
    try:
        with pytest.raises(TypeError, match="pts: expected a 2-D torch.float64 CUDA tensor"):
            it.eval_points_grad_tensors(pos.float())
        with pytest.raises(TypeError, match="stride\\(1\\) == 1"):
            it.eval_points_grad_tensors(pos.T.contiguous().T)
        with pytest.raises(AssertionError, match="Dimension mismatch"):
            it.eval_points_grad_tensors(pos[:, :2])
        with pytest.raises(TypeError, match="grad: expected a 2-D"):
            it.eval_points_grad_tensors(pos, None, torch.zeros(3, 64, dtype=torch.float64, device="cuda").T)
        with pytest.raises(ValueError, match="grad: expected shape"):
            it.eval_points_grad_tensors(pos, None, torch.zeros(3, 64, dtype=torch.float64, device="cuda"))
        with pytest.raises(TypeError):
            it.eval_points_grad_host(_rows(case.obs).astype(np.float32))
        with pytest.raises(ValueError, match="grad: expected shape"):
            it.eval_points_grad_host(_rows(case.obs), None, np.zeros((3, 64)))
        with pytest.raises(ValueError, match="contiguous"):
            it.eval_points_grad_host(_rows(case.obs), None, np.asfortranarray(np.zeros((64, 3))))
    finally:
        it.close()


# ---- 8. graph capture
@pytest.mark.parametrize("method,kind", [("linear", "regular"), ("cubic", "rectilinear")])
def test_graph_capture_of_one_kernel(method, kind):
    """The fused form is one kernel: captured on a side stream (a single node, no parallel branches) and replayed once on new
    points; the replay gives the eager bits.  That the captured call itself took the fused path, and launched the fused kernel
    and nothing behind it, is read from the handle right after the capture: the call in front of it went through the split
    path, so neither the path nor the kernel name is left over from an earlier call."""
    import torch

    case = _case(method, kind, 3, np.float64, nobs=5000, seed=83)
    fresh = _case(method, kind, 3, np.float64, nobs=5000, seed=84)
    it = _handle(case)
    try:
        pts_t = torch.from_numpy(_rows(case.obs)).cuda()
        out = torch.zeros(5000, dtype=torch.float64, device="cuda")
        grad = torch.zeros((5000, 3), dtype=torch.float64, device="cuda")
        it.eval_points_grad_tensors(pts_t, out, grad)  # warm: nothing is left to allocate or build
        it.finish()
        assert it.last_points_path() == "fused"
        eager_out, eager_grad = _device(it, torch.from_numpy(_rows(fresh.obs)).cuda())
        it.set_option("points_path", 2)
        _device(it, pts_t)
        assert it.last_points_path() == "split" and not it.kernel_name().startswith(FUSED[method]), it.kernel_name()
        it.set_option("points_path", 0)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            it.eval_points_grad_tensors(pts_t, out, grad, no_alloc=True)
        # the captured call: the fused path (the split path would need a reserved block: none was reserved), whose only
        # launch is the fused kernel
        assert it.last_points_path() == "fused"
        assert it.kernel_name().startswith(FUSED[method]), it.kernel_name()
        pts_t.copy_(torch.from_numpy(_rows(fresh.obs)))
        out.zero_()
        grad.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        it.finish()
        _assert_same(out.cpu().numpy(), eager_out, "replay out")
        _assert_same(grad.cpu().numpy(), eager_grad, "replay grad")
    finally:
        it.close()


# ---- 9. interpn_points_grad and the classes
def test_entry_points_interpn_points_grad_and_classes():
    import torch

    import interpn_amd

    for method, kind, n, dtype in (("linear", "regular", 3, np.float64), ("linear", "rectilinear", 2, np.float32),
                                   ("cubic", "rectilinear", 2, np.float64), ("cubic", "regular", 3, np.float32),
                                   ("cubic", "regular", 1, np.float64), ("linear", "rectilinear", 4, np.float64)):
        case = _case(method, kind, n, dtype, nobs=77, seed=31)
        shape = (7, 11)
        cols = [o.reshape(shape) for o in case.obs]
        xi = np.stack(cols, axis=-1)
        assert xi.shape == shape + (n,)
        valsn = case.vals.reshape(case.dims)
        for lin in ((True, False) if method == "cubic" else (True,)):
            kw = dict(method=method, assume_regular=(kind == "regular"), linearize_extrapolation=lin)
            want_out, want_grad = interpn_amd.interpn_grad(cols, case.grids, valsn, **kw)
            want_grad = np.ascontiguousarray(np.moveaxis(want_grad, 0, -1))
            out, grad = interpn_amd.interpn_points_grad(xi, case.grids, valsn, **kw)
            assert isinstance(out, np.ndarray) and out.shape == shape and grad.shape == xi.shape
            _assert_same(out, want_out, "interpn_points_grad numpy out")
            _assert_same(grad, want_grad, "interpn_points_grad numpy grad")
            tout, tgrad = interpn_amd.interpn_points_grad(torch.from_numpy(xi).cuda(), case.grids, valsn, **kw)
            assert tout.is_cuda and tuple(tout.shape) == shape and tuple(tgrad.shape) == xi.shape
            _assert_same(tout.cpu().numpy(), want_out, "interpn_points_grad tensor out")
            _assert_same(tgrad.cpu().numpy(), want_grad, "interpn_points_grad tensor grad")
            with pytest.raises(ValueError, match="violate interpolator bounds"):
                interpn_amd.interpn_points_grad(xi, case.grids, valsn, check_bounds=True, **kw)
            with pytest.raises(ValueError, match="violate interpolator bounds"):
                interpn_amd.interpn_points_grad(torch.from_numpy(xi).cuda(), case.grids, valsn, check_bounds=True, **kw)
        # the classes (multicubic: linearize_extrapolation = True, their default)
        name = {"linear": "Multilinear", "cubic": "Multicubic"}[method] + kind.capitalize()
        cls = getattr(interpn_amd, name)
        obj = cls.new(case.dims, case.starts, case.steps, case.vals) if kind == "regular" else cls.new(case.grids, case.vals)
        cwant_out, cwant_grad = (obj.eval_cubic_grad if method == "cubic" else obj.eval_grad)(case.obs)
        cwant_grad = np.ascontiguousarray(cwant_grad.T).reshape(xi.shape)
        cout, cgrad = obj.eval_points_grad(xi)
        _assert_same(cout, cwant_out.reshape(shape), name)
        _assert_same(cgrad, cwant_grad, name + " grad")
        tout, tgrad = obj.eval_points_grad(torch.from_numpy(xi).cuda())
        assert tout.is_cuda and tuple(tout.shape) == shape and tuple(tgrad.shape) == xi.shape
        _assert_same(tout.cpu().numpy(), cwant_out.reshape(shape), name + " tensor")
        _assert_same(tgrad.cpu().numpy(), cwant_grad, name + " tensor grad")


# ---- 10. autograd
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("method,kind", [("cubic", "regular"), ("cubic", "rectilinear"), ("linear", "rectilinear")])
def test_autograd_interp_points(method, kind, n):
    """The forward value is eval_points'; pts.grad equals the stacked result of autograd.interp on the columns bit for bit;
    gradcheck on f64 handles at a quarter and three quarters of randomly chosen cells, far from every knot relative to its
    step (1e-6), as tests/test_grad_gpu.py and tests/test_cubic_grad_gpu.py do."""
    import torch

    from interpn_amd import autograd

    case = _case(method, kind, n, np.float64, nobs=64, seed=91)
    rng = np.random.default_rng(17 + n)
    cols = []
    for d in range(n):
        g = np.asarray(case.grids[d], dtype=np.float64)
        c = rng.integers(0, g.size - 1, 24)
        frac = np.where(rng.random(24) < 0.5, 0.25, 0.75)
        cols.append(g[c] + frac * (g[c + 1] - g[c]))
    it = _handle(case, True, True)
    try:
        pts = torch.from_numpy(_rows(cols)).cuda().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda p: autograd.interp_points(it, p), (pts,), eps=1e-6, atol=1e-6, rtol=1e-5)
        y = autograd.interp_points(it, pts)
        plain = it.eval_points_tensors(pts.detach())
        it.finish()
        assert bool((y.detach() == plain).all())
        w = torch.from_numpy(rng.uniform(-2, 2, 24)).cuda()
        (y * w).sum().backward()
        inputs = [torch.from_numpy(c).cuda().requires_grad_(True) for c in cols]
        (autograd.interp(it, inputs) * w).sum().backward()
        stacked = torch.stack([t.grad for t in inputs], dim=-1)
        assert tuple(pts.grad.shape) == (24, n) and bool((pts.grad == stacked).all())
        # any leading shape, and a view of a wider tensor
        buf = torch.zeros((4, 6, n + 1), dtype=torch.float64, device="cuda")
        buf[..., :n] = pts.detach().reshape(4, 6, n)
        buf.requires_grad_(True)
        y2 = autograd.interp_points(it, buf[..., :n])
        assert tuple(y2.shape) == (4, 6)
        (y2 * w.reshape(4, 6)).sum().backward()
        assert bool((buf.grad[..., :n].reshape(24, n) == stacked).all()) and bool((buf.grad[..., n] == 0).all())
    finally:
        it.close()


# ---- the fused multilinear kernel's row-stride limit
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
def test_row_stride_limit_of_the_fused_multilinear_kernel(n, dtype):
    """k_linear_points_grad addresses a workgroup's rows by 32-bit offsets, so rows of up to 2^20 elements are fused and
    longer ones take the split path (points_path = 1 is then unsupported).  Two points at a stride of exactly 2^20 and of
    2^20 + 1 elements, in the points block, in the gradient block and in both; and 513 points at 2^20, where the last point of
    the first workgroup's iteration (point 511) has the largest offset there is: 511 * 2^20 elements."""
    import torch

    from interpn_amd import _lib

    limit = 1 << 20
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    case = _case("linear", "regular", n, dtype, nobs=513, seed=97)
    it = _handle(case)
    try:
        want_out, want_grad = _columns(it, case.obs)
        rows = torch.from_numpy(_rows(case.obs)).cuda()

        def run(npts, stride, gstride):
            pbuf = torch.empty((npts - 1) * stride + n, dtype=tdt, device="cuda")
            gbuf = torch.empty((npts - 1) * gstride + n + 1, dtype=tdt, device="cuda")
            pts = pbuf.as_strided((npts, n), (stride, 1))
            grad = gbuf.as_strided((npts, n), (gstride, 1))
            pts.copy_(rows[:npts])
            grad.fill_(SENTINEL)
            gbuf[-1] = SENTINEL  # the element behind the last row's last component
            out, _ = it.eval_points_grad_tensors(pts, None, grad)
            it.finish()
            _assert_same(out.cpu().numpy(), want_out[:npts], (npts, stride, gstride, "out"))
            _assert_same(grad.cpu().numpy(), want_grad[:npts], (npts, stride, gstride, "grad"))
            assert float(gbuf[-1]) == SENTINEL
            return it.last_points_path(), it.kernel_name()

        for stride, gstride, fused in ((limit, limit, True), (limit + 1, n, False), (n, limit + 1, False), (limit + 1, limit + 1, False)):
            path, name = run(2, stride, gstride)
            assert path == ("fused" if fused else "split"), (stride, gstride, path)
            assert name.startswith(FUSED["linear"]) == fused, name
        path, name = run(513, limit, limit)
        assert path == "fused" and name.startswith(FUSED["linear"]), (path, name)
        # a forced fused path has no kernel for longer rows
        it.set_option("points_path", 1)
        pbuf = torch.zeros(limit + 1 + n, dtype=tdt, device="cuda")
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            it.eval_points_grad_tensors(pbuf.as_strided((2, n), (limit + 1, 1)))
    finally:
        it.close()
