"""Point-major field sets on the GPU: (n, N) points in, (n, K) values out.  Every result is compared BIT FOR BIT with the
oracle run on each field alone (`tests.helpers.run_oracle`, as tests/test_fields_gpu.py builds its rows), transposed: on the
fused path (interpn::k_linear_fields_points), on the split path (k_split_points, the column form, k_join_fields), in the
device and the host form.

Wall time of the whole file on one MI355X: 3.0 s (81 cases; `pytest -m gpu tests/test_fields_points_gpu.py`).
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

KERNEL = "interpn::k_linear_fields_points<"
SHAPES = {2: [37, 53], 3: [17, 12, 23]}
COUNTS = [1, 63, 64, 65, 255, 256, 257, 3000]  # ragged waves and workgroups
KT = 8  # fields of the fused kernel's result tile
KS = [1, 2, 3, 4, 5, 8, 9, KT, KT + 1]
PER_FIELD_ONLY = [("cubic", [9, 11], False), ("cubic", [9, 11], True), ("cubic", [7, 9, 8], False), ("cubic", [7, 9, 8], True),
                  ("nearest", [9, 7, 11], False), ("linear", [301], False), ("linear", [5, 4, 6, 7], False),
                  ("linear", [3, 2, 4, 3, 2, 3, 4], False)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (ctx, len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


def _fields_case(method, kind, shape, dtype, k, seed, nobs=3000, linearize=False):
    case = synthetic_case(method, kind, len(shape), shape, nobs, seed, dtype=dtype, linearize=linearize)
    rng = np.random.default_rng(1000 + seed)
    fields = np.stack([rng.uniform(-1.0, 1.0, case.vals.size).astype(dtype) for _ in range(k)])
    return case, fields


def _want(oracle, case, fields, fma=True, obs=None):
    """(n, K): the per-field oracle rows of tests/test_fields_gpu.py::_want, transposed."""
    obs = case.obs if obs is None else obs
    rows = []
    for f in range(fields.shape[0]):
        c = dataclasses.replace(case, vals=fields[f], obs=obs)
        rows.append(run_oracle(oracle, c, fma=fma, out=np.zeros(obs[0].size, dtype=fields.dtype)))
    return np.ascontiguousarray(np.stack(rows).T)


def _make(case, fields, fma=None):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Fields.regular(case.method, case.dims, case.starts, case.steps, fields,
                                          linearize_extrapolation=case.linearize, dtype=fields.dtype, fma=fma)
    return interpn_amd.Fields.rectilinear(case.method, case.grids, fields, linearize_extrapolation=case.linearize,
                                          dtype=fields.dtype, fma=fma)


def _rows(obs, n=None):
    return np.ascontiguousarray(np.stack([o[:n] for o in obs], axis=1))


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _device(fs, pts, **kw):
    out = fs.eval_points_tensors(_cuda(pts) if isinstance(pts, np.ndarray) else pts, **kw)
    fs.finish()
    return out.cpu().numpy()


def _columns(fs, obs, n=None):
    """What the column form gives on the same points, transposed."""
    got = fs.eval_tensors([_cuda(o[:n]) for o in obs])
    fs.finish()
    return np.ascontiguousarray(got.cpu().numpy().T)


# ---- 1. the fused path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_fused_path_every_instantiation(oracle, kind, n, dtype, fma):
    tname = "double" if dtype == np.float64 else "float"
    for k in sorted(set(KS)):
        case, fields = _fields_case("linear", kind, SHAPES[n], dtype, k, seed=7 * n + k)
        want = _want(oracle, case, fields, fma)  # once: the points are independent, a prefix's rows are the rows' prefix
        fs = _make(case, fields, fma)
        try:
            assert fs.get_option("fused_table_bytes") > 0 and fs.get_option("points_path") == -1
            fs.set_option("points_path", 1)
            cols = _columns(fs, case.obs)
            fs.set_option("fused", 1)
            cols_fused = _columns(fs, case.obs)
            fs.set_option("fused", -1)
            for count in COUNTS:
                pts = _rows(case.obs, count)
                dev = _device(fs, pts)
                assert fs.last_points_path == "fused" and fs.get_option("last_points_path") == 0
                name = fs.kernel_name()
                assert name == f"{KERNEL}{tname}, {n}, {'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>", name
                _assert_same(dev, want[:count], ("device", kind, n, k, count))
                host = fs.eval_points_host(pts)
                assert fs.last_points_path == "fused"
                _assert_same(host, want[:count], ("host", kind, n, k, count))
                assert dev.tobytes() == cols[:count].tobytes() == cols_fused[:count].tobytes()
        finally:
            fs.close()


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("shape", [[2, 2], [2, 2, 2]], ids=str)
def test_axes_of_exactly_two_points(oracle, shape, kind):
    for dtype in (np.float64, np.float32):
        case, fields = _fields_case("linear", kind, shape, dtype, 5, seed=sum(shape), nobs=1500)
        want = _want(oracle, case, fields)
        fs = _make(case, fields)
        try:
            pts = _rows(case.obs)
            _assert_same(_device(fs, pts), want, ("device", shape, dtype))
            assert fs.last_points_path == "fused"
            _assert_same(fs.eval_points_host(pts), want, ("host", shape, dtype))
        finally:
            fs.close()


# ---- 2. load and store forms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("kind,n,dtype,k", [("regular", 3, np.float64, 3), ("rectilinear", 2, np.float32, 5),
                                            ("regular", 2, np.float64, 9), ("rectilinear", 3, np.float32, 4)])
def test_load_and_store_forms(oracle, kind, n, dtype, k, path):
    import torch

    count = 1000  # 15 whole waves and a ragged one
    case, fields = _fields_case("linear", kind, SHAPES[n], dtype, k, seed=3 * n + k, nobs=count)
    want = _want(oracle, case, fields)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    sent_in, sent_out = 4321.5, -12345.5
    fs = _make(case, fields)
    try:
        fs.set_option("points_path", 1 if path == "fused" else 2)
        fs.set_option("points_slice", 256)
        rows = _rows(case.obs)
        # loads: (row stride, base offset in elements)
        for stride, off in ((n, 0), (n, 1), (n + 1, 0), (40, 0)):
            buf = np.full(off + count * stride + 3, sent_in, dtype=dtype)
            view = buf[off:off + count * stride].reshape(count, stride)
            view[:, :n] = rows
            keep = buf.copy()
            tbuf = _cuda(buf)
            tview = tbuf[off:off + count * stride].view(count, stride)[:, :n]
            assert tview.data_ptr() == tbuf.data_ptr() + off * buf.itemsize and (count == 1 or tview.stride(0) == stride)
            _assert_same(_device(fs, tview), want, ("device load", stride, off))
            assert fs.last_points_path == path
            _assert_same(tbuf.cpu().numpy(), keep, ("device load: the block is only read", stride, off))
            _assert_same(fs.eval_points_host(view[:, :n]), want, ("host load", stride, off))
            _assert_same(buf, keep, ("host load: the block is only read", stride, off))
        # stores: row stride of out
        pts = _cuda(rows)
        for ostride in (k, k + 1, 40):
            if ostride < k:
                continue
            tout = torch.full((count * ostride + 5,), sent_out, dtype=tdt, device="cuda:0")
            oview = tout[2:2 + count * ostride].view(count, ostride)[:, :k]
            fs.eval_points_tensors(pts, oview)
            fs.finish()
            got = tout.cpu().numpy()
            block = got[2:2 + count * ostride].reshape(count, ostride)
            _assert_same(block[:, :k], want, ("device store", ostride))
            assert np.all(block[:, k:] == sent_out) and np.all(got[:2] == sent_out) and np.all(got[2 + count * ostride:] == sent_out), ostride
            hout = np.full((count, ostride), sent_out, dtype=dtype)
            fs.eval_points_host(rows, hout[:, :k])
            _assert_same(hout[:, :k], want, ("host store", ostride))
            assert np.all(hout[:, k:] == sent_out), ostride
    finally:
        fs.close()


# ---- 3. the split path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,shape,linearize", PER_FIELD_ONLY,
                         ids=[f"{m}-N{len(s)}-{'lin' if l else 'nolin'}" for m, s, l in PER_FIELD_ONLY])
def test_split_path_methods_without_a_fused_form(oracle, method, shape, linearize, kind):
    case, fields = _fields_case(method, kind, shape, np.float64, 3, seed=40 + len(shape), nobs=700, linearize=linearize)
    want = _want(oracle, case, fields)
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused_table_bytes") == 0
        fs.set_option("points_slice", 256)  # slices of 256, 256 and a ragged 188
        pts = _rows(case.obs)
        _assert_same(_device(fs, pts), want, ("device", method, shape))
        assert fs.last_points_path == "split" and fs.last_path == "per_field" and not fs.kernel_name().startswith(KERNEL)
        fs.set_option("host_chunk", 300)
        _assert_same(fs.eval_points_host(pts), want, ("host", method, shape))
        assert fs.last_points_path == "split"
        for count in (1, 255, 256, 257):
            _assert_same(_device(fs, pts[:count]), want[:count], ("device", method, shape, count))
    finally:
        fs.close()


@pytest.mark.parametrize("kind,n,dtype,k", [("regular", 3, np.float64, 3), ("rectilinear", 2, np.float32, 9),
                                            ("rectilinear", 3, np.float32, 20), ("regular", 2, np.float64, 2)])
def test_split_path_on_a_fusable_set(oracle, kind, n, dtype, k):
    case, fields = _fields_case("linear", kind, SHAPES[n], dtype, k, seed=5 * n + k)
    want = _want(oracle, case, fields)
    fs = _make(case, fields)
    try:
        pts = _rows(case.obs)
        fused = _device(fs, pts)
        assert fs.last_points_path == "fused"
        _assert_same(fused, want, "fused")
        fs.set_option("points_slice", 256)
        fs.set_option("points_path", 2)
        fs.set_option("fused", 1)  # the slices' column evaluation: k_linear_fields
        got = _device(fs, pts)
        assert fs.last_points_path == "split" and fs.last_path == "fused"
        assert got.tobytes() == fused.tobytes()
        fs.set_option("fused", 0)  # ... and per field
        got = _device(fs, pts)
        assert fs.last_points_path == "split" and fs.last_path == "per_field"
        assert got.tobytes() == fused.tobytes()
        assert fs.eval_points_host(pts).tobytes() == fused.tobytes()
        fs.set_option("points_path", -1)  # fused = 0 turns the set's fused kernels off: split
        got = _device(fs, pts)
        assert fs.last_points_path == "split" and got.tobytes() == fused.tobytes()
        for count in COUNTS:
            _assert_same(_device(fs, pts[:count]), want[:count], ("split", count))
    finally:
        fs.close()


# ---- 4. failing points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "split_fused", "split_per_field"])
@pytest.mark.parametrize("bad", [0, 37 + 64, 300], ids=["first", "mid_wave", "second_slice"])
@pytest.mark.parametrize("value", [np.nan, 1e300], ids=["nan", "huge"])
def test_failing_point_contract(oracle, bad, mode, value):
    """A coordinate a regular grid cannot place (what tests/test_points_gpu.py uses): the device form reports the index in the
    whole call — also from the second slice of the split path, where every handle of the per-field path counts from the
    slice's start — and the host form writes exactly the rows in front of it."""
    k, count = 3, 700
    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, k, seed=11, nobs=count)
    case.obs[1][bad] = value
    case.obs[2][bad + 300] = np.inf  # a later failure (another slice, another chunk) must not be the one reported
    want = _want(oracle, case, fields, obs=[o[:bad] for o in case.obs]) if bad else np.zeros((0, k))
    fs = _make(case, fields)
    try:
        fs.set_option("points_slice", 256)
        fs.set_option("points_path", 1 if mode == "fused" else 2)
        fs.set_option("fused", 0 if mode == "split_per_field" else 1)
        pts = _rows(case.obs)
        fs.eval_points_tensors(_cuda(pts))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as err:
            fs.finish()
        assert err.value.first_bad_index == bad
        assert fs.last_points_path == ("fused" if mode == "fused" else "split")
        assert fs.last_path == ("per_field" if mode == "split_per_field" else "fused")
        for chunk in (0, 250):  # one chunk, and chunks that end in front of / behind the failing point
            fs.set_option("host_chunk", chunk)
            sentinel = 777.25
            out = np.full((count, k + 2), sentinel)  # two guard columns behind every row
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
                fs.eval_points_host(pts, out[:, :k])
            _assert_same(out[:bad, :k], want, ("host head", chunk))
            assert np.all(out[bad:] == sentinel) and np.all(out[:, k:] == sentinel), chunk
        # the status words are clear again: a clean batch afterwards is clean
        _assert_same(_device(fs, pts[:bad]), want, "clean again")
    finally:
        fs.close()


@pytest.mark.parametrize("path", [1, 2], ids=["fused", "split"])
def test_nan_and_inf_propagate_as_in_the_column_form(path):
    """A rectilinear grid places every coordinate: NaN and +-inf give what the column form gives, bit for bit."""
    case, fields = _fields_case("linear", "rectilinear", SHAPES[3], np.float64, 3, seed=13, nobs=600)
    case.obs[0][5] = np.nan
    case.obs[1][300] = np.inf
    case.obs[2][599] = -np.inf
    fs = _make(case, fields)
    try:
        want = _columns(fs, case.obs)
        assert np.isnan(want[5]).all()
        fs.set_option("points_path", path)
        fs.set_option("points_slice", 256)
        assert _device(fs, _rows(case.obs)).tobytes() == want.tobytes()
        assert fs.eval_points_host(_rows(case.obs)).tobytes() == want.tobytes()
    finally:
        fs.close()


# ---- 5. capture and allocation --------------------------------------------------------------------------------------------
def test_no_alloc_and_reserved_scratch(oracle):
    from interpn_amd._lib import InterpnHipError

    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, 3, seed=17, nobs=700)
    want = _want(oracle, case, fields)
    pts = _cuda(_rows(case.obs))
    fs = _make(case, fields)
    try:
        _assert_same(_device(fs, pts, no_alloc=True), want, "fused: nothing reserved, nothing needed")
        assert fs.last_points_path == "fused"
        fs.set_option("points_path", 2)
        with pytest.raises(InterpnHipError, match="[Oo]ut of memory|memory"):
            fs.eval_points_tensors(pts, no_alloc=True)
        fs.reserve_points(700)
        _assert_same(_device(fs, pts, no_alloc=True), want, "split: reserved")
        assert fs.last_points_path == "split"
    finally:
        fs.close()


def test_graph_capture_and_side_stream(oracle):
    import torch

    count = 5001
    case, fields = _fields_case("linear", "rectilinear", SHAPES[3], np.float64, 5, seed=21, nobs=count)
    want = _want(oracle, case, fields)
    fs = _make(case, fields)
    try:
        pts = _cuda(_rows(case.obs))
        out = torch.zeros((count, 5), dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            fs.eval_points_tensors(pts, out)  # torch's current stream is the side stream
        fs.finish()
        assert fs.last_points_path == "fused"
        _assert_same(out.cpu().numpy(), want, "side stream")
        out.zero_()
        torch.cuda.synchronize()
        fs.eval_points_tensors(pts, out, stream=side)  # the stream given explicitly
        fs.finish(side)
        _assert_same(out.cpu().numpy(), want, "stream=")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fs.eval_points_tensors(pts, out)  # one kernel, no parallel branches
        assert fs.last_points_path == "fused"
        rng = np.random.default_rng(77)
        for rep in range(2):
            host = [rng.uniform(-1.1, 1.1, count) for _ in range(3)]
            pts.copy_(torch.from_numpy(_rows(host)))
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            _assert_same(out.cpu().numpy(), _want(oracle, case, fields, obs=host), ("replay", rep))
        fs.finish()
    finally:
        fs.close()


# ---- 6. entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,n", [("linear", 2), ("linear", 3), ("cubic", 2)])
def test_interpn_fields_points(oracle, method, n):
    import torch

    import interpn_amd

    k = 3
    case, fields = _fields_case(method, "regular", SHAPES[n], np.float64, k, seed=9 + n, nobs=35, linearize=True)
    want = _want(oracle, case, fields).reshape(5, 7, k)
    xi = _rows(case.obs).reshape(5, 7, n)
    vals_last = np.ascontiguousarray(np.moveaxis(fields.reshape(k, *SHAPES[n]), 0, -1))  # scipy's (*dims, K)
    got = interpn_amd.interpn_fields_points(xi, case.grids, vals_last, method=method, assume_regular=True)
    assert got.shape == (5, 7, k)
    _assert_same(got, want, "numpy")
    out = np.zeros((5, 7, k))
    assert interpn_amd.interpn_fields_points(xi, case.grids, vals_last, method=method, out=out, assume_regular=True) is out
    _assert_same(out, want, "numpy, out=")
    tgot = interpn_amd.interpn_fields_points(_cuda(xi), case.grids, _cuda(vals_last), method=method, assume_regular=True)
    assert tuple(tgot.shape) == (5, 7, k) and tgot.is_cuda
    _assert_same(tgot.cpu().numpy(), want, "tensors")
    tout = torch.zeros((5, 7, k), dtype=torch.float64, device="cuda:0")
    assert interpn_amd.interpn_fields_points(_cuda(xi), case.grids, vals_last, method=method, out=tout, assume_regular=True) is tout
    _assert_same(tout.cpu().numpy(), want, "tensors, out=")
    inside = np.clip(xi, -1.0, 1.0)
    interpn_amd.interpn_fields_points(inside, case.grids, vals_last, method=method, check_bounds=True, assume_regular=True)
    with pytest.raises(ValueError, match="violate interpolator bounds"):
        interpn_amd.interpn_fields_points(_cuda(xi), case.grids, vals_last, method=method, check_bounds=True, assume_regular=True)


def test_eval_points_dispatch_and_argument_errors(oracle):
    import torch

    k = 3
    case, fields = _fields_case("linear", "regular", SHAPES[2], np.float64, k, seed=4, nobs=35)
    want = _want(oracle, case, fields)
    fs = _make(case, fields)
    try:
        pts = _rows(case.obs)
        _assert_same(fs.eval_points(pts), want, "numpy")
        got = fs.eval_points(_cuda(pts), no_alloc=True)
        fs.finish()
        _assert_same(got.cpu().numpy(), want, "tensor")
        _assert_same(fs.eval_points(pts.reshape(5, 7, 2)).reshape(35, k), want, "(..., N)")
        fort = np.asfortranarray(pts)  # neither contiguous nor unit-stride rows: copied once
        _assert_same(fs.eval_points(fort), want, "copied")
        assert fs.eval_points(np.zeros((0, 2))).shape == (0, k)
        with pytest.raises(TypeError, match="no_alloc"):
            fs.eval_points(pts, no_alloc=True)
        with pytest.raises(ValueError, match=r"expected shape \(\.\.\., 2\)"):
            fs.eval_points(np.zeros((35, 3)))
        with pytest.raises(ValueError, match=r"expected shape \(\.\.\., 2\)"):
            fs.eval_points(torch.zeros((35, 3), dtype=torch.float64, device="cuda:0"))
        with pytest.raises(TypeError, match="expected dtype float64"):
            fs.eval_points(pts.astype(np.float32))
        with pytest.raises(TypeError, match="torch.float64"):
            fs.eval_points(_cuda(pts.astype(np.float32)))
        with pytest.raises(ValueError, match="every row must be contiguous"):
            fs.eval_points(pts, np.zeros((35, 2 * k))[:, ::2])
        with pytest.raises(ValueError, match="every row must be contiguous"):
            fs.eval_points(_cuda(pts), torch.zeros((35, 2 * k), dtype=torch.float64, device="cuda:0")[:, ::2])
        with pytest.raises(ValueError, match="out: expected shape"):
            fs.eval_points(pts, np.zeros((35, k - 1)))
        with pytest.raises(ValueError, match="row stride"):
            fs.eval_points(pts, np.zeros((1, 35 * k)).reshape(35, k)[::-1])
        lib_st = fs.get_option("last_points_path")
        assert lib_st == 0
        # the library's own checks, in their order
        from interpn_amd import _lib
        from ctypes import c_void_p

        lib = _lib.load()
        buf = torch.zeros(64, dtype=torch.float64, device="cuda:0")
        p = c_void_p(buf.data_ptr())
        dev = lambda *a: lib.interpn_hip_fields_eval_points_device(fs._h, *a)
        assert dev(p, 1, 4, p, k, None, 0, None) == 32       # point_stride < ndims
        assert dev(p, 2, 4, p, k - 1, None, 0, None) == 32   # out_stride < nfields
        assert dev(None, 1, 0, None, 0, None, 0, None) == 32  # ... in front of npoints == 0
        assert dev(None, 2, 0, None, k, None, 0, None) == 0  # npoints == 0: OK whatever the pointers are
        assert dev(None, 2, 4, p, k, None, 0, None) == 32 and dev(p, 2, 4, None, k, None, 0, None) == 32
        assert dev(p, 2**61, 8, p, k, None, 0, None) == 32 and dev(p, 2, 8, p, 2**61, None, 0, None) == 32  # byte sizes overflow
        assert dev(p, 2, 4, p, k, None, 2, None) == 32       # unknown flag
        assert lib.interpn_hip_fields_eval_points_host(fs._h, None, 1, 0, None, 0) == 32
        assert lib.interpn_hip_fields_eval_points_host(fs._h, None, 2, 0, None, k) == 0
        assert lib.interpn_hip_fields_reserve_points(fs._h, 100, -1) == 32
        with pytest.raises(ValueError):
            fs.set_option("points_path", 0)
    finally:
        fs.close()


# ---- 7. the automatic rule ------------------------------------------------------------------------------------------------
AUTO = [  # shape, dtype, K, points: the classes of the column form's rule (tests/test_fields_gpu.py::AUTO) on both sides of its
    # batch thresholds; the point-major rule takes the fused kernel in all of them
    ([64, 64, 64], np.float64, 4, 20_000_000),  # column form: per field (sweep kernel)
    ([64, 64, 64], np.float64, 4, 100_000),     # ... below the sweep kernel's batch size
    ([64, 64, 64], np.float32, 2, 1_000_000),   # column form: per field (half-empty lines)
    ([300, 200], np.float64, 1, 1000),          # ... a quarter-full line
    ([300, 200], np.float64, 4, 1_000_000),     # column form: fused
    ([40, 30, 20], np.float64, 3, 64),
]


@pytest.mark.parametrize("shape,dtype,k,npts", AUTO, ids=[f"{'x'.join(map(str, a[0]))}-{np.dtype(a[1]).name}-K{a[2]}-{a[3]}" for a in AUTO])
def test_automatic_path_with_the_table(shape, dtype, k, npts):
    import torch

    case, fields = _fields_case("linear", "regular", shape, dtype, k, seed=k, nobs=64)
    fs = _make(case, fields)
    try:
        assert fs.get_option("points_path") == -1 and fs.get_option("fused") == -1
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(npts % 1000 + k)
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        pts = torch.rand((npts, len(shape)), dtype=tdt, device="cuda:0", generator=gen) * 2.1 - 1.05
        got = fs.eval_points_tensors(pts)
        fs.finish()
        assert fs.last_points_path == "fused" and fs.kernel_name().startswith(KERNEL), (fs.last_points_path, fs.kernel_name())
        fs.set_option("points_path", 2)
        other = fs.eval_points_tensors(pts)
        fs.finish()
        assert fs.last_points_path == "split"
        view = torch.int64 if dtype == np.float64 else torch.int32
        assert torch.equal(got.view(view), other.view(view))
    finally:
        fs.close()


def test_automatic_path_without_the_table_and_forced_paths(oracle, monkeypatch):
    from interpn_amd._lib import InterpnHipError

    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, 4, seed=2, nobs=300)
    want = _want(oracle, case, fields)
    pts = _rows(case.obs)
    fs = _make(case, fields)
    try:
        fs.set_option("fused", 0)  # the set's fused kernels are off
        _assert_same(_device(fs, pts), want, "fused = 0")
        assert fs.last_points_path == "split"
        fs.set_option("points_path", 1)  # "wherever the table exists" overrides it
        _assert_same(_device(fs, pts), want, "points_path = 1")
        assert fs.last_points_path == "fused"
    finally:
        fs.close()
    monkeypatch.setenv("INTERPN_HIP_FIELDS_TABLE_BUDGET", "1")  # a set the memory rule left without the table
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused_table_bytes") == 0
        _assert_same(_device(fs, pts), want, "no table")
        assert fs.last_points_path == "split"
        fs.set_option("points_path", 1)
        with pytest.raises(InterpnHipError):
            fs.eval_points_tensors(_cuda(pts))
        with pytest.raises(InterpnHipError):
            fs.eval_points_host(pts)
    finally:
        fs.close()
