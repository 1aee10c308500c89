"""Gradients of a field set on the GPU (interpn_hip_fields_eval_grad_*, Fields.eval_grad_*, interpn_fields_grad,
interpn_amd.autograd.interp_fields): K values and their K x N Jacobian in one call.

The definition is by reference to what exists: value row f is `Fields.eval_*`'s, gradient block f is the single handle's
`eval_grad_*` (multicubic: `eval_cubic_grad_*`) of field f.  Every comparison against those is on bit patterns — NaN
payloads and signed zeros count — and nothing has a tolerance.  The numpy restatements (tests/grad_restatement.py,
tests/cubic_grad_restatement.py) are compared bit for bit too, except that a NaN need only be a NaN on both sides (numpy's
NaN payloads are not the device's)."""

import dataclasses
import functools
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest

from tests import cubic_grad_restatement as cgr
from tests import grad_restatement as gr
from tests.helpers import synthetic_case

pytestmark = pytest.mark.gpu

OK, DIM_MISMATCH, INVALID, UNSUPPORTED = 0, 1, 32, 33
FUSED_KERNEL = "interpn::k_linear_fields_grad<"
SHAPES = {2: [9, 8], 3: [7, 6, 5]}
KMAX = 9
PER_LINE = {(8, 3): 2, (8, 2): 4, (4, 3): 4, (4, 2): 8}  # (element size, N) -> P, fields per table line


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_FIELDS_FUSED", "INTERPN_HIP_FIELDS_TABLE_BUDGET", "INTERPN_HIP_BRICKS", "INTERPN_HIP_FORCE_GENERIC"):
        monkeypatch.delenv(name, raising=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_bits(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (ctx, len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


def _assert_restated(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape, got.dtype, want.dtype)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (ctx, int((~same).sum()), np.argwhere(~same)[:5].tolist(), got[~same][:5], want[~same][:5])


def _tdtype(dtype):
    import torch

    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def _tensors(obs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(o)).to("cuda:0") for o in obs]


def _fields_case(method, kind, shape, dtype, k, seed, nobs=3000, linearize=False, extrap=0.3):
    case = synthetic_case(method, kind, len(shape), shape, nobs, seed, dtype=dtype, linearize=linearize, extrap=extrap)
    rng = np.random.default_rng(1000 + seed)
    fields = np.stack([rng.uniform(-1.0, 1.0, case.vals.size).astype(dtype) for _ in range(k)])
    return case, fields


def _make(case, fields, fma=None):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Fields.regular(case.method, case.dims, case.starts, case.steps, fields, linearize_extrapolation=case.linearize,
                                          dtype=fields.dtype, fma=fma)
    return interpn_amd.Fields.rectilinear(case.method, case.grids, fields, linearize_extrapolation=case.linearize, dtype=fields.dtype,
                                          fma=fma)


def _single(case, vals, fma=None):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, vals,
                                                linearize_extrapolation=case.linearize, dtype=vals.dtype, fma=fma)
    return interpn_amd.Interpolator.rectilinear(case.method, case.grids, vals, linearize_extrapolation=case.linearize, dtype=vals.dtype,
                                                fma=fma)


def _single_handles(case, fields, fma=None, obs=None):
    """(out (K, n), grad (K, N, n)) of K single handles, one per field, on the device."""
    obs_t = _tensors(case.obs if obs is None else obs)
    outs, grads = [], []
    for f in range(fields.shape[0]):
        it = _single(case, fields[f], fma)
        try:
            o, g = (it.eval_cubic_grad_tensors if case.method == "cubic" else it.eval_grad_tensors)(obs_t)
            it.finish()
            outs.append(o.cpu().numpy())
            grads.append(g.cpu().numpy())
        finally:
            it.close()
    return np.stack(outs), np.stack(grads)


def _restated(case, fields, fma=True, obs=None):
    """(out (K, n), grad (K, N, n), ok (n,)) of the numpy restatement, field by field."""
    mod = cgr if case.method == "cubic" else gr
    outs, grads, ok = [], [], None
    for f in range(fields.shape[0]):
        c = dataclasses.replace(case, vals=fields[f], obs=case.obs if obs is None else obs)
        o, g, ok = mod.eval_grad_case(c, fma=fma)
        outs.append(o)
        grads.append(g)
    return np.stack(outs), np.stack(grads), ok


def _device(fs, obs, out=None, grad=None, **kw):
    out_t, grad_t = fs.eval_grad_tensors(_tensors(obs), out, grad, **kw)
    fs.finish()
    return out_t.cpu().numpy(), grad_t.cpu().numpy()


def _kernel_name(dtype, n, kind, fma):
    tname = "double" if np.dtype(dtype) == np.float64 else "float"
    return f"{FUSED_KERNEL}{tname}, {n}, {'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>"


@functools.lru_cache(maxsize=None)
def _parity_reference(kind, n, dtype_name, fma):
    """The case of the parity test with KMAX fields, the restatement and the KMAX single handles' results: computed once per
    (kind, N, dtype, flavour); a set of K fields holds the first K."""
    dtype = np.dtype(dtype_name).type
    case, fields = _fields_case("linear", kind, SHAPES[n], dtype, KMAX, seed=31 * n + (kind == "regular") + 2 * fma)
    for d in range(n):  # reaching beyond the grid on every side
        assert case.obs[d].min() < case.grids[d][0] and case.obs[d].max() > case.grids[d][-1]
    r_out, r_grad, ok = _restated(case, fields, fma)
    assert ok.all()
    s_out, s_grad = _single_handles(case, fields, fma)
    return case, fields, r_out, r_grad, s_out, s_grad


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9])
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_parity_of_every_fused_instantiation(kind, n, dtype, fma, k):
    case, fields, r_out, r_grad, s_out, s_grad = _parity_reference(kind, n, np.dtype(dtype).name, fma)
    fs = _make(case, fields[:k], fma)
    try:
        assert fs.get_option("fused_table_bytes") > 0
        values = fs.eval_tensors(_tensors(case.obs))
        fs.finish()
        values = values.cpu().numpy()
        results = {}
        for fused in (1, 0):
            fs.set_option("fused", fused)
            out, grad = _device(fs, case.obs)
            name = fs.kernel_name()
            if fused:
                assert fs.last_path == "fused" and fs.get_option("last_path") == 0
                assert name == _kernel_name(dtype, n, kind, fma), name
            else:
                assert fs.last_path == "per_field" and fs.get_option("last_path") == 1
                assert not name.startswith(FUSED_KERNEL) and "k_linear_grad" in name, name
            ctx = (kind, n, k, "fused" if fused else "per_field")
            assert grad.shape == (k, n, case.obs[0].size)
            _assert_bits(out, values, ("value rows against Fields.eval_tensors",) + ctx)
            _assert_bits(out, s_out[:k], ("value rows against the single handles",) + ctx)
            _assert_bits(grad, s_grad[:k], ("gradient against the single handles",) + ctx)
            _assert_restated(out, r_out[:k], ("value rows against the restatement",) + ctx)
            _assert_restated(grad, r_grad[:k], ("gradient against the restatement",) + ctx)
            hout, hgrad = fs.eval_grad_host(case.obs)
            assert fs.last_path == ("fused" if fused else "per_field")
            _assert_bits(hout, out, ("host values",) + ctx)
            _assert_bits(hgrad, grad, ("host gradient",) + ctx)
            results[fused] = (out, grad)
        assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
    finally:
        fs.close()


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "per_field"])
@pytest.mark.parametrize("kind,n,dtype,k", [("regular", 3, np.float64, 3), ("rectilinear", 2, np.float32, 9),
                                            ("rectilinear", 3, np.float32, 5), ("regular", 2, np.float64, 5)])
def test_batch_sizes_and_guards(kind, n, dtype, k, fused):
    """Views into wider sentinel-filled blocks (row strides beyond n, an odd offset, P spare rows behind the K and K * N
    rows): exactly the first n elements of the K value rows and the K * N component rows change."""
    import torch

    p = PER_LINE[(np.dtype(dtype).itemsize, n)]
    big_case, fields = _fields_case("linear", kind, SHAPES[n], dtype, k, seed=5 * n + k, nobs=1000)
    w_out, w_grad, ok = _restated(big_case, fields)
    assert ok.all()
    fs = _make(big_case, fields)
    try:
        fs.set_option("fused", fused)
        for npts in (1, 63, 64, 65, 255, 256, 257, 1000):
            obs = [o[:npts].copy() for o in big_case.obs]
            pad, off = 24, 3
            sentinel = -12345.5
            width = npts + 2 * pad
            tout = torch.full((k + p, width), sentinel, dtype=_tdtype(dtype), device="cuda:0")
            tgrad = torch.full(((k + p) * n, width), sentinel, dtype=_tdtype(dtype), device="cuda:0")
            gview = tgrad[:k * n].unflatten(0, (k, n))[:, :, off:off + npts]
            fs.eval_grad_tensors(_tensors(obs), tout[:k, off:off + npts], gview)
            fs.finish()
            assert fs.last_path == ("fused" if fused else "per_field")
            got_out, got_grad = tout.cpu().numpy(), tgrad.cpu().numpy()
            _assert_restated(got_out[:k, off:off + npts], w_out[:, :npts], ("device out", npts))
            _assert_restated(got_grad[:k * n, off:off + npts].reshape(k, n, npts), w_grad[:, :, :npts], ("device grad", npts))
            for blk, rows in ((got_out, k), (got_grad, k * n)):
                assert np.all(blk[:, :off] == sentinel) and np.all(blk[:, off + npts:] == sentinel), npts
                assert np.all(blk[rows:] == sentinel), ("rows behind the last field", npts)
            # the host form, the same way
            hout = np.full((k + p, width), sentinel, dtype=dtype)
            hgrad = np.full(((k + p) * n, width), sentinel, dtype=dtype)
            fs.eval_grad_host(obs, hout[:k, pad:pad + npts], hgrad[:k * n].reshape(k, n, width)[:, :, pad:pad + npts])
            _assert_bits(hout[:k, pad:pad + npts], got_out[:k, off:off + npts], ("host out", npts))
            _assert_bits(hgrad[:k * n, pad:pad + npts], got_grad[:k * n, off:off + npts], ("host grad", npts))
            for blk, rows in ((hout, k), (hgrad, k * n)):
                assert np.all(blk[:, :pad] == sentinel) and np.all(blk[:, pad + npts:] == sentinel) and np.all(blk[rows:] == sentinel)
    finally:
        fs.close()


def _check_fused_against_restatement(case, fields, ctx, fma=True):
    w_out, w_grad, ok = _restated(case, fields, fma)
    assert ok.all()
    fs = _make(case, fields, fma)
    try:
        fs.set_option("fused", 1)
        values = fs.eval_tensors(_tensors(case.obs))
        out, grad = _device(fs, case.obs)
        assert fs.last_path == "fused" and fs.kernel_name().startswith(FUSED_KERNEL), ctx
        _assert_bits(out, values.cpu().numpy(), ("values", ctx))
        _assert_restated(out, w_out, ("out", ctx))
        _assert_restated(grad, w_grad, ("grad", ctx))
        fs.set_option("fused", 0)
        out0, grad0 = _device(fs, case.obs)
        assert fs.last_path == "per_field"
        _assert_bits(out, out0, ("per-field out", ctx))
        _assert_bits(grad, grad0, ("per-field grad", ctx))
    finally:
        fs.close()


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("shape", [[2, 2], [2, 9], [9, 2], [2, 9, 2], [7, 2, 5], [2, 2, 2]], ids=str)
def test_axes_of_exactly_two_points(shape, kind):
    for dtype in (np.float64, np.float32):
        case, fields = _fields_case("linear", kind, shape, dtype, 5, seed=sum(shape), nobs=1500)
        _check_fused_against_restatement(case, fields, (shape, kind, np.dtype(dtype).name))


def _clustered_axis(length, rng, dtype):
    """[-1, 1] in `length` knots whose cell widths alternate at random between wide and a twentieth of it."""
    w = rng.choice([1.0, 0.05], length - 1)
    g = -1.0 + 2.0 * np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
    g[0], g[-1] = -1.0, 1.0
    g = g.astype(dtype)
    assert np.all(np.diff(g) > 0)
    return g


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("length", [5, 64, 65, 3000])
def test_rectilinear_axis_lengths(length, dtype):
    """Axes inside the LDS image and beyond it, clustered knots: the divisor is the cell's own x1 - x0."""
    for shape in ([length, 9], [4, 5, length]):
        case, fields = _fields_case("linear", "rectilinear", shape, dtype, 3, seed=length % 89 + len(shape), nobs=3000)
        rng = np.random.default_rng(length)
        case = dataclasses.replace(case, grids=[_clustered_axis(m, rng, dtype) for m in shape])
        _check_fused_against_restatement(case, fields, (shape, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
def test_non_finite_nodes_and_nan_coordinates(n, dtype):
    k = 5
    case, fields = _fields_case("linear", "rectilinear", SHAPES[n], dtype, k, seed=53 + n, nobs=1500)
    rng = np.random.default_rng(99 + n)
    for v in (np.nan, np.inf, -np.inf, -0.0):
        for f in range(k):
            fields[f][rng.integers(0, fields[f].size, 4)] = v
    for d in range(n):
        for v in (np.nan, np.inf, -np.inf):
            case.obs[d][rng.integers(100, 1500, 4)] = v
    s_out, s_grad = _single_handles(case, fields)
    r_out, r_grad, _ok = _restated(case, fields)
    assert np.isnan(s_grad).any() and np.isinf(s_grad).any()
    fs = _make(case, fields)
    try:
        for fused in (1, 0):
            fs.set_option("fused", fused)
            out, grad = _device(fs, case.obs)
            assert fs.last_path == ("fused" if fused else "per_field")
            _assert_bits(out, s_out, ("out", fused))
            _assert_bits(grad, s_grad, ("grad", fused))
            _assert_restated(out, r_out, ("out restated", fused))
            _assert_restated(grad, r_grad, ("grad restated", fused))
    finally:
        fs.close()


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "per_field"])
@pytest.mark.parametrize("dtype,n", [(np.float64, 3), (np.float32, 2), (np.float32, 3), (np.float64, 2)])
def test_failing_point_contract(dtype, n, fused):
    npts, bad, k = 3000, 1500, 3
    case, fields = _fields_case("linear", "regular", SHAPES[n], dtype, k, seed=11 + n, nobs=npts)
    w_out, w_grad, _ = _restated(case, fields)
    case.obs[n - 1][bad] = 1e300 if dtype == np.float64 else 3e38
    case.obs[0][bad + 700] = np.nan  # a later failure must not be the one reported
    _, _, ok = _restated(case, fields[:1])
    assert int(np.argmin(ok)) == bad and not ok[bad]
    fs = _make(case, fields)
    try:
        fs.set_option("fused", fused)
        fs.eval_grad_tensors(_tensors(case.obs))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as err:
            fs.finish()
        assert err.value.first_bad_index == bad
        assert fs.last_path == ("fused" if fused else "per_field")
        fs.set_option("host_chunk", 1000)  # three chunks, the failing point in the second
        sentinel = dtype(777.25)
        out = np.full((k, npts), sentinel, dtype=dtype)
        grad = np.full((k, n, npts), sentinel, dtype=dtype)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
            fs.eval_grad_host(case.obs, out, grad)
        _assert_restated(out[:, :bad], w_out[:, :bad], "host out in front")
        _assert_restated(grad[:, :, :bad], w_grad[:, :, :bad], "host grad in front")
        assert np.all(out[:, bad:] == sentinel) and np.all(grad[:, :, bad:] == sentinel)
        # the status word is cleared: a clean batch afterwards is clean
        _device(fs, [o[:bad] for o in case.obs])
    finally:
        fs.close()


@pytest.mark.parametrize("shape", [[301], [5, 4, 6, 7]], ids=str)
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_per_field_multilinear_other_dimensions(kind, shape):
    case, fields = _fields_case("linear", kind, shape, np.float64, 3, seed=len(shape), nobs=1200)
    r_out, r_grad, ok = _restated(case, fields)
    assert ok.all()
    s_out, s_grad = _single_handles(case, fields)
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused_table_bytes") == 0
        fs.set_option("fused", 1)  # wherever the table exists: not here
        out, grad = _device(fs, case.obs)
        assert fs.last_path == "per_field" and "k_linear_grad_n<" in fs.kernel_name()
        _assert_bits(out, s_out, "out")
        _assert_bits(grad, s_grad, "grad")
        _assert_restated(out, r_out, "out restated")
        _assert_restated(grad, r_grad, "grad restated")
        hout, hgrad = fs.eval_grad_host(case.obs)
        _assert_bits(hout, out, "host out")
        _assert_bits(hgrad, grad, "host grad")
    finally:
        fs.close()


@pytest.mark.parametrize("linearize", [False, True], ids=["hold", "linearize"])
@pytest.mark.parametrize("shape", [[9, 11], [7, 9, 8]], ids=str)
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_per_field_multicubic(kind, shape, linearize):
    case, fields = _fields_case("cubic", kind, shape, np.float64, 3, seed=7 + len(shape), nobs=1200, linearize=linearize)
    r_out, r_grad, ok = _restated(case, fields)
    assert ok.all()
    s_out, s_grad = _single_handles(case, fields)
    fs = _make(case, fields)
    try:
        out, grad = _device(fs, case.obs)
        assert fs.last_path == "per_field" and "cubic" in fs.kernel_name()
        _assert_bits(out, s_out, "out")
        _assert_bits(grad, s_grad, "grad")
        _assert_restated(out, r_out, "out restated")
        _assert_restated(grad, r_grad, "grad restated")
        values = fs.eval_tensors(_tensors(case.obs))
        fs.finish()
        _assert_bits(out, values.cpu().numpy(), "values")
        hout, hgrad = fs.eval_grad_host(case.obs)
        _assert_bits(hout, out, "host out")
        _assert_bits(hgrad, grad, "host grad")
    finally:
        fs.close()


def test_nearest_sets_are_unsupported():
    import interpn_amd
    from interpn_amd import _lib

    lib = _lib.load()
    case, fields = _fields_case("nearest", "regular", SHAPES[2], np.float64, 2, seed=3, nobs=64)
    n = 64
    out, grad = np.zeros((2, n)), np.zeros((2, 2, n))
    fs = _make(case, fields)
    try:
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            fs.eval_grad_host(case.obs, out, grad)
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            fs.eval_grad(case.obs)
        vp = (c_void_p * 2)(*[o.ctypes.data for o in case.obs])
        lens = (c_size_t * 2)(n, n)
        path = c_int(-1)
        # before any device work: the (host) pointers are never dereferenced
        assert lib.interpn_hip_fields_eval_grad_device(fs._h, vp, 2, c_void_p(out.ctypes.data), n, c_void_p(grad.ctypes.data), n, n, None, 0,
                                                       path) == UNSUPPORTED
        assert lib.interpn_hip_fields_eval_grad_host(fs._h, vp, lens, 2, c_void_p(out.ctypes.data), n, c_void_p(grad.ctypes.data), n,
                                                     n) == UNSUPPORTED
        assert not out.any() and not grad.any()
    finally:
        fs.close()
    vals = fields.reshape(2, *SHAPES[2])
    with pytest.raises(_lib.InterpnHipError, match="unsupported"):
        interpn_amd.interpn_fields_grad(case.obs, case.grids, vals, method="nearest")


def test_set_refused_its_table(monkeypatch):
    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, 4, seed=2, nobs=1200)
    s_out, s_grad = _single_handles(case, fields)
    monkeypatch.setenv("INTERPN_HIP_FIELDS_TABLE_BUDGET", "0")
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused_table_bytes") == 0
        fs.set_option("fused", 1)
        out, grad = _device(fs, case.obs)
        assert fs.last_path == "per_field" and not fs.kernel_name().startswith(FUSED_KERNEL)
        _assert_bits(out, s_out, "out")
        _assert_bits(grad, s_grad, "grad")
    finally:
        fs.close()


def test_side_stream_and_graph_capture():
    """A fused evaluation on a side stream (torch's current stream, and given explicitly), and one captured into a graph
    (one kernel on the capture stream: a linear chain, no parallel branches) and replayed twice on new coordinates in the
    same buffers: the bits of an eager call."""
    import torch

    npts, n, k = 5001, 3, 5
    case, fields = _fields_case("linear", "rectilinear", SHAPES[n], np.float64, k, seed=21, nobs=npts)
    fs = _make(case, fields)
    try:
        fs.set_option("fused", 1)
        eager_out, eager_grad = _device(fs, case.obs)
        obs = _tensors(case.obs)
        out = torch.zeros((k, npts), dtype=torch.float64, device="cuda:0")
        grad = torch.zeros((k, n, npts), dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            fs.eval_grad_tensors(obs, out, grad)  # torch's current stream is the side stream
        fs.finish()
        assert fs.last_path == "fused"
        _assert_bits(out.cpu().numpy(), eager_out, "side stream out")
        _assert_bits(grad.cpu().numpy(), eager_grad, "side stream grad")
        out.zero_()
        grad.zero_()
        torch.cuda.synchronize()
        fs.eval_grad_tensors(obs, out, grad, stream=side)  # the stream given explicitly
        fs.finish(side)
        _assert_bits(out.cpu().numpy(), eager_out, "stream= out")
        _assert_bits(grad.cpu().numpy(), eager_grad, "stream= grad")
        out.zero_()
        grad.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fs.eval_grad_tensors(obs, out, grad, no_alloc=True)
        assert fs.last_path == "fused"
        assert float(out.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0  # captured, not run
        rng = np.random.default_rng(77)
        for rep in range(2):
            host = [rng.uniform(-1.2, 1.2, npts) for _ in range(n)]
            want_out, want_grad = _device(fs, host)
            for d in range(n):
                obs[d].copy_(torch.from_numpy(host[d]))
            out.zero_()
            grad.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits(out.cpu().numpy(), want_out, ("replay out", rep))
            _assert_bits(grad.cpu().numpy(), want_grad, ("replay grad", rep))
        fs.finish()
    finally:
        fs.close()


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_interpn_fields_grad_both_layouts(kind):
    import torch

    import interpn_amd

    k, n = 3, 2
    case, fields = _fields_case("linear", kind, SHAPES[n], np.float64, k, seed=9, nobs=600)
    obs2d = [o.reshape(20, 30) for o in case.obs]
    want = [interpn_amd.interpn_grad(obs2d, case.grids, fields[f].reshape(SHAPES[n])) for f in range(k)]
    want_out = np.stack([w[0] for w in want])   # (K, 20, 30)
    want_jac = np.stack([w[1] for w in want])   # (K, N, 20, 30)
    vals_first = fields.reshape(k, *SHAPES[n])
    vals_last = np.ascontiguousarray(np.moveaxis(vals_first, 0, -1))
    out, jac = interpn_amd.interpn_fields_grad(obs2d, case.grids, vals_first)
    assert out.shape == (k, 20, 30) and jac.shape == (k, n, 20, 30)
    _assert_bits(out, want_out, "host, fields first")
    _assert_bits(jac, want_jac, "host, fields first")
    out, jac = interpn_amd.interpn_fields_grad(obs2d, case.grids, vals_last, field_axis=-1)
    assert out.shape == (20, 30, k) and jac.shape == (20, 30, k, n)
    _assert_bits(out, np.ascontiguousarray(np.moveaxis(want_out, 0, -1)), "host, fields last")
    _assert_bits(jac, np.ascontiguousarray(want_jac.transpose(2, 3, 0, 1)), "host, fields last")
    tobs = [torch.from_numpy(o).to("cuda:0") for o in obs2d]
    out, jac = interpn_amd.interpn_fields_grad(tobs, case.grids, torch.from_numpy(vals_first).to("cuda:0"))
    assert tuple(out.shape) == (k, 20, 30) and tuple(jac.shape) == (k, n, 20, 30)
    _assert_bits(out.cpu().numpy(), want_out, "device, fields first")
    _assert_bits(jac.cpu().numpy(), want_jac, "device, fields first")
    out, jac = interpn_amd.interpn_fields_grad(tobs, case.grids, torch.from_numpy(vals_last).to("cuda:0"), field_axis=-1)
    assert tuple(out.shape) == (20, 30, k) and tuple(jac.shape) == (20, 30, k, n) and jac.is_contiguous()
    _assert_bits(out.cpu().numpy(), np.ascontiguousarray(np.moveaxis(want_out, 0, -1)), "device, fields last")
    _assert_bits(jac.cpu().numpy(), np.ascontiguousarray(want_jac.transpose(2, 3, 0, 1)), "device, fields last")
    with pytest.raises(ValueError, match="field_axis"):
        interpn_amd.interpn_fields_grad(obs2d, case.grids, vals_first, field_axis=1)


@pytest.mark.parametrize("kind,n", [("regular", 3), ("rectilinear", 2)])
def test_autograd_interp_fields(kind, n):
    import torch

    from interpn_amd import autograd

    k = 3
    case, fields = _fields_case("linear", kind, SHAPES[n], np.float64, k, seed=91, nobs=200, extrap=0.1)
    fs = _make(case, fields)
    try:
        _out, jac = fs.eval_grad_tensors(_tensors(case.obs))
        fs.finish()
        assert torch.isfinite(jac).all()
        for f in range(k):  # one-hot in field f: obs[d].grad is J[f, d], bit for bit
            obs = [t.reshape(10, 20).requires_grad_(True) for t in _tensors(case.obs)]
            res = autograd.interp_fields(fs, obs)
            assert tuple(res.shape) == (k, 10, 20)
            sel = torch.zeros_like(res)
            sel[f] = 1.0
            res.backward(sel)
            for d in range(n):
                _assert_bits(obs[d].grad.reshape(-1).cpu().numpy(), jac[f, d].cpu().numpy(), ("one-hot", f, d))
        obs = [t.requires_grad_(True) for t in _tensors(case.obs)]
        res = autograd.interp_fields(fs, obs)
        gout = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (k, 200))).to("cuda:0")
        res.backward(gout)
        want = (gout[:, None] * jac).sum(0)
        for d in range(n):
            assert torch.equal(obs[d].grad, want[d]), d
        # only the coordinates that ask for it get a gradient
        obs = [t.requires_grad_(d == 1) for d, t in enumerate(_tensors(case.obs))]
        autograd.interp_fields(fs, obs).sum().backward()
        assert obs[0].grad is None and obs[1].grad is not None
    finally:
        fs.close()


def test_python_layout_rules():
    import torch

    case, fields = _fields_case("linear", "regular", SHAPES[2], np.float64, 3, seed=4, nobs=100)
    fs = _make(case, fields)
    try:
        obs = _tensors(case.obs)
        bad_last = torch.zeros((3, 2, 200), dtype=torch.float64, device="cuda:0")[:, :, ::2]
        with pytest.raises(ValueError, match="last axis must be contiguous"):
            fs.eval_grad_tensors(obs, None, bad_last)
        uneven = torch.zeros((3, 3, 100), dtype=torch.float64, device="cuda:0")[:, :2]  # stride(0) = 3 rows, stride(1) = 1 row
        with pytest.raises(ValueError, match="one uniform stride"):
            fs.eval_grad_tensors(obs, None, uneven)
        with pytest.raises(ValueError, match="rows must be contiguous"):
            fs.eval_grad_tensors(obs, torch.zeros((3, 200), dtype=torch.float64, device="cuda:0")[:, ::2])
        with pytest.raises(TypeError, match="grad: expected"):
            fs.eval_grad_tensors(obs, None, torch.zeros((3, 100), dtype=torch.float64, device="cuda:0"))
        with pytest.raises(ValueError, match="one uniform stride"):
            fs.eval_grad_host(case.obs, None, np.zeros((3, 3, 100))[:, :2])
        with pytest.raises(TypeError, match="takes no"):
            fs.eval_grad(case.obs, stream=None)
        out, grad = fs.eval_grad(obs)
        fs.finish()
        hout, hgrad = fs.eval_grad(case.obs)
        _assert_bits(out.cpu().numpy(), hout, "eval_grad dispatch")
        _assert_bits(grad.cpu().numpy(), hgrad, "eval_grad dispatch")
    finally:
        fs.close()


def test_abi_argument_checks():
    import torch

    from interpn_amd import _lib

    lib = _lib.load()
    n, k, nd = 64, 3, 2
    case, fields = _fields_case("linear", "regular", SHAPES[nd], np.float64, k, seed=71, nobs=n)
    fs = _make(case, fields)
    try:
        out = np.zeros((k, n))
        grad = np.zeros((k, nd, n))
        # host pointers throughout: every call below returns before any device work
        vp = (c_void_p * 3)(*[o.ctypes.data for o in case.obs], case.obs[0].ctypes.data)
        lens = (c_size_t * 3)(n, n, n)
        po, pg = c_void_p(out.ctypes.data), c_void_p(grad.ctypes.data)

        def dev(obs=vp, nobs=nd, o=po, ostride=n, g=pg, gstride=n, npoints=n, flags=0):
            return lib.interpn_hip_fields_eval_grad_device(fs._h, obs, nobs, o, ostride, g, gstride, npoints, None, flags, None)

        def host(obs=vp, ls=lens, nobs=nd, o=po, ostride=n, g=pg, gstride=n, nout=n):
            return lib.interpn_hip_fields_eval_grad_host(fs._h, obs, ls, nobs, o, ostride, g, gstride, nout)

        assert dev(g=None) == INVALID and host(g=None) == INVALID
        assert dev(o=None) == INVALID and host(o=None) == INVALID
        assert dev(gstride=n - 1) == INVALID and host(gstride=n - 1) == INVALID
        assert dev(ostride=n - 1) == INVALID and host(ostride=n - 1) == INVALID
        assert dev(flags=2) == INVALID and dev(flags=0x80000000) == INVALID
        for nobs in (1, 3):
            assert dev(nobs=nobs) == DIM_MISMATCH and host(nobs=nobs) == DIM_MISMATCH
        assert host(ls=(c_size_t * 2)(n, n - 1)) == DIM_MISMATCH
        assert host(ls=None) == INVALID
        null1 = (c_void_p * 2)(case.obs[0].ctypes.data, None)
        assert dev(obs=null1) == INVALID and host(obs=null1) == INVALID
        assert lib.interpn_hip_fields_eval_grad_device(None, vp, nd, po, n, pg, n, n, None, 0, None) == INVALID
        assert lib.interpn_hip_fields_eval_grad_host(None, vp, lens, nd, po, n, pg, n, n) == INVALID
        # no points: nothing to do, whatever the other pointers are
        assert dev(o=None, g=None, ostride=0, gstride=0, npoints=0) == OK
        assert host(ls=(c_size_t * 2)(0, 0), o=None, g=None, ostride=0, gstride=0, nout=0) == OK
        assert not out.any() and not grad.any()
        # and a valid call through the same entry point reports its path
        path = c_int(-1)
        tobs = _tensors(case.obs)
        tout = torch.zeros((k, n), dtype=torch.float64, device="cuda:0")
        tgrad = torch.zeros((k, nd, n), dtype=torch.float64, device="cuda:0")
        tp = (c_void_p * 2)(*[t.data_ptr() for t in tobs])
        fs.set_option("fused", 1)
        assert lib.interpn_hip_fields_eval_grad_device(fs._h, tp, nd, c_void_p(tout.data_ptr()), n, c_void_p(tgrad.data_ptr()), n, n, None,
                                                       1, path) == OK
        fs.finish()
        assert path.value == 0 and fs.get_option("last_path") == 0
        ref_out, ref_grad = _device(fs, case.obs)
        _assert_bits(tout.cpu().numpy(), ref_out, "raw call out")
        _assert_bits(tgrad.cpu().numpy(), ref_grad, "raw call grad")
    finally:
        fs.close()
