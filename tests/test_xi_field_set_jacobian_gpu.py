"""Point-major gradients of a field set on the GPU (interpn_hip_fields_eval_points_grad_*, Fields.eval_points_grad_*,
interpn_fields_points_grad, interpn_amd.autograd.interp_fields_points): (n, N) points in, (n, K) values and the (n, K, N)
Jacobian out, one call.

The definition is by reference: out[i, f] and jac[i, f, d] have the bits of out[f, i] and grad[f, d, i] of the column form
`Fields.eval_grad_*` on the de-interleaved columns.  Every comparison against that is on bit patterns — NaN payloads and
signed zeros count — and nothing has a tolerance.  The numpy restatements (tests/grad_restatement.py,
tests/cubic_grad_restatement.py), which do not depend on the code under test, are compared bit for bit too, except that a
NaN need only be a NaN on both sides (numpy's NaN payloads are not the device's).

The file is named to be collected after every earlier GPU file, so that the positions of the existing GPU tests in a
whole-suite run, and the streams they are handed, stay what they were.

Wall time of this file on one MI355X: 4.5 s."""

import dataclasses
import functools
from ctypes import c_int, c_void_p

import numpy as np
import pytest

from tests import cubic_grad_restatement as cgr
from tests import grad_restatement as gr
from tests.helpers import synthetic_case

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, 32, 33
KERNEL = "interpn::k_linear_fields_points_grad<"
SHAPES = {2: [9, 8], 3: [7, 6, 5]}
KMAX = 17


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


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _rows(obs):
    return np.ascontiguousarray(np.stack(obs, axis=1))


def _pm(out, grad):
    """The column form's (K, n) and (K, N, n) as the point-major (n, K) and (n, K, N)."""
    return np.ascontiguousarray(out.T), np.ascontiguousarray(grad.transpose(2, 0, 1))


def _fields_case(method, kind, shape, dtype, k, seed, nobs=1500, linearize=False, extrap=0.3):
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


def _restated(case, fields, fma=True, obs=None):
    """Point-major (out (n, K), jac (n, K, N), ok (n,)) of the numpy restatement, field by field."""
    mod = cgr if case.method == "cubic" else gr
    outs, grads, ok = [], [], None
    for f in range(fields.shape[0]):
        c = dataclasses.replace(case, vals=fields[f], obs=case.obs if obs is None else obs)
        o, g, ok = mod.eval_grad_case(c, fma=fma)
        outs.append(o)
        grads.append(g)
    return _pm(np.stack(outs), np.stack(grads)) + (ok,)


def _columns(fs, obs):
    """The reference by definition: the column form on the de-interleaved columns, point-major."""
    out, grad = fs.eval_grad_tensors([_cuda(o) for o in obs])
    fs.finish()
    return _pm(out.cpu().numpy(), grad.cpu().numpy())


def _device(fs, pts, out=None, jac=None, **kw):
    out_t, jac_t = fs.eval_points_grad_tensors(pts if hasattr(pts, "is_cuda") else _cuda(pts), out, jac, **kw)
    fs.finish()
    return out_t.cpu().numpy(), jac_t.cpu().numpy()


def _kernel_name(dtype, n, kind, fma):
    tname = "double" if np.dtype(dtype) == np.float64 else "float"
    return f"{KERNEL}{tname}, {n}, {'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>"


def _check_both_paths(fs, case, ctx, w_out=None, w_jac=None, slice_points=256):
    """Fused and split against the column form (and the restatement, where given), device and host."""
    c_out, c_jac = _columns(fs, case.obs)
    pts = _rows(case.obs)
    for path in (1, 2):
        fs.set_option("points_path", path)
        fs.set_option("points_slice", slice_points)
        out, jac = _device(fs, pts)
        assert fs.last_points_path == ("fused" if path == 1 else "split"), ctx
        if path == 1:
            assert fs.kernel_name().startswith(KERNEL), (ctx, fs.kernel_name())
        _assert_bits(out, c_out, ("out", path, ctx))
        _assert_bits(jac, c_jac, ("jac", path, ctx))
        if w_out is not None:
            _assert_restated(out, w_out, ("out restated", path, ctx))
            _assert_restated(jac, w_jac, ("jac restated", path, ctx))
        hout, hjac = fs.eval_points_grad_host(pts)
        _assert_bits(hout, c_out, ("host out", path, ctx))
        _assert_bits(hjac, c_jac, ("host jac", path, ctx))
    fs.set_option("points_path", -1)


# ---- 1. every fused instantiation ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parity_reference(kind, n, dtype_name, fma):
    """The case of the parity test with KMAX fields and its restatement: computed once per (kind, N, dtype, flavour); a set
    of K fields holds the first K."""
    dtype = np.dtype(dtype_name).type
    case, fields = _fields_case("linear", kind, SHAPES[n], dtype, KMAX, seed=31 * n + (kind == "regular") + 2 * fma)
    for d in range(n):  # reaching beyond the grid on every side
        assert case.obs[d].min() < case.grids[d][0] and case.obs[d].max() > case.grids[d][-1]
    r_out, r_jac, ok = _restated(case, fields, fma)
    assert ok.all()
    r_out.setflags(write=False)
    r_jac.setflags(write=False)
    return case, fields, r_out, r_jac


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 17])
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_parity_of_every_fused_instantiation(kind, n, dtype, fma, k):
    """A full line, a padded last line, more than one line group and more than one 8-field tile; points beyond the grid on
    every side."""
    case, fields, r_out, r_jac = _parity_reference(kind, n, np.dtype(dtype).name, fma)
    fs = _make(case, fields[:k], fma)
    try:
        assert fs.get_option("fused_table_bytes") > 0
        c_out, c_jac = _columns(fs, case.obs)
        pts = _rows(case.obs)
        # automatic: fused, but for two fields per line in four line groups or more (3-D f64, K >= 7)
        auto = "split" if (np.dtype(dtype).itemsize, n) == (8, 3) and k >= 7 else "fused"
        out, jac = _device(fs, pts)
        assert fs.last_points_path == auto and fs.get_option("last_points_path") == (auto == "split"), (auto, fs.last_points_path)
        _assert_bits(out, c_out, ("automatic, values", kind, n, k))
        _assert_bits(jac, c_jac, ("automatic, Jacobian", kind, n, k))
        fs.set_option("points_path", 1)
        out, jac = _device(fs, pts)
        assert fs.last_points_path == "fused" and fs.get_option("last_points_path") == 0 and fs.last_path == "fused"
        assert fs.kernel_name() == _kernel_name(dtype, n, kind, fma), fs.kernel_name()
        assert out.shape == (pts.shape[0], k) and jac.shape == (pts.shape[0], k, n)
        ctx = (kind, n, np.dtype(dtype).name, fma, k)
        _assert_bits(out, c_out, ("values against the column form",) + ctx)
        _assert_bits(jac, c_jac, ("Jacobian against the column form",) + ctx)
        _assert_restated(out, r_out[:, :k], ("values against the restatement",) + ctx)
        _assert_restated(jac, r_jac[:, :k], ("Jacobian against the restatement",) + ctx)
        hout, hjac = fs.eval_points_grad_host(pts)
        assert fs.last_points_path == "fused"
        _assert_bits(hout, c_out, ("host values",) + ctx)
        _assert_bits(hjac, c_jac, ("host Jacobian",) + ctx)
    finally:
        fs.close()


# ---- 2. ragged waves and workgroups, wider blocks --------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["wide", "dense"])
@pytest.mark.parametrize("path", ["fused", "split"])
@pytest.mark.parametrize("kind,n,dtype,k", [("regular", 3, np.float64, 3), ("rectilinear", 2, np.float32, 9),
                                            ("rectilinear", 3, np.float32, 5), ("regular", 2, np.float64, 5)])
def test_batch_sizes_and_guards(kind, n, dtype, k, path, layout):
    """wide: `pts` is buf[:, :N] of an (n, N + 1) block, out_stride = K + 3, jac_stride = K N + 5, every base an odd number
    of elements into its sentinel-filled block.  dense: stride == N (the LDS load) and jac_stride == K N (the one-run
    store).  Exactly the first K and K N elements of the first n rows change."""
    import torch

    big, fields = _fields_case("linear", kind, SHAPES[n], dtype, k, seed=5 * n + k, nobs=1000)
    w_out, w_jac, ok = _restated(big, fields)
    assert ok.all()
    rows = _rows(big.obs)
    td, sentinel, off = _tdtype(dtype), -12345.5, 3
    ps, os_, js = (n + 1, k + 3, k * n + 5) if layout == "wide" else (n, k, k * n)
    fs = _make(big, fields)
    try:
        fs.set_option("points_path", 1 if path == "fused" else 2)
        fs.set_option("points_slice", 256)
        for npts in (1, 63, 64, 65, 255, 256, 257, 1000):
            tp = torch.full((off + npts * ps + 7,), 7.75, dtype=td, device="cuda:0")
            pview = tp[off:off + npts * ps].view(npts, ps)[:, :n]
            pview.copy_(_cuda(rows[:npts]))
            to = torch.full((off + (npts + 2) * os_,), sentinel, dtype=td, device="cuda:0")
            tj = torch.full((off + (npts + 2) * js,), sentinel, dtype=td, device="cuda:0")
            oview = to[off:off + npts * os_].view(npts, os_)[:, :k]
            jview = tj[off:off + npts * js].view(npts, js)[:, :k * n].unflatten(1, (k, n))
            fs.eval_points_grad_tensors(pview, oview, jview)
            fs.finish()
            assert fs.last_points_path == path
            go, gj = to.cpu().numpy(), tj.cpu().numpy()
            _assert_restated(go[off:off + npts * os_].reshape(npts, os_)[:, :k], w_out[:npts], ("out", npts))
            _assert_restated(gj[off:off + npts * js].reshape(npts, js)[:, :k * n].reshape(npts, k, n), w_jac[:npts], ("jac", npts))
            for blk, st, width in ((go, os_, k), (gj, js, k * n)):
                assert np.all(blk[:off] == sentinel) and np.all(blk[off + npts * st:] == sentinel), (npts, "around")
                assert np.all(blk[off:off + npts * st].reshape(npts, st)[:, width:] == sentinel), (npts, "behind a row")
            # the host form, the same way
            hp = np.full(off + npts * ps + 7, 7.75, dtype=dtype)
            hp[off:off + npts * ps].reshape(npts, ps)[:, :n] = rows[:npts]
            ho = np.full(off + (npts + 2) * os_, sentinel, dtype=dtype)
            hj = np.full(off + (npts + 2) * js, sentinel, dtype=dtype)
            fs.eval_points_grad_host(hp[off:off + npts * ps].reshape(npts, ps)[:, :n],
                                     ho[off:off + npts * os_].reshape(npts, os_)[:, :k],
                                     hj[off:off + npts * js].reshape(npts, js)[:, :k * n].reshape(npts, k, n))
            _assert_bits(ho, go, ("host out block", npts))
            _assert_bits(hj, gj, ("host jac block", npts))
    finally:
        fs.close()


# ---- 3. grids ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("shape", [[2, 2], [2, 9], [9, 2], [2, 9, 2], [7, 2, 5], [2, 2, 2]], ids=str)
def test_axes_of_exactly_two_points(shape, kind):
    for dtype in (np.float64, np.float32):
        case, fields = _fields_case("linear", kind, shape, dtype, 5, seed=sum(shape), nobs=700)
        w_out, w_jac, ok = _restated(case, fields)
        assert ok.all()
        fs = _make(case, fields)
        try:
            _check_both_paths(fs, case, (shape, kind, np.dtype(dtype).name), w_out, w_jac)
        finally:
            fs.close()


def _clustered_axis(length, rng, dtype):
    """[-1, 1] in `length` knots whose cell widths alternate at random between wide and a twentieth of it."""
    w = rng.choice([1.0, 0.05], length - 1)
    g = -1.0 + 2.0 * np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
    g[0], g[-1] = -1.0, 1.0
    g = g.astype(dtype)
    assert np.all(np.diff(g) > 0)
    return g


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("length", [5, 3000])
def test_clustered_rectilinear_axes(length, dtype):
    """Axes inside the LDS image and beyond it, clustered knots: the divisor is the cell's own x1 - x0, which differs from
    lane to lane and reaches the storing lane through LDS."""
    for shape in ([length, 9], [4, 5, length]):
        case, fields = _fields_case("linear", "rectilinear", shape, dtype, 3, seed=length % 89 + len(shape), nobs=1500)
        rng = np.random.default_rng(length)
        case = dataclasses.replace(case, grids=[_clustered_axis(m, rng, dtype) for m in shape])
        w_out, w_jac, ok = _restated(case, fields)
        assert ok.all()
        fs = _make(case, fields)
        try:
            _check_both_paths(fs, case, (shape, np.dtype(dtype).name), w_out, w_jac, slice_points=512)
        finally:
            fs.close()


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
    fs = _make(case, fields)
    try:
        c_out, c_jac = _columns(fs, case.obs)
        assert np.isnan(c_jac).any() and np.isinf(c_jac).any()
        _check_both_paths(fs, case, (n, np.dtype(dtype).name))
    finally:
        fs.close()


# ---- 4. the failing-point contract -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "split_fused", "split_per_field"])
@pytest.mark.parametrize("dtype,n", [(np.float64, 3), (np.float32, 2)])
def test_failing_point_contract(dtype, n, mode):
    """An unrepresentable coordinate is reported through the status; the index counts from the call's first point, across
    slices of 256 points and across host chunks."""
    npts, bad, k = 1500, 700, 3
    case, fields = _fields_case("linear", "regular", SHAPES[n], dtype, k, seed=11 + n, nobs=npts)
    w_out, w_jac, _ = _restated(case, fields)
    case.obs[n - 1][bad] = 1e300 if dtype == np.float64 else 3e38
    case.obs[0][bad + 300] = np.nan  # a later failure, in a later slice, must not be the one reported
    _, _, ok = _restated(case, fields[:1])
    assert int(np.argmin(ok)) == bad and not ok[bad]
    pts = _rows(case.obs)
    fs = _make(case, fields)
    try:
        fs.set_option("points_slice", 256)
        fs.set_option("points_path", 1 if mode == "fused" else 2)
        fs.set_option("fused", 0 if mode == "split_per_field" else 1)
        fs.eval_points_grad_tensors(_cuda(pts))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as err:
            fs.finish()
        assert err.value.first_bad_index == bad
        assert fs.last_points_path == ("fused" if mode == "fused" else "split")
        fs.set_option("host_chunk", 600)  # three chunks, the failing point in the second, in a later slice of it
        sentinel = dtype(777.25)
        out = np.full((npts, k + 2), sentinel, dtype=dtype)
        jac = np.full((npts, k * n + 1), sentinel, dtype=dtype)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
            fs.eval_points_grad_host(pts, out[:, :k], jac[:, :k * n].reshape(npts, k, n))
        _assert_restated(out[:bad, :k], w_out[:bad], "host out in front")
        _assert_restated(jac[:bad, :k * n].reshape(bad, k, n), w_jac[:bad], "host jac in front")
        assert np.all(out[bad:] == sentinel) and np.all(jac[bad:] == sentinel)
        assert np.all(out[:, k:] == sentinel) and np.all(jac[:, k * n:] == sentinel)
        # the status word is cleared: a clean batch afterwards is clean
        _device(fs, pts[:bad])
    finally:
        fs.close()


# ---- 5. the split path -------------------------------------------------------------------------------------------------------
def _check_split(case, fields, ctx, restate=True, expect_kernel=None):
    """Three slices of 256, 256 and a ragged rest, against the column form and the restatement."""
    fs = _make(case, fields)
    try:
        c_out, c_jac = _columns(fs, case.obs)
        fs.set_option("points_slice", 256)
        pts = _rows(case.obs)
        assert 512 < pts.shape[0] < 768 and pts.shape[0] % 256
        out, jac = _device(fs, pts)
        assert fs.last_points_path == "split" and not fs.kernel_name().startswith(KERNEL), (ctx, fs.kernel_name())
        if expect_kernel:
            assert expect_kernel in fs.kernel_name(), (ctx, fs.kernel_name())
        _assert_bits(out, c_out, ("out", ctx))
        _assert_bits(jac, c_jac, ("jac", ctx))
        if restate:
            w_out, w_jac, ok = _restated(case, fields)
            assert ok.all()
            _assert_restated(out, w_out, ("out restated", ctx))
            _assert_restated(jac, w_jac, ("jac restated", ctx))
        hout, hjac = fs.eval_points_grad_host(pts)
        _assert_bits(hout, c_out, ("host out", ctx))
        _assert_bits(hjac, c_jac, ("host jac", ctx))
        return fs.last_path
    finally:
        fs.close()


@pytest.mark.parametrize("linearize", [False, True], ids=["hold", "linearize"])
@pytest.mark.parametrize("shape", [[9, 11], [7, 9, 8]], ids=str)
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_split_multicubic(kind, shape, linearize):
    case, fields = _fields_case("cubic", kind, shape, np.float64, 3, seed=7 + len(shape), nobs=700, linearize=linearize)
    assert _check_split(case, fields, (kind, shape, linearize), expect_kernel="cubic") == "per_field"


@pytest.mark.parametrize("shape", [[301], [5, 4, 6, 7]], ids=str)
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_split_multilinear_other_dimensions(kind, shape):
    case, fields = _fields_case("linear", kind, shape, np.float64, 3, seed=len(shape), nobs=700)
    assert _check_split(case, fields, (kind, shape), expect_kernel="k_linear_grad_n<") == "per_field"


def test_split_set_refused_its_table(monkeypatch):
    from interpn_amd._lib import InterpnHipError

    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, 4, seed=2, nobs=700)
    monkeypatch.setenv("INTERPN_HIP_FIELDS_TABLE_BUDGET", "0")
    assert _check_split(case, fields, "no table") == "per_field"
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused_table_bytes") == 0
        fs.set_option("points_path", 1)
        with pytest.raises(InterpnHipError, match="unsupported"):
            fs.eval_points_grad_tensors(_cuda(_rows(case.obs)))
        with pytest.raises(InterpnHipError, match="unsupported"):
            fs.eval_points_grad_host(_rows(case.obs))
    finally:
        fs.close()


@pytest.mark.parametrize("option,value,column_path", [("fused", 0, "per_field"), ("points_path", 2, "fused")])
def test_split_by_option(option, value, column_path):
    case, fields = _fields_case("linear", "rectilinear", SHAPES[3], np.float32, 5, seed=23, nobs=700)
    w_out, w_jac, ok = _restated(case, fields)
    assert ok.all()
    pts = _rows(case.obs)
    fs = _make(case, fields)
    try:
        fused = _device(fs, pts)
        assert fs.last_points_path == "fused"
        fs.set_option(option, value)
        fs.set_option("points_slice", 256)
        out, jac = _device(fs, pts)
        assert fs.last_points_path == "split" and fs.last_path == column_path and not fs.kernel_name().startswith(KERNEL)
        _assert_bits(out, fused[0], "out")
        _assert_bits(jac, fused[1], "jac")
        _assert_restated(out, w_out, "out restated")
        _assert_restated(jac, w_jac, "jac restated")
    finally:
        fs.close()


def test_nearest_sets_are_unsupported():
    import interpn_amd
    from interpn_amd import _lib

    case, fields = _fields_case("nearest", "regular", SHAPES[2], np.float64, 2, seed=3, nobs=64)
    pts = _rows(case.obs)
    fs = _make(case, fields)
    try:
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            fs.eval_points_grad_host(pts)
        with pytest.raises(_lib.InterpnHipError, match="unsupported"):
            fs.eval_points_grad(_cuda(pts))
    finally:
        fs.close()
    vals = np.ascontiguousarray(np.moveaxis(fields.reshape(2, *SHAPES[2]), 0, -1))
    with pytest.raises(_lib.InterpnHipError, match="unsupported"):
        interpn_amd.interpn_fields_points_grad(pts, case.grids, vals, method="nearest")


def test_abi_checks_in_their_order():
    """The header's check list on live sets, with host pointers that are never dereferenced: each status comes back in front
    of everything behind it in the list."""
    from interpn_amd import _lib

    lib = _lib.load()
    buf = np.zeros(64)
    p = c_void_p(buf.ctypes.data)
    n, k = 2, 3
    case, fields = _fields_case("nearest", "regular", SHAPES[n], np.float64, k, seed=3, nobs=64)
    fs = _make(case, fields)
    try:
        dev = lambda *a: lib.interpn_hip_fields_eval_points_grad_device(fs._h, *a)
        host = lambda *a: lib.interpn_hip_fields_eval_points_grad_host(fs._h, *a)
        # 2. a nearest set: in front of the strides, of npoints == 0, of the pointers and of the flags
        assert dev(None, 1, 0, None, 0, None, 0, None, 6, None) == UNSUPPORTED
        assert dev(p, n, 4, p, k, p, k * n, None, 0, None) == UNSUPPORTED
        assert host(None, 1, 0, None, 0, None, 0) == UNSUPPORTED
    finally:
        fs.close()
    case, fields = _fields_case("linear", "regular", SHAPES[n], np.float64, k, seed=3, nobs=64)
    fs = _make(case, fields)
    try:
        dev = lambda *a: lib.interpn_hip_fields_eval_points_grad_device(fs._h, *a)
        host = lambda *a: lib.interpn_hip_fields_eval_points_grad_host(fs._h, *a)
        # 3. the strides: in front of npoints == 0 and of the pointers
        for bad in ((n - 1, k, k * n), (n, k - 1, k * n), (n, k, k * n - 1)):
            assert dev(None, bad[0], 0, None, bad[1], None, bad[2], None, 0, None) == INVALID, bad
            assert host(None, bad[0], 0, None, bad[1], None, bad[2]) == INVALID, bad
        # 4. npoints == 0: OK whatever the pointers are, in front of the flags and of points_path
        path = c_int(-7)
        assert dev(None, n, 0, None, k, None, k * n, None, 6, path) == OK and path.value == 1
        assert host(None, n, 0, None, k, None, k * n) == OK
        # 5. the pointers, and blocks whose bytes overflow size_t: in front of the flags
        for ptrs in ((None, p, p), (p, None, p), (p, p, None)):
            assert dev(ptrs[0], n, 4, ptrs[1], k, ptrs[2], k * n, None, 6, None) == INVALID, ptrs
            assert host(ptrs[0], n, 4, ptrs[1], k, ptrs[2], k * n) == INVALID, ptrs
        huge = (1 << 61) // n
        assert dev(p, n, huge, p, k, p, k * n, None, 0, None) == INVALID
        assert dev(p, 1 << 40, 1 << 30, p, k, p, k * n, None, 0, None) == INVALID
        assert host(p, n, 1 << 58, p, k, p, (1 << 6) + k * n) == INVALID
        # 6. unknown flags
        assert dev(p, n, 4, p, k, p, k * n, None, 2, None) == INVALID
        assert lib.interpn_hip_fields_reserve_points_grad(fs._h, 100, -1) == INVALID
        assert lib.interpn_hip_fields_reserve_points_grad(fs._h, 0, 1) == OK
        assert not buf.any()
    finally:
        fs.close()


# ---- 6. capture and allocation ------------------------------------------------------------------------------------------------
def test_no_alloc_and_reserved_scratch():
    from interpn_amd._lib import InterpnHipError

    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, 3, seed=17, nobs=700)
    pts = _cuda(_rows(case.obs))
    fs = _make(case, fields)
    try:
        want = _columns(fs, case.obs)
        got = _device(fs, pts, no_alloc=True)  # fused: nothing reserved, nothing needed
        assert fs.last_points_path == "fused"
        _assert_bits(got[0], want[0], "fused out")
        _assert_bits(got[1], want[1], "fused jac")
        fs.set_option("points_path", 2)
        with pytest.raises(InterpnHipError, match="[Oo]ut of memory|memory"):
            fs.eval_points_grad_tensors(pts, no_alloc=True)
        fs.reserve_points_grad(700)
        got = _device(fs, pts, no_alloc=True)
        assert fs.last_points_path == "split"
        _assert_bits(got[0], want[0], "split out")
        _assert_bits(got[1], want[1], "split jac")
    finally:
        fs.close()


def test_side_stream_and_graph_capture():
    """One fused evaluation on a side stream, and one captured into a graph (one kernel on the capture stream: a single
    branch) and replayed twice on new points in the same buffers: the bits of an eager call."""
    import torch

    npts, n, k = 1501, 3, 5
    case, fields = _fields_case("linear", "rectilinear", SHAPES[n], np.float64, k, seed=21, nobs=npts)
    fs = _make(case, fields)
    try:
        pts = _cuda(_rows(case.obs))
        eager_out, eager_jac = _device(fs, pts)
        assert fs.last_points_path == "fused"
        out = torch.zeros((npts, k), dtype=torch.float64, device="cuda:0")
        jac = torch.zeros((npts, k, n), dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            fs.eval_points_grad_tensors(pts, out, jac)  # torch's current stream is the side stream
        fs.finish()
        _assert_bits(out.cpu().numpy(), eager_out, "side stream out")
        _assert_bits(jac.cpu().numpy(), eager_jac, "side stream jac")
        out.zero_()
        jac.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fs.eval_points_grad_tensors(pts, out, jac, no_alloc=True)
        assert fs.last_points_path == "fused"
        assert float(out.abs().max()) == 0.0 and float(jac.abs().max()) == 0.0  # captured, not run
        rng = np.random.default_rng(77)
        for rep in range(2):
            host = rng.uniform(-1.2, 1.2, (npts, n))
            want_out, want_jac = _device(fs, host)
            pts.copy_(torch.from_numpy(host))
            out.zero_()
            jac.zero_()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            _assert_bits(out.cpu().numpy(), want_out, ("replay out", rep))
            _assert_bits(jac.cpu().numpy(), want_jac, ("replay jac", rep))
        fs.finish()
    finally:
        fs.close()


# ---- 7. the one-call form and autograd ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["linear", "cubic"])
@pytest.mark.parametrize("kind,n", [("regular", 3), ("rectilinear", 2)])
def test_interpn_fields_points_grad(kind, n, method):
    import torch

    import interpn_amd

    k = 3
    shape = SHAPES[n] if method == "linear" else [s + 2 for s in SHAPES[n]]
    case, fields = _fields_case(method, kind, shape, np.float64, k, seed=9, nobs=35)
    xi = _rows(case.obs).reshape(5, 7, n)
    obs3 = [o.reshape(5, 7) for o in case.obs]
    vals_first = fields.reshape(k, *shape)
    vals_last = np.ascontiguousarray(np.moveaxis(vals_first, 0, -1))
    w_out, w_jac = interpn_amd.interpn_fields_grad(obs3, case.grids, vals_first, method=method)  # (K, 5, 7), (K, N, 5, 7)
    w_out = np.ascontiguousarray(np.moveaxis(w_out, 0, -1))
    w_jac = np.ascontiguousarray(w_jac.transpose(2, 3, 0, 1))
    out, jac = interpn_amd.interpn_fields_points_grad(xi, case.grids, vals_last, method=method)
    assert out.shape == (5, 7, k) and jac.shape == (5, 7, k, n)
    _assert_bits(out, w_out, "numpy out")
    _assert_bits(jac, w_jac, "numpy jac")
    out, jac = interpn_amd.interpn_fields_points_grad(torch.from_numpy(xi).to("cuda:0"), case.grids,
                                                      torch.from_numpy(vals_last).to("cuda:0"), method=method)
    assert out.is_cuda and jac.is_cuda and tuple(out.shape) == (5, 7, k) and tuple(jac.shape) == (5, 7, k, n)
    _assert_bits(out.cpu().numpy(), w_out, "cuda out")
    _assert_bits(jac.cpu().numpy(), w_jac, "cuda jac")


@pytest.mark.parametrize("kind,n", [("regular", 3), ("rectilinear", 2)])
def test_autograd_interp_fields_points(kind, n):
    """pts.grad against autograd.interp_fields on the unbound columns, bit for bit, for a random grad_out.  K = 2: both
    backward passes then add the same two rounded products, and a sum of two terms has one order."""
    import torch

    from interpn_amd import autograd

    k, npts = 2, 200
    case, fields = _fields_case("linear", kind, SHAPES[n], np.float64, k, seed=91, nobs=npts, extrap=0.1)
    fs = _make(case, fields)
    try:
        gout = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (10, 20, k))).to("cuda:0")
        cols = [_cuda(o).reshape(10, 20).requires_grad_(True) for o in case.obs]
        res_c = autograd.interp_fields(fs, cols)  # (K, 10, 20)
        res_c.backward(gout.permute(2, 0, 1))
        want = torch.stack([c.grad for c in cols], dim=-1)
        pts = _cuda(_rows(case.obs)).reshape(10, 20, n).requires_grad_(True)
        res = autograd.interp_fields_points(fs, pts)
        assert tuple(res.shape) == (10, 20, k) and fs.last_points_path == "fused"
        assert torch.equal(res.detach(), res_c.detach().permute(1, 2, 0))
        res.backward(gout)
        assert tuple(pts.grad.shape) == (10, 20, n)
        _assert_bits(pts.grad.cpu().numpy(), want.cpu().numpy(), "pts.grad")
        # one-hot in field f: pts.grad is J[:, f, :], bit for bit
        _out, jac = fs.eval_points_grad_tensors(pts.detach().reshape(-1, n))
        fs.finish()
        for f in range(k):
            q = pts.detach().clone().requires_grad_(True)
            r = autograd.interp_fields_points(fs, q)
            sel = torch.zeros_like(r)
            sel[..., f] = 1.0
            r.backward(sel)
            _assert_bits(q.grad.reshape(-1, n).cpu().numpy(), jac[:, f].cpu().numpy(), ("one-hot", f))
    finally:
        fs.close()


def test_python_layout_rules():
    import torch

    case, fields = _fields_case("linear", "regular", SHAPES[2], np.float64, 3, seed=4, nobs=100)
    fs = _make(case, fields)
    try:
        pts = _cuda(_rows(case.obs))
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda:0")
        with pytest.raises(ValueError, match=r"pts: expected shape \(\.\.\., 2\)"):
            fs.eval_points_grad_tensors(z(100, 3))
        with pytest.raises(TypeError, match="pts: expected"):
            fs.eval_points_grad_tensors(pts.float())
        with pytest.raises(ValueError, match=r"out: expected shape \(100, 3\)"):
            fs.eval_points_grad_tensors(pts, z(3, 100))
        with pytest.raises(ValueError, match=r"jac: expected shape \(100, 3, 2\)"):
            fs.eval_points_grad_tensors(pts, None, z(100, 2, 3))
        with pytest.raises(TypeError, match="jac: expected"):
            fs.eval_points_grad_tensors(pts, None, torch.zeros((100, 3, 2), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(ValueError, match="jac: every row must be contiguous"):
            fs.eval_points_grad_tensors(pts, None, z(100, 3, 4)[:, :, ::2])
        with pytest.raises(ValueError, match="out: every row must be contiguous"):
            fs.eval_points_grad_tensors(pts, z(100, 6)[:, ::2])
        with pytest.raises(TypeError, match="takes no"):
            fs.eval_points_grad(_rows(case.obs), stream=None)
        out, jac = fs.eval_points_grad(pts)
        fs.finish()
        hout, hjac = fs.eval_points_grad(_rows(case.obs))
        _assert_bits(out.cpu().numpy(), hout, "dispatch out")
        _assert_bits(jac.cpu().numpy(), hjac, "dispatch jac")
        eo, ej = fs.eval_points_grad(np.zeros((0, 2)))
        assert eo.shape == (0, 3) and ej.shape == (0, 3, 2)
    finally:
        fs.close()
