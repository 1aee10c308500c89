"""Field sets on the GPU: every row of a result is compared BIT FOR BIT with the oracle run on that field alone
(`tests.helpers.run_oracle`), on the fused path (interpn::k_linear_fields) and on the per-field path.

Wall time of the whole file on one MI355X: see DESIGN.md section 9 (measured with `pytest -m gpu tests/test_fields_gpu.py`).
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

FUSED_KERNEL = "interpn::k_linear_fields<"
SHAPES = {2: [37, 53], 3: [17, 12, 23]}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_rows(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (ctx, len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


def _fields_case(method, kind, shape, dtype, k, seed, nobs=3000, linearize=False):
    case = synthetic_case(method, kind, len(shape), shape, nobs, seed, dtype=dtype, linearize=linearize)
    rng = np.random.default_rng(1000 + seed)
    fields = np.stack([rng.uniform(-1.0, 1.0, case.vals.size).astype(dtype) for _ in range(k)])
    return case, fields


def _want(oracle, case, fields, fma, obs=None):
    obs = case.obs if obs is None else obs
    rows = []
    for f in range(fields.shape[0]):
        c = dataclasses.replace(case, vals=fields[f], obs=obs)
        rows.append(run_oracle(oracle, c, fma=fma, out=np.zeros(obs[0].size, dtype=fields.dtype)))
    return np.stack(rows)


def _make(case, fields, fma=None, vals=None):
    import interpn_amd

    vals = fields if vals is None else vals
    if case.kind == "regular":
        return interpn_amd.Fields.regular(case.method, case.dims, case.starts, case.steps, vals, linearize_extrapolation=case.linearize,
                                          dtype=fields.dtype, fma=fma)
    return interpn_amd.Fields.rectilinear(case.method, case.grids, vals, linearize_extrapolation=case.linearize, dtype=fields.dtype,
                                          fma=fma)


def _tensors(obs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(o)).to("cuda:0") for o in obs]


def _eval_both(fs, obs):
    """(host result, device result) of one set at the same points."""
    host = fs.eval_host([np.ascontiguousarray(o) for o in obs])
    path_host = fs.last_path
    dev = fs.eval_tensors(_tensors(obs))
    fs.finish()
    assert fs.last_path == path_host
    return host, dev.cpu().numpy()


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_fused_and_per_field_paths(oracle, kind, n, dtype, k, fma):
    case, fields = _fields_case("linear", kind, SHAPES[n], dtype, k, seed=7 * n + k)
    want = _want(oracle, case, fields, fma)
    fs = _make(case, fields, fma)
    try:
        assert fs.nfields == k and fs.ndims() == n
        assert fs.get_option("fused_table_bytes") > 0
        fs.set_option("fused", 1)  # wherever the table exists (what the set picks by itself: test_automatic_path)
        host, dev = _eval_both(fs, case.obs)
        assert fs.last_path == "fused"
        name = fs.kernel_name()
        assert name.startswith(FUSED_KERNEL), name
        tname = "double" if dtype == np.float64 else "float"
        assert name == f"{FUSED_KERNEL}{tname}, {n}, {'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>", name
        _assert_rows(host, want, ("fused host", kind, n, k))
        _assert_rows(dev, want, ("fused device", kind, n, k))
        fs.set_option("fused", 0)
        host0, dev0 = _eval_both(fs, case.obs)
        assert fs.last_path == "per_field"
        assert not fs.kernel_name().startswith(FUSED_KERNEL)
        _assert_rows(host0, want, ("per-field host", kind, n, k))
        _assert_rows(dev0, want, ("per-field device", kind, n, k))
        assert host0.tobytes() == host.tobytes() and dev0.tobytes() == dev.tobytes()
        fs.set_option("fused", 1)
        fs.eval_tensors(_tensors(case.obs))
        fs.finish()
        assert fs.last_path == "fused"
    finally:
        fs.close()


PER_FIELD_ONLY = [("cubic", [9, 11], False), ("cubic", [9, 11], True), ("cubic", [7, 9, 8], False), ("cubic", [7, 9, 8], True),
                  ("nearest", [9, 7, 11], False), ("linear", [301], False), ("linear", [5, 4, 6, 7], False),
                  ("linear", [3, 2, 4, 3, 2, 3, 4], False)]


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,shape,linearize", PER_FIELD_ONLY,
                         ids=[f"{m}-N{len(s)}-{'lin' if l else 'nolin'}" for m, s, l in PER_FIELD_ONLY])
def test_methods_without_a_fused_form(oracle, method, shape, linearize, kind):
    case, fields = _fields_case(method, kind, shape, np.float64, 3, seed=40 + len(shape), nobs=2000, linearize=linearize)
    want = _want(oracle, case, fields, True)
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused_table_bytes") == 0
        fs.set_option("fused", 1)  # "wherever the table exists": there is none
        host, dev = _eval_both(fs, case.obs)
        assert fs.last_path == "per_field" and not fs.kernel_name().startswith(FUSED_KERNEL)
        _assert_rows(host, want, ("host", method, shape))
        _assert_rows(dev, want, ("device", method, shape))
    finally:
        fs.close()


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "per_field"])
@pytest.mark.parametrize("kind,n,dtype,k", [("regular", 3, np.float64, 3), ("rectilinear", 2, np.float32, 5),
                                            ("rectilinear", 3, np.float64, 2), ("regular", 2, np.float64, 9)])
def test_batch_sizes_guards_and_row_stride(oracle, kind, n, dtype, k, fused):
    import torch

    for npts in (1, 63, 64, 65, 257, 100_003):
        case, fields = _fields_case("linear", kind, SHAPES[n], dtype, k, seed=npts % 97, nobs=npts)
        want = _want(oracle, case, fields, True)
        fs = _make(case, fields)
        try:
            fs.set_option("fused", fused)
            pad = 24
            sentinel = dtype(-12345.5)
            # host form: rows of a wider array (row stride = npts + 2 * pad), guard elements on both sides
            wide = np.full((k, npts + 2 * pad), sentinel, dtype=dtype)
            fs.eval_host(case.obs, wide[:, pad:pad + npts])
            assert fs.last_path == ("fused" if fused else "per_field")
            _assert_rows(wide[:, pad:pad + npts], want, ("host", npts))
            assert np.all(wide[:, :pad] == sentinel) and np.all(wide[:, pad + npts:] == sentinel), npts
            # device form, the same with an odd offset (rows not 16-byte aligned)
            off = 3
            twide = torch.full((k, npts + 2 * pad), float(sentinel), dtype=torch.float64 if dtype == np.float64 else torch.float32,
                               device="cuda:0")
            fs.eval_tensors(_tensors(case.obs), twide[:, off:off + npts])
            fs.finish()
            got = twide.cpu().numpy()
            _assert_rows(got[:, off:off + npts], want, ("device", npts))
            assert np.all(got[:, :off] == sentinel) and np.all(got[:, off + npts:] == sentinel), npts
        finally:
            fs.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("length", [5, 64, 65, 3000])
def test_rectilinear_axis_lengths(oracle, length, dtype):
    for shape in ([length, 9], [6, length], [length, 6, 5], [4, 5, length]):
        case, fields = _fields_case("linear", "rectilinear", shape, dtype, 3, seed=length % 89 + len(shape), nobs=4000)
        want = _want(oracle, case, fields, True)
        fs = _make(case, fields)
        try:
            fs.set_option("fused", 1)
            host, dev = _eval_both(fs, case.obs)
            assert fs.last_path == "fused" and fs.kernel_name().startswith(FUSED_KERNEL)
            _assert_rows(host, want, ("host", shape))
            _assert_rows(dev, want, ("device", shape))
        finally:
            fs.close()


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("shape", [[2, 2], [2, 9], [9, 2], [2, 9, 2], [7, 2, 5], [2, 2, 2]], ids=str)
def test_axes_of_exactly_two_points(oracle, shape, kind):
    for dtype in (np.float64, np.float32):
        case, fields = _fields_case("linear", kind, shape, dtype, 5, seed=sum(shape), nobs=1500)
        want = _want(oracle, case, fields, True)
        fs = _make(case, fields)
        try:
            fs.set_option("fused", 1)
            host, dev = _eval_both(fs, case.obs)
            assert fs.last_path == "fused"
            _assert_rows(host, want, ("host", shape, dtype))
            _assert_rows(dev, want, ("device", shape, dtype))
        finally:
            fs.close()


def test_set_created_from_a_cuda_tensor_and_from_a_sequence(oracle):
    import torch

    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, 4, seed=3)
    want = _want(oracle, case, fields, True)
    tvals = torch.from_numpy(fields.reshape(4, *SHAPES[3])).to("cuda:0")  # shape (K, *dims): borrowed, not copied
    for vals in (tvals, [fields[f] for f in range(4)], [tvals[f] for f in range(4)]):
        fs = _make(case, fields, vals=vals)
        try:
            host, dev = _eval_both(fs, case.obs)
            assert fs.last_path == "fused"
            _assert_rows(host, want, "host")
            _assert_rows(dev, want, "device")
        finally:
            fs.close()


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "per_field"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_failing_point_contract(oracle, dtype, fused):
    """A NaN at a known index of a regular grid: the same index from both forms, for every field; host rows written in
    front of it and untouched behind it (the reference's loop stops there)."""
    bad = 1234
    case, fields = _fields_case("linear", "regular", SHAPES[3], dtype, 3, seed=11, nobs=5000)
    case.obs[1][bad] = np.nan
    case.obs[2][bad + 700] = np.inf  # a later failure must not be the one reported
    head = [o[:bad] for o in case.obs]
    want = _want(oracle, case, fields, True, obs=head)
    fs = _make(case, fields)
    try:
        fs.set_option("fused", fused)
        for chunk in (0, 1000):  # one chunk, and chunks that end in front of / behind the failing point
            fs.set_option("host_chunk", chunk)
            sentinel = dtype(777.25)
            out = np.full((3, 5000), sentinel, dtype=dtype)
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
                fs.eval_host(case.obs, out)
            _assert_rows(out[:, :bad], want, ("host head", chunk))
            assert np.all(out[:, bad:] == sentinel), chunk
        fs.eval_tensors(_tensors(case.obs))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as err:
            fs.finish()
        assert err.value.first_bad_index == bad
        assert fs.last_path == ("fused" if fused else "per_field")
        # the status word is cleared: a clean batch afterwards is clean
        fs.eval_tensors(_tensors(head))
        fs.finish()
    finally:
        fs.close()


def test_graph_capture_and_side_stream(oracle):
    import torch

    npts = 50_001
    case, fields = _fields_case("linear", "rectilinear", SHAPES[3], np.float64, 5, seed=21, nobs=npts)
    fs = _make(case, fields)
    try:
        obs = [torch.zeros(npts, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        out = torch.zeros((5, npts), dtype=torch.float64, device="cuda:0")
        side = torch.cuda.Stream()
        for d in range(3):
            obs[d].copy_(torch.from_numpy(case.obs[d]))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            fs.eval_tensors(obs, out)  # torch's current stream is the side stream
        fs.finish()
        assert fs.last_path == "fused"
        _assert_rows(out.cpu().numpy(), _want(oracle, case, fields, True), "side stream")
        out.zero_()
        torch.cuda.synchronize()
        fs.eval_tensors(obs, out, stream=side)  # the stream given explicitly
        fs.finish(side)
        _assert_rows(out.cpu().numpy(), _want(oracle, case, fields, True), "stream=")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fs.eval_tensors(obs, out)
        assert fs.last_path == "fused"
        rng = np.random.default_rng(77)
        for rep in range(2):
            host = [rng.uniform(-1.1, 1.1, npts) for _ in range(3)]
            for d in range(3):
                obs[d].copy_(torch.from_numpy(host[d]))
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            _assert_rows(out.cpu().numpy(), _want(oracle, case, fields, True, obs=host), ("replay", rep))
        fs.finish()
    finally:
        fs.close()


def test_table_refused_by_the_memory_rule(oracle, monkeypatch):
    """The fused table is built only while it fits the budget (a quarter of the free device memory; the test-only
    INTERPN_HIP_FIELDS_TABLE_BUDGET lowers it): without it the set evaluates per field, which is not an error."""
    import interpn_amd

    case, fields = _fields_case("linear", "regular", SHAPES[3], np.float64, 4, seed=2)
    want = _want(oracle, case, fields, True)
    _per_line, _lines, nbytes = interpn_amd.fields_layout(np.float64, SHAPES[3], 4)
    for budget, has_table in ((nbytes, True), (nbytes - 1, False)):
        monkeypatch.setenv("INTERPN_HIP_FIELDS_TABLE_BUDGET", str(budget))
        fs = _make(case, fields)
        try:
            assert fs.get_option("fused_table_bytes") == (nbytes if has_table else 0)
            fs.set_option("fused", 1)
            host, dev = _eval_both(fs, case.obs)
            assert fs.last_path == ("fused" if has_table else "per_field")
            _assert_rows(host, want, ("host", budget))
            _assert_rows(dev, want, ("device", budget))
        finally:
            fs.close()
    monkeypatch.setenv("INTERPN_HIP_FIELDS_FUSED", "0")
    monkeypatch.delenv("INTERPN_HIP_FIELDS_TABLE_BUDGET")
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused") == 0 and fs.get_option("fused_table_bytes") == 0
    finally:
        fs.close()


def test_interpn_fields_both_layouts(oracle):
    import torch

    import interpn_amd

    case, fields = _fields_case("linear", "regular", SHAPES[2], np.float64, 3, seed=9, nobs=600)
    want = _want(oracle, case, fields, True)
    obs2d = [o.reshape(20, 30) for o in case.obs]
    vals_first = fields.reshape(3, *SHAPES[2])
    got = interpn_amd.interpn_fields(obs2d, case.grids, vals_first, assume_regular=True)
    assert got.shape == (3, 20, 30)
    _assert_rows(got.reshape(3, -1), want, "fields first")
    vals_last = np.ascontiguousarray(np.moveaxis(vals_first, 0, -1))  # scipy's (*dims, K)
    got = interpn_amd.interpn_fields(obs2d, case.grids, vals_last, field_axis=-1, assume_regular=True)
    assert got.shape == (20, 30, 3)
    _assert_rows(np.moveaxis(got, -1, 0).reshape(3, -1), want, "fields last")
    out = np.zeros((3, 20, 30))
    assert interpn_amd.interpn_fields(obs2d, case.grids, vals_first, out=out, assume_regular=True) is out
    _assert_rows(out.reshape(3, -1), want, "out=")
    tobs = [torch.from_numpy(o).to("cuda:0") for o in obs2d]
    got = interpn_amd.interpn_fields(tobs, case.grids, torch.from_numpy(vals_last).to("cuda:0"), field_axis=-1, assume_regular=True,
                                     check_bounds=False)
    assert tuple(got.shape) == (20, 30, 3)
    _assert_rows(np.moveaxis(got.cpu().numpy(), -1, 0).reshape(3, -1), want, "tensors, fields last")
    inside = [np.clip(o, -1.0, 1.0) for o in obs2d]
    interpn_amd.interpn_fields(inside, case.grids, vals_first, assume_regular=True, check_bounds=True)
    with pytest.raises(ValueError, match="violate interpolator bounds"):
        interpn_amd.interpn_fields([torch.from_numpy(o).to("cuda:0") for o in obs2d], case.grids, vals_first, assume_regular=True,
                                   check_bounds=True)


AUTO = [  # shape, dtype, K, points, path
    ([64, 64, 64], np.float64, 4, 20_000_000, "per_field"),   # two fields per line against the sweep kernel on an L2-sized field
    ([64, 64, 64], np.float64, 4, 1_000_000, "fused"),        # ... below the sweep kernel's batch size
    ([128, 128, 128], np.float64, 2, 20_000_000, "fused"),    # ... a field beyond the L2
    ([64, 64, 64], np.float32, 4, 20_000_000, "fused"),       # four fields per line
    ([64, 64, 64], np.float32, 2, 1_000_000, "per_field"),    # half-empty lines
    ([300, 200], np.float64, 2, 1_000_000, "per_field"),
    ([300, 200], np.float64, 4, 1_000_000, "fused"),
    ([300, 200], np.float64, 1, 1_000_000, "per_field"),
    ([40, 30, 20], np.float64, 3, 100_000, "fused"),          # 3 of 4 slots
]


@pytest.mark.parametrize("shape,dtype,k,npts,path", AUTO, ids=[f"{'x'.join(map(str, a[0]))}-{np.dtype(a[1]).name}-K{a[2]}-{a[3]}" for a in AUTO])
def test_automatic_path(shape, dtype, k, npts, path):
    """What fused = -1 does for the classes measured in profiles/fields_bench.json, and that the
    choice does not change a bit of the result."""
    import torch

    case, fields = _fields_case("linear", "regular", shape, dtype, k, seed=k, nobs=64)
    fs = _make(case, fields)
    try:
        assert fs.get_option("fused") == -1
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(npts % 1000 + k)
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        obs = [torch.rand(npts, dtype=tdt, device="cuda:0", generator=gen) * 2.1 - 1.05 for _ in shape]
        got = fs.eval_tensors(obs)
        fs.finish()
        assert fs.last_path == path, (fs.last_path, fs.kernel_name())
        assert fs.kernel_name().startswith(FUSED_KERNEL) == (path == "fused")
        if shape == [64, 64, 64] and dtype == np.float64 and path == "per_field":
            assert fs.kernel_name().startswith("interpn::k_linear_sweep<"), fs.kernel_name()
        fs.set_option("fused", 1 if path == "per_field" else 0)
        other = fs.eval_tensors(obs)
        fs.finish()
        assert fs.last_path != path
        assert torch.equal(got.view(torch.int64 if dtype == np.float64 else torch.int32),
                           other.view(torch.int64 if dtype == np.float64 else torch.int32))
    finally:
        fs.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_full_size_parity(oracle, dtype):
    """64^3, K = 4, 1e7 points: every row against the oracle, fused and per-field."""
    npts = 10_000_000
    case, fields = _fields_case("linear", "regular", [64, 64, 64], dtype, 4, seed=64, nobs=npts)
    want = _want(oracle, case, fields, True)
    fs = _make(case, fields)
    try:
        obs = _tensors(case.obs)
        fs.set_option("fused", 1)
        got = fs.eval_tensors(obs)
        fs.finish()
        assert fs.last_path == "fused" and fs.kernel_name().startswith(FUSED_KERNEL)
        _assert_rows(got.cpu().numpy(), want, "fused")
        fs.set_option("fused", 0)
        got0 = fs.eval_tensors(obs)
        fs.finish()
        assert fs.last_path == "per_field"
        _assert_rows(got0.cpu().numpy(), want, "per field")
    finally:
        fs.close()
