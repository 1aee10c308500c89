"""Field sets on a lattice on the GPU (interpn_hip_fields_eval_lattice_*): every field of every result is compared BIT FOR
BIT, at the same fma flavour, with (a) the oracle run on that field alone at the `np.meshgrid(..., indexing="ij")`-expanded
points and (b) `Interpolator.eval_lattice` of that field alone — on the fused path (interpn::k_lattice_axes +
interpn::k_lattice_fields_rows) and on the per-field one, in both result layouts.

Wall time of the whole file on one MI355X: see DESIGN.md section 16.
"""

import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import run_oracle, synthetic_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS_KERNEL = "interpn::k_lattice_fields_rows<"
SHAPES = {2: [37, 53], 3: [17, 12, 23]}
LATTICE = {2: [41, 67], 3: [11, 13, 71]}
LAYOUTS = (0, -1)  # field_axis
SENTINEL = -777.25
WAVES, CAP = 4, 8
DEFAULT_BUDGET = 160 * 1024 // 8


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_bits(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (ctx, len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


def _fields_case(method, kind, shape, dtype, k, seed, linearize=False):
    case = synthetic_case(method, kind, len(shape), shape, 1, seed, dtype=dtype, linearize=linearize, specials=False)
    rng = np.random.default_rng(1000 + seed)
    fields = np.stack([rng.uniform(-1.0, 1.0, case.vals.size).astype(dtype) for _ in range(k)])
    return case, fields


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


def _want(oracle, case, fields, axes, fma=True):
    """Reference (a): the oracle per field on the expanded points, shape (K, *m)."""
    points = _expand(axes)
    rows = []
    for f in range(fields.shape[0]):
        c = dataclasses.replace(case, vals=fields[f], obs=points)
        rows.append(run_oracle(oracle, c, fma=fma, out=np.zeros(points[0].size, dtype=fields.dtype)))
    return np.stack(rows).reshape((fields.shape[0],) + tuple(a.size for a in axes))


def _make(case, fields, fma=None):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Fields.regular(case.method, case.dims, case.starts, case.steps, fields, linearize_extrapolation=case.linearize,
                                          dtype=fields.dtype, fma=fma)
    return interpn_amd.Fields.rectilinear(case.method, case.grids, fields, linearize_extrapolation=case.linearize, dtype=fields.dtype,
                                          fma=fma)


def _make_one(case, vals, fma=None):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, vals,
                                                linearize_extrapolation=case.linearize, dtype=vals.dtype, fma=fma)
    return interpn_amd.Interpolator.rectilinear(case.method, case.grids, vals, linearize_extrapolation=case.linearize,
                                                dtype=vals.dtype, fma=fma)


def _single(case, fields, axes, fma=None, lattice=None):
    """Reference (b): `Interpolator.eval_lattice_tensors` of every field alone, shape (K, *m)."""
    rows = []
    ax_t = _tensors(axes)
    for f in range(fields.shape[0]):
        it = _make_one(case, fields[f], fma)
        try:
            if lattice is not None:
                it.set_option("lattice", lattice)
            res = it.eval_lattice_tensors(ax_t)
            it.finish()
            rows.append(res.cpu().numpy())
        finally:
            it.close()
    return np.stack(rows)


def _tensors(arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def _field_major(res, field_axis):
    """A result of either layout as (K, *m)."""
    res = res.cpu().numpy() if hasattr(res, "cpu") else np.asarray(res)
    return res if field_axis == 0 else np.ascontiguousarray(np.moveaxis(res, -1, 0))


def _eval(fs, axes, field_axis, **kw):
    res = fs.eval_lattice_tensors(_tensors(axes), field_axis=field_axis, **kw)
    fs.finish()
    m = tuple(a.size for a in axes)
    assert tuple(res.shape) == ((fs.nfields,) + m if field_axis == 0 else m + (fs.nfields,))
    return _field_major(res, field_axis)


def _eval_host(fs, axes, field_axis, out=None):
    res = fs.eval_lattice_host(axes, out, field_axis=field_axis)
    m = tuple(a.size for a in axes)
    assert res.shape == ((fs.nfields,) + m if field_axis == 0 else m + (fs.nfields,))
    return _field_major(res, field_axis)


def _kernel(dtype, method, n, kind, fma, field_axis):
    return (f"{ROWS_KERNEL}{'double' if dtype == np.float64 else 'float'}, {0 if method == 'linear' else 1}, {n}, "
            f"{'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}, {'true' if field_axis else 'false'}>")


def _round16(v):
    return (v + 15) // 16 * 16


def _wave_bytes(n_last, elem, g, field_axis):
    return g * _round16(n_last * elem) + (_round16(64 * (g | 1) * elem) if field_axis else 0)


def _group(n_last, elem, k, field_axis, budget=DEFAULT_BUDGET):
    """G by the formula of lattice.h."""
    g = 0
    while g < min(k, CAP) and WAVES * _wave_bytes(n_last, elem, g + 1, field_axis) <= budget:
        g += 1
    return g


# ---- 1. every fused instantiation -----------------------------------------------------------------------------------------
FUSED = [("linear", False), ("cubic", False), ("cubic", True)]


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("method,linearize", FUSED, ids=["linear", "cubic-nolin", "cubic-lin"])
def test_fused_instantiations(oracle, method, linearize, n, kind, dtype, fma):
    k = 3
    case, fields = _fields_case(method, kind, SHAPES[n], dtype, k, seed=3 * n + len(method), linearize=linearize)
    axes = _axes(case, LATTICE[n], seed=100 + n)
    want = _want(oracle, case, fields, axes, fma)
    _assert_bits(_single(case, fields, axes, fma, lattice=1), want, ("single handles vs oracle", method, n, kind))
    fs = _make(case, fields, fma)
    try:
        fs.set_option("lattice", 1)
        assert fs.last_lattice_path is None
        for field_axis in LAYOUTS:
            dev = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused"
            assert fs.kernel_name() == _kernel(dtype, method, n, kind, fma, field_axis), fs.kernel_name()
            assert fs.get_option("last_lattice_group") == k
            host = _eval_host(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused"
            _assert_bits(dev, want, ("fused device", method, n, kind, field_axis))
            _assert_bits(host, want, ("fused host", method, n, kind, field_axis))
    finally:
        fs.close()


# ---- 2. field counts and groups -------------------------------------------------------------------------------------------
GROUP_CASES = [("linear", "regular", [9, 7, 32], [6, 5, 70], np.float64), ("cubic", "rectilinear", [37, 64], [23, 70], np.float32)]
GROUP_IDS = ["linear3-f64", "cubic2-f32"]


@pytest.fixture(scope="module")
def group_refs(oracle):
    """The references of the nine-field sets of GROUP_CASES, computed once: the first K fields serve every smaller K."""
    refs = {}
    for name, (method, kind, shape, lens, dtype) in zip(GROUP_IDS, GROUP_CASES):
        case, fields = _fields_case(method, kind, shape, dtype, CAP + 1, seed=17)
        axes = _axes(case, lens, seed=21)
        refs[name] = (case, fields, axes, _want(oracle, case, fields, axes))
    return refs


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, CAP + 1])
@pytest.mark.parametrize("name", GROUP_IDS)
def test_field_counts_at_the_default_budget(group_refs, name, k):
    case, fields, axes, want = group_refs[name]
    elem = fields.dtype.itemsize
    fs = _make(case, fields[:k])
    try:
        fs.set_option("lattice", 1)
        for field_axis in LAYOUTS:
            got = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused"
            g = _group(case.dims[-1], elem, k, field_axis)
            assert 1 <= g <= min(k, CAP) and fs.get_option("last_lattice_group") == g, (g, fs.get_option("last_lattice_group"))
            _assert_bits(got, want[:k], ("K", name, k, field_axis))
            _assert_bits(_eval_host(fs, axes, field_axis), want[:k], ("K host", name, k, field_axis))
    finally:
        fs.close()


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("name", GROUP_IDS)
def test_groups_smaller_than_the_set(group_refs, name, g):
    """K = 8 with the LDS budget set so that G = 1, 2, 3: several passes per row, and for G = 3 a short last pass."""
    case, fields, axes, want = group_refs[name]
    elem, k = fields.dtype.itemsize, 8
    fs = _make(case, fields[:k])
    try:
        fs.set_option("lattice", 1)
        for field_axis in LAYOUTS:
            kb = next(kb for kb in range(1, 61) if _group(case.dims[-1], elem, k, field_axis, kb * 1024) == g)
            fs.set_option("axis_lds_kb", kb)
            got = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused" and fs.get_option("last_lattice_group") == g
            _assert_bits(got, want[:k], ("G", name, g, field_axis))
    finally:
        fs.close()


# ---- 3. axis lengths and guards -------------------------------------------------------------------------------------------
LENGTH_CASES = [("linear", "regular", 3, np.float64), ("cubic", "rectilinear", 2, np.float32)]


@pytest.mark.parametrize("other", [1, 2, 7])
@pytest.mark.parametrize("last", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("method,kind,n,dtype", LENGTH_CASES, ids=["linear3-regular-f64", "cubic2-rectilinear-f32"])
def test_axis_lengths_and_guards(oracle, method, kind, n, dtype, last, other):
    import torch

    k = 3
    lens = [other] * (n - 1) + [last]
    count = int(np.prod(lens))
    case, fields = _fields_case(method, kind, SHAPES[n], dtype, k, seed=11)
    axes = _axes(case, lens, seed=last + other)
    want = _want(oracle, case, fields, axes)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 1)
        ax_t = _tensors(axes)
        # field-major: out_stride = prod(m) + 5, one more row behind the K fields
        buf = torch.full((k + 1, count + 5), SENTINEL, dtype=tdt, device="cuda:0")
        fs.eval_lattice_tensors(ax_t, buf[:k, :count], field_axis=0)
        fs.finish()
        assert fs.last_lattice_path == "fused"
        got = buf.cpu().numpy()
        _assert_bits(got[:k, :count].reshape(want.shape), want, ("field-major", lens))
        assert (got[:k, count:] == SENTINEL).all() and (got[k] == SENTINEL).all()
        # fields-last: out_stride = K + 3, buf[:, :K] of a wider tensor, one more row behind the points
        buf = torch.full((count + 1, k + 3), SENTINEL, dtype=tdt, device="cuda:0")
        fs.eval_lattice_tensors(ax_t, buf[:count, :k], field_axis=-1)
        fs.finish()
        assert fs.last_lattice_path == "fused"
        got = buf.cpu().numpy()
        _assert_bits(np.ascontiguousarray(got[:count, :k].T).reshape(want.shape), want, ("fields-last", lens))
        assert (got[:count, k:] == SENTINEL).all() and (got[count] == SENTINEL).all()
        # the same views on the host
        hbuf = np.full((k + 1, count + 5), SENTINEL, dtype=dtype)
        fs.eval_lattice_host(axes, hbuf[:k, :count], field_axis=0)
        _assert_bits(hbuf[:k, :count].reshape(want.shape), want, ("host field-major", lens))
        assert (hbuf[:k, count:] == SENTINEL).all() and (hbuf[k] == SENTINEL).all()
        hbuf = np.full((count + 1, k + 3), SENTINEL, dtype=dtype)
        fs.eval_lattice_host(axes, hbuf[:count, :k], field_axis=-1)
        _assert_bits(np.ascontiguousarray(hbuf[:count, :k].T).reshape(want.shape), want, ("host fields-last", lens))
        assert (hbuf[:count, k:] == SENTINEL).all() and (hbuf[count] == SENTINEL).all()
    finally:
        fs.close()


# ---- 4. per-field path ----------------------------------------------------------------------------------------------------
PER_FIELD = [  # method, shape, lattice, options, whether a fused result exists
    ("linear", [17, 12, 23], [11, 13, 71], {"lattice": 0}, True),
    ("cubic", [37, 53], [41, 67], {"lattice": 0}, True),
    ("nearest", [9, 7, 11], [6, 5, 70], {"lattice": 1}, False),
    ("linear", [301], [777], {"lattice": 1}, False),
    ("cubic", [5, 6, 4, 7], [4, 3, 5, 33], {"lattice": 1}, False),
    ("linear", [9, 7, 33], [6, 5, 70], {"lattice": 1, "axis_lds_kb": 1}, False),  # four lines of 32 f64 fit 1 KiB, of 33 do not
]


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,shape,lens,options,both", PER_FIELD,
                         ids=["lattice0-linear3", "lattice0-cubic2", "nearest", "N1", "N4", "beyond-budget"])
def test_per_field_path(oracle, method, shape, lens, options, both, kind):
    k = 3
    case, fields = _fields_case(method, kind, shape, np.float64, k, seed=len(shape) + 5)
    axes = _axes(case, lens, seed=13)
    want = _want(oracle, case, fields, axes)
    _assert_bits(_single(case, fields, axes), want, ("single handles vs oracle", method, shape))
    fs = _make(case, fields)
    try:
        for name, value in options.items():
            fs.set_option(name, value)
        fs.set_option("points_slice", max(256, 3 * int(np.prod(lens[1:]))))  # fields-last: several slices of leading indices
        for field_axis in LAYOUTS:
            got = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "per_field"
            assert fs.get_option("last_lattice_path") == 1
            _assert_bits(got, want, ("per field", method, shape, field_axis))
            _assert_bits(_eval_host(fs, axes, field_axis), want, ("per field host", method, shape, field_axis))
            if both:
                fs.set_option("lattice", 1)
                fused = _eval(fs, axes, field_axis)
                assert fs.last_lattice_path == "fused"
                _assert_bits(fused, got, ("fused vs per field", method, field_axis))
                fs.set_option("lattice", 0)
    finally:
        fs.close()


def test_line_at_the_budget_is_fused(oracle):
    """The neighbour of the last PER_FIELD case: 32 f64 columns fill 1 KiB with four lines, so the field-major form is fused
    with G = 1 and the fields-last form, which needs a tile on top, goes per field."""
    k = 2
    case, fields = _fields_case("linear", "regular", [9, 7, 32], np.float64, k, seed=8)
    axes = _axes(case, [6, 5, 70], seed=13)
    want = _want(oracle, case, fields, axes)
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 1)
        fs.set_option("axis_lds_kb", 1)
        _assert_bits(_eval(fs, axes, 0), want, "field-major")
        assert fs.last_lattice_path == "fused" and fs.get_option("last_lattice_group") == 1
        _assert_bits(_eval(fs, axes, -1), want, "fields-last")
        assert fs.last_lattice_path == "per_field"
    finally:
        fs.close()


# ---- 5. failing points on regular grids -----------------------------------------------------------------------------------
def _formula(lens, bad):
    """min over bad (d, j) of j * prod(lens[e], e > d)."""
    return min(j * int(np.prod(lens[d + 1:], dtype=object)) for d, j in bad)


BAD_SETS = [[(0, 5)], [(1, 3)], [(2, 7)], [(0, 6), (2, 2)], [(2, 0)]]
FAIL_LENS = [9, 8, 45]


@pytest.fixture(scope="module")
def failing_refs(oracle):
    refs = {}
    for method in ("linear", "cubic"):
        case, fields = _fields_case(method, "regular", [17, 12, 23], np.float64, 3, seed=23)
        clean = _axes(case, FAIL_LENS, seed=9)
        refs[method] = (case, fields, clean, _want(oracle, case, fields, clean))
    return refs


@pytest.mark.parametrize("value", [np.nan, np.inf, 1e300], ids=["nan", "inf", "1e300"])
@pytest.mark.parametrize("bad", BAD_SETS, ids=["axis0", "middle", "last", "two", "first-point"])
@pytest.mark.parametrize("method,mode", [("linear", 1), ("cubic", 1), ("linear", 0)], ids=["linear-fused", "cubic-fused", "linear-per-field"])
def test_failing_points_on_regular_grids(failing_refs, method, mode, bad, value):
    lens = FAIL_LENS
    case, fields, clean, want = failing_refs[method]
    k, count = fields.shape[0], int(np.prod(lens))
    axes = [a.copy() for a in clean]
    for d, j in bad:
        axes[d][j] = value
    first = _formula(lens, bad)
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", mode)
        fs.set_option("points_slice", 2 * lens[1] * lens[2])  # per-field, fields-last: five slices of leading indices
        fs.set_option("host_chunk", 2 * lens[1] * lens[2] + 7)  # host form: five chunks
        for field_axis in LAYOUTS:
            fs.eval_lattice_tensors(_tensors(axes), field_axis=field_axis)
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
                fs.finish()
            assert e.value.first_bad_index == first, (e.value.first_bad_index, first, field_axis)
            assert fs.last_lattice_path == ("fused" if mode else "per_field")
            # host form: exactly the prefix of every field, the rest of `out` as it was
            out = np.full([k] + lens if field_axis == 0 else lens + [k], SENTINEL)
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
                fs.eval_lattice_host(axes, out, field_axis=field_axis)
            assert e.value.first_bad_index == first
            flat = _field_major(out, field_axis).reshape(k, count)
            _assert_bits(flat[:, :first], want.reshape(k, count)[:, :first], ("prefix", bad, field_axis))
            assert (flat[:, first:] == SENTINEL).all()
            # the status words are cleared: a clean lattice afterwards is clean
            _assert_bits(_eval(fs, clean, field_axis), want, ("clean after failure", bad, field_axis))
    finally:
        fs.close()


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "per_field"])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_rectilinear_grids_propagate_nan(oracle, method, mode):
    lens = [9, 8, 45]
    case, fields = _fields_case(method, "rectilinear", [17, 12, 23], np.float64, 2, seed=29)
    axes = _axes(case, lens, seed=4)
    axes[0][2] = np.nan
    axes[2][31] = np.nan
    expect_nan = np.zeros([2] + lens, dtype=bool)
    expect_nan[:, 2, :, :] = True
    expect_nan[:, :, :, 31] = True
    ref = _single(case, fields, axes, lattice=mode)
    assert np.array_equal(np.isnan(ref), expect_nan)
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", mode)
        for field_axis in LAYOUTS:
            got = _eval(fs, axes, field_axis)  # finish() inside: no failure reported
            assert np.array_equal(np.isnan(got), expect_nan)
            _assert_bits(got[~expect_nan], ref[~expect_nan], ("beside the NaN planes", field_axis))
            host = _eval_host(fs, axes, field_axis)
            assert np.array_equal(np.isnan(host), expect_nan)
            _assert_bits(host[~expect_nan], ref[~expect_nan], ("host", field_axis))
    finally:
        fs.close()


# ---- 6. streams, reserve, capture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_axis", LAYOUTS, ids=["field-major", "fields-last"])
@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "per_field"])
def test_streams_and_reserve(oracle, mode, field_axis):
    import torch

    import interpn_amd

    lens = [12, 9, 130]
    k = 3
    case, fields = _fields_case("linear", "rectilinear", SHAPES[3], np.float64, k, seed=31)
    axes = [_axes(case, lens, seed=6), _axes(case, lens, seed=7)]
    want = [_want(oracle, case, fields, a) for a in axes]
    shape = [k] + lens if field_axis == 0 else lens + [k]
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", mode)
        # no_alloc without a reserved block: the out-of-memory status, not a silent allocation and not another failure
        with pytest.raises(interpn_amd._lib.InterpnHipError, match="[Oo]ut of memory|memory"):
            fs.eval_lattice_tensors(_tensors(axes[0]), field_axis=field_axis, no_alloc=True)
        ax0 = _tensors(axes[0])
        scratch = torch.zeros(shape, dtype=torch.float64, device="cuda:0")
        vp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ax0])
        m = (ctypes.c_size_t * 3)(*lens)
        stride = int(np.prod(lens)) if field_axis == 0 else k
        st = interpn_amd._lib.load().interpn_hip_fields_eval_lattice_device(
            fs._h, vp, m, 3, ctypes.c_void_p(scratch.data_ptr()), stride, 0 if field_axis == 0 else 1, None, interpn_amd._lib.EVAL_NO_ALLOC,
            None)
        assert st == 35, st  # INTERPN_HIP_ERR_OUT_OF_MEMORY
        torch.cuda.synchronize()
        fs.reserve_lattice(lens, 2)
        allocs = fs.get_option("scratch_allocs")
        assert allocs >= 1
        _assert_bits(_eval(fs, axes[0], field_axis, no_alloc=True), want[0], "no_alloc after reserve")
        # two side streams at once
        ax_t = [_tensors(a) for a in axes]
        outs = [torch.zeros(shape, dtype=torch.float64, device="cuda:0") for _ in range(2)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for rep in range(3):
            for i in range(2):
                fs.eval_lattice_tensors(ax_t[i], outs[i], field_axis=field_axis, stream=streams[i], no_alloc=True)
        fs.finish()
        assert fs.get_option("scratch_allocs") == allocs
        for i in range(2):
            _assert_bits(_field_major(outs[i], field_axis), want[i], ("side stream", i))
    finally:
        fs.close()


@pytest.mark.parametrize("field_axis", LAYOUTS, ids=["field-major", "fields-last"])
def test_fused_evaluation_in_a_graph(oracle, field_axis):
    """One fused evaluation (two kernels on one stream: a single-branch graph), replayed on new axis contents."""
    import torch

    lens = [12, 9, 130]
    k = 3
    case, fields = _fields_case("cubic", "regular", SHAPES[3], np.float64, k, seed=37)
    axes = _axes(case, lens, seed=6)
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 1)
        fs.reserve_lattice(lens, 1)
        ax_t = _tensors(axes)
        out = torch.zeros([k] + lens if field_axis == 0 else lens + [k], dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fs.eval_lattice_tensors(ax_t, out, field_axis=field_axis)
        assert fs.last_lattice_path == "fused"
        for rep in range(2):
            fresh = _axes(case, lens, seed=50 + rep)
            for d in range(3):
                ax_t[d].copy_(torch.from_numpy(fresh[d]))
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            got = _field_major(out, field_axis)
            _assert_bits(got, _eval(fs, fresh, field_axis), ("replay vs eager", rep))
            _assert_bits(got, _want(oracle, case, fields, fresh), ("replay vs oracle", rep))
        fs.finish()
    finally:
        fs.close()


# ---- 7. one-call form -----------------------------------------------------------------------------------------------------
def _exact_grids(kind, shape, rng):
    grids = []
    for d, n in enumerate(shape):
        g = -1.0 + 0.125 * np.arange(n)  # exactly equal spacings: the one-call forms take the grid for regular
        if kind == "rectilinear":
            g[1:-1] += rng.uniform(-0.03, 0.03, n - 2)
        grids.append(g)
    return grids


@pytest.mark.parametrize("method", ["linear", "cubic", "nearest"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_interpn_fields_lattice_entry_point(kind, method):
    import torch

    import interpn_amd

    rng = np.random.default_rng(41)
    shape, lens, k = [9, 12, 17], [6, 5, 70], 3
    grids = _exact_grids(kind, shape, rng)
    assert interpn_amd._check_regular(grids) == (kind == "regular")
    vals = rng.uniform(-1, 1, [k] + shape)
    axes = [np.sort(rng.uniform(g[0], g[-1], m)) for g, m in zip(grids, lens)]
    axes[1][2] = grids[1][-1] + 0.5
    want = np.stack([interpn_amd.interpn_lattice(axes, grids, vals[f], method=method) for f in range(k)])
    got = interpn_amd.interpn_fields_lattice(axes, grids, vals, method=method)
    _assert_bits(got, want, ("fields first", kind, method))
    vals_last = np.ascontiguousarray(np.moveaxis(vals, 0, -1))
    want_last = np.ascontiguousarray(np.moveaxis(want, 0, -1))
    got = interpn_amd.interpn_fields_lattice(axes, grids, vals_last, method=method, field_axis=-1)
    _assert_bits(got, want_last, ("fields last", kind, method))
    out = np.zeros(lens + [k])
    assert interpn_amd.interpn_fields_lattice(axes, grids, vals_last, method=method, field_axis=-1, out=out) is out
    _assert_bits(out, want_last, "out=")
    for field_axis, v, w in ((0, vals, want), (-1, vals_last, want_last)):
        got_t = interpn_amd.interpn_fields_lattice(_tensors(axes), grids, torch.from_numpy(v).to("cuda:0"), method=method,
                                                   field_axis=field_axis)
        assert isinstance(got_t, torch.Tensor) and got_t.is_cuda
        _assert_bits(got_t.cpu().numpy(), w, ("torch input", field_axis))
        got_t = interpn_amd.interpn_fields_lattice(_tensors(axes), grids, v, method=method, field_axis=field_axis)
        _assert_bits(got_t.cpu().numpy(), w, ("torch axes, numpy vals", field_axis))


def test_eval_lattice_dispatch_and_argument_errors_with_a_set(oracle):
    import interpn_amd

    k, lens = 2, [5, 9]
    case, fields = _fields_case("linear", "regular", [9, 11], np.float64, k, seed=3)
    axes = _axes(case, lens, seed=1)
    want = _want(oracle, case, fields, axes)
    fs = _make(case, fields)
    try:
        _assert_bits(fs.eval_lattice(axes), want, "numpy")
        res = fs.eval_lattice(_tensors(axes), field_axis=-1)
        fs.finish()
        _assert_bits(_field_major(res, -1), want, "torch")
        lib, h = interpn_amd._lib.load(), fs._h
        vp = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in _tensors(axes)])
        m = (ctypes.c_size_t * 2)(*lens)
        dev = lib.interpn_hip_fields_eval_lattice_device
        assert dev(h, vp, m, 2, ctypes.c_void_p(res.data_ptr()), 44, 0, None, 0, None) == 32   # stride below prod(m) = 45
        assert dev(h, vp, m, 2, ctypes.c_void_p(res.data_ptr()), 1, 1, None, 0, None) == 32    # stride below K
        assert dev(h, vp, m, 2, ctypes.c_void_p(res.data_ptr()), 45, 3, None, 0, None) == 32   # no such layout
        assert dev(h, vp, m, 2, None, 45, 0, None, 0, None) == 32
        assert dev(h, vp, m, 2, ctypes.c_void_p(res.data_ptr()), 45, 0, None, 2, None) == 32   # unknown flag
        assert dev(h, vp, m, 3, ctypes.c_void_p(res.data_ptr()), 45, 0, None, 0, None) == 1    # "Dimension mismatch"
        # the order of the checks: the lattice's own come first, the layout value and the strides behind them
        assert dev(h, vp, m, 3, ctypes.c_void_p(res.data_ptr()), 1, 3, None, 0, None) == 1
        assert dev(h, None, m, 2, ctypes.c_void_p(res.data_ptr()), 1, 3, None, 0, None) == 32
        m0 = (ctypes.c_size_t * 2)(0, 9)
        assert dev(h, vp, m0, 2, None, 0, 3, None, 0, None) == 0                               # an empty axis, whatever the layout says
        host = lib.interpn_hip_fields_eval_lattice_host
        assert host(h, vp, m, 3, ctypes.c_void_p(res.data_ptr()), 1, 3, None) == 1
        assert host(h, vp, m, 2, ctypes.c_void_p(res.data_ptr()), 45, 3, None) == 32
        assert host(h, vp, m, 2, ctypes.c_void_p(res.data_ptr()), 1, 1, None) == 32
        m0 = (ctypes.c_size_t * 2)(0, 9)
        assert dev(h, vp, m0, 2, None, 0, 0, None, 0, None) == 0                               # an empty axis: nothing to do
    finally:
        fs.close()


# ---- 8. one moderate case -------------------------------------------------------------------------------------------------
def test_moderate_regrid(oracle):
    """3-D linear f64 64^3, K = 3, onto 96 x 96 x 200, fields-last, automatic mode: 9216 rows (>= 4 x 256) and a last grid
    axis of 64 <= 4 x 200, G = K = 3 — the rule takes the fused path.  Sampled against the oracle, compared as a whole with
    the per-field path."""
    import interpn_amd

    k, shape, lens = 3, [64, 64, 64], [96, 96, 200]
    case, fields = _fields_case("linear", "regular", shape, np.float64, k, seed=43)
    axes = [np.sort(a) for a in _axes(case, lens, seed=44)]
    assert interpn_amd.fields_lattice_plan(np.float64, "linear", shape, lens, k, field_axis=-1)[:2] == ("fused", 3)
    fs = _make(case, fields)
    try:
        got = _eval(fs, axes, -1)
        assert fs.last_lattice_path == "fused" and fs.get_option("last_lattice_group") == 3
        fs.set_option("lattice", 0)
        per_field = _eval(fs, axes, -1)
        assert fs.last_lattice_path == "per_field"
        _assert_bits(got, per_field, "fused vs per field")
        rng = np.random.default_rng(45)
        idx = [rng.integers(0, m, 200000) for m in lens]
        points = [np.ascontiguousarray(axes[d][idx[d]]) for d in range(3)]
        for f in range(k):
            c = dataclasses.replace(case, vals=fields[f], obs=points)
            want = run_oracle(oracle, c, fma=True, out=np.zeros(points[0].size))
            _assert_bits(got[f][idx[0], idx[1], idx[2]], want, ("sample vs oracle", f))
    finally:
        fs.close()
