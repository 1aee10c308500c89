"""Field-set gradients on a lattice on the GPU (interpn_hip_fields_eval_lattice_grad_*): every value and every Jacobian
element is compared BIT FOR BIT, at the same fma flavour, with code that predates the kernel — the values with
`Fields.eval_lattice_*`, and values and Jacobian with `Interpolator.eval_lattice_grad_*` of every field alone — on the fused
path (interpn::k_lattice_axes + interpn::k_lattice_fields_grad_rows) and on the per-field one, in both result layouts.

Wall time of the whole file (158 cases) on one MI355X: 3.7 s, 6 s with the interpreter's start.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import synthetic_case  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS_KERNEL = "interpn::k_lattice_fields_grad_rows<"
SHAPES = {2: [9, 8], 3: [7, 6, 5]}
LATTICE = {2: [41, 67], 3: [11, 13, 71]}
LAYOUTS = (0, -1)  # field_axis
SENTINEL = -777.25
WAVES, CAP = 4, 8
DEFAULT_BUDGET = 20 * 1024


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_bits(got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (ctx, len(bad), bad[:5].tolist(), [(got[tuple(b)], want[tuple(b)]) for b in bad[:5]])


def _assert_pair(got, want, ctx):
    _assert_bits(got[0], want[0], (ctx, "values"))
    _assert_bits(got[1], want[1], (ctx, "jacobian"))


def _fields_case(method, kind, shape, dtype, k, seed, linearize=False):
    case = synthetic_case(method, kind, len(shape), shape, 1, seed, dtype=dtype, linearize=linearize, specials=False)
    rng = np.random.default_rng(1000 + seed)
    fields = np.stack([rng.uniform(-1.0, 1.0, case.vals.size).astype(dtype) for _ in range(k)])
    return case, fields


def _axis(g, m, rng, dtype):
    """`m` coordinates for the grid axis `g`: below and above the grid, in the first, the last and a middle interval (with
    the two ends: all five cubic saturation classes, the Low sign among them), exact knots, a repeated value, the rest
    random; shuffled."""
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


def _tensors(arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def _single(case, fields, axes, fma=None, options=None):
    """The reference: `Interpolator.eval_lattice_grad_tensors` of every field alone, (K, *m) values and (K, N, *m) Jacobian."""
    vals, jac = [], []
    ax_t = _tensors(axes)
    for f in range(fields.shape[0]):
        it = _make_one(case, fields[f], fma)
        try:
            for name, value in (options or {}).items():
                it.set_option(name, value)
            out, grad = it.eval_lattice_grad_tensors(ax_t)
            it.finish()
            vals.append(out.cpu().numpy())
            jac.append(grad.cpu().numpy())
        finally:
            it.close()
    return np.stack(vals), np.stack(jac)


def _field_major(out, jac, field_axis):
    """Results of either layout as (K, *m) and (K, N, *m)."""
    out = out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)
    jac = jac.cpu().numpy() if hasattr(jac, "cpu") else np.asarray(jac)
    if field_axis == 0:
        return out, jac
    return np.ascontiguousarray(np.moveaxis(out, -1, 0)), np.ascontiguousarray(np.moveaxis(np.moveaxis(jac, -1, 0), -1, 0))


def _check_shapes(fs, axes, out, jac, field_axis):
    m, k, nd = tuple(a.size for a in axes), fs.nfields, len(axes)
    assert tuple(out.shape) == ((k,) + m if field_axis == 0 else m + (k,))
    assert tuple(jac.shape) == ((k, nd) + m if field_axis == 0 else m + (k, nd))


def _eval(fs, axes, field_axis, **kw):
    out, jac = fs.eval_lattice_grad_tensors(_tensors(axes), field_axis=field_axis, **kw)
    fs.finish()
    _check_shapes(fs, axes, out, jac, field_axis)
    return _field_major(out, jac, field_axis)


def _eval_host(fs, axes, field_axis):
    out, jac = fs.eval_lattice_grad_host(axes, field_axis=field_axis)
    _check_shapes(fs, axes, out, jac, field_axis)
    return _field_major(out, jac, field_axis)


def _kernel(dtype, method, n, kind, fma, field_axis):
    return (f"{ROWS_KERNEL}{'double' if dtype == np.float64 else 'float'}, {0 if method == 'linear' else 1}, {n}, "
            f"{'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}, {'true' if field_axis else 'false'}>")


def _round16(v):
    return (v + 15) // 16 * 16


def _wave_bytes(method, n, n_last, elem, g, field_axis):
    lines = n + 1 if method == "linear" else n
    return _round16(g * lines * n_last * elem) + (_round16(64 * ((g * (n + 1)) | 1) * elem) if field_axis else 0)


def _group(method, n, n_last, elem, k, field_axis, budget=DEFAULT_BUDGET):
    """G by the formula of lattice.h."""
    g = 0
    while g < min(k, CAP) and WAVES * _wave_bytes(method, n, n_last, elem, g + 1, field_axis) <= budget:
        g += 1
    return g


# ---- 1. every fused instantiation -----------------------------------------------------------------------------------------
FUSED = [("linear", False), ("cubic", False), ("cubic", True)]


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("method,linearize", FUSED, ids=["linear", "cubic-nolin", "cubic-lin"])
def test_fused_instantiations(method, linearize, n, kind, dtype, fma):
    k = 3
    case, fields = _fields_case(method, kind, SHAPES[n], dtype, k, seed=3 * n + len(method), linearize=linearize)
    axes = _axes(case, LATTICE[n], seed=100 + n)
    want = _single(case, fields, axes, fma, {"lattice": 1})
    fs = _make(case, fields, fma)
    try:
        fs.set_option("lattice", 1)
        for field_axis in LAYOUTS:
            value = fs.eval_lattice_tensors(_tensors(axes), field_axis=field_axis)  # the value form of the set
            fs.finish()
            dev = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused"
            assert fs.kernel_name() == _kernel(dtype, method, n, kind, fma, field_axis), fs.kernel_name()
            g = _group(method, n, SHAPES[n][-1], fields.dtype.itemsize, k, field_axis)
            assert 1 <= g <= k and fs.get_option("last_lattice_group") == g
            host = _eval_host(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused"
            _assert_pair(dev, want, ("fused device", method, n, kind, field_axis))
            _assert_pair(host, want, ("fused host", method, n, kind, field_axis))
            value = value.cpu().numpy()
            _assert_bits(value if field_axis == 0 else np.ascontiguousarray(np.moveaxis(value, -1, 0)), want[0], "Fields.eval_lattice")
    finally:
        fs.close()


# ---- 2. field counts and groups -------------------------------------------------------------------------------------------
GROUP_CASES = [("linear", "regular", [9, 7, 32], [6, 5, 70], np.float64), ("cubic", "rectilinear", [37, 64], [23, 70], np.float32)]
GROUP_IDS = ["linear3-f64", "cubic2-f32"]


@pytest.fixture(scope="module")
def group_refs():
    """The references of the nine-field sets of GROUP_CASES, computed once: the first K fields serve every smaller K."""
    refs = {}
    for name, (method, kind, shape, lens, dtype) in zip(GROUP_IDS, GROUP_CASES):
        case, fields = _fields_case(method, kind, shape, dtype, CAP + 1, seed=17)
        axes = _axes(case, lens, seed=21)
        refs[name] = (case, fields, axes, _single(case, fields, axes, None, {"lattice": 1}))
    return refs


@pytest.mark.parametrize("k", list(range(1, CAP + 2)))
@pytest.mark.parametrize("name", GROUP_IDS)
def test_field_counts(group_refs, name, k):
    """K = 1 .. 9 with a 60 KiB budget, so that whole sets fit a pass; K = 9 exceeds the cap of 8: with G = 8 two passes, the
    last of one field."""
    case, fields, axes, want = group_refs[name]
    elem, n = fields.dtype.itemsize, len(case.dims)
    fs = _make(case, fields[:k])
    try:
        fs.set_option("lattice", 1)
        fs.set_option("axis_lds_kb", 60)
        for field_axis in LAYOUTS:
            got = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused"
            g = _group(case.method, n, case.dims[-1], elem, k, field_axis, 60 * 1024)
            assert 1 <= g <= min(k, CAP) and fs.get_option("last_lattice_group") == g, (g, fs.get_option("last_lattice_group"))
            if name == "cubic2-f32" or field_axis == 0:
                assert g == min(k, CAP)
            _assert_pair(got, (want[0][:k], want[1][:k]), ("K", name, k, field_axis))
    finally:
        fs.close()


@pytest.mark.parametrize("g", [1, 2, 3])
@pytest.mark.parametrize("name", GROUP_IDS)
def test_groups_smaller_than_the_set(group_refs, monkeypatch, name, g):
    """K = 8 with the LDS budget set so that G = 1, 2, 3 (chosen with the plan function): several passes per row, and for
    G = 3 a short last pass."""
    import interpn_amd

    case, fields, axes, want = group_refs[name]
    k = 8
    lens = [a.size for a in axes]
    monkeypatch.setenv("INTERPN_HIP_LATTICE", "1")

    def planned(kb, field_axis):
        monkeypatch.setenv("INTERPN_HIP_AXIS_LDS_KB", str(kb))
        return interpn_amd.fields_lattice_grad_plan(fields.dtype, case.method, case.dims, lens, k, field_axis)[1]

    fs = _make(case, fields[:k])
    try:
        fs.set_option("lattice", 1)
        for field_axis in LAYOUTS:
            kb = next(kb for kb in range(1, 61) if planned(kb, field_axis) == g)
            fs.set_option("axis_lds_kb", kb)
            got = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "fused" and fs.get_option("last_lattice_group") == g
            _assert_pair(got, (want[0][:k], want[1][:k]), ("G", name, g, field_axis))
    finally:
        fs.close()


# ---- 3. axis lengths, strides and guards ----------------------------------------------------------------------------------
LENGTH_CASES = [("linear", "regular", 3, np.float64), ("cubic", "rectilinear", 2, np.float32)]
LENGTH_IDS = ["linear3-regular-f64", "cubic2-rectilinear-f32"]


def _guarded(fs, axes, want, mk, dtype):
    """Both layouts with strides above their minima inside sentinel-filled buffers: `mk(shape)` makes one, torch or numpy."""
    k, nd = fs.nfields, len(axes)
    count = int(np.prod([a.size for a in axes]))
    on_device = not isinstance(mk((1,)), np.ndarray)
    call = (lambda o, j, fa: fs.eval_lattice_grad_tensors(_tensors(axes), o, j, field_axis=fa)) if on_device else (
        lambda o, j, fa: fs.eval_lattice_grad_host(axes, o, j, field_axis=fa))
    host = (lambda t: t.cpu().numpy()) if on_device else (lambda t: t)
    # field-major: out_stride = jac_stride = prod(m) + 5, one more row behind each block
    obuf, jbuf = mk((k + 1, count + 5)), mk((k * nd + 1, count + 3))
    call(obuf[:k, :count], jbuf[:k * nd].reshape(k, nd, count + 3)[:, :, :count], 0)
    fs.finish()
    o, j = host(obuf), host(jbuf)
    _assert_bits(o[:k, :count].reshape(want[0].shape), want[0], "field-major values")
    _assert_bits(j[:k * nd, :count].reshape(want[1].shape), want[1], "field-major jacobian")
    assert (o[:k, count:] == SENTINEL).all() and (o[k] == SENTINEL).all()
    assert (j[:k * nd, count:] == SENTINEL).all() and (j[k * nd] == SENTINEL).all()
    # fields-last: out_stride = K + 3, jac_stride = (K + 1) N, one more row behind the points
    obuf, jbuf = mk((count + 1, k + 3)), mk((count + 1, k + 1, nd))
    call(obuf[:count, :k], jbuf[:count, :k], -1)
    fs.finish()
    o, j = host(obuf), host(jbuf)
    got = _field_major(o[:count, :k], j[:count, :k], -1)
    _assert_bits(got[0].reshape(want[0].shape), want[0], "fields-last values")
    _assert_bits(got[1].reshape(want[1].shape), want[1], "fields-last jacobian")
    assert (o[:count, k:] == SENTINEL).all() and (o[count] == SENTINEL).all()
    assert (j[:count, k:] == SENTINEL).all() and (j[count] == SENTINEL).all()


def _guard_makers(dtype):
    import torch

    tdt = torch.float64 if dtype == np.float64 else torch.float32
    return (lambda shape: torch.full(shape, SENTINEL, dtype=tdt, device="cuda:0")), (lambda shape: np.full(shape, SENTINEL, dtype=dtype))


@pytest.mark.parametrize("other", [1, 2, 7])
@pytest.mark.parametrize("last", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("method,kind,n,dtype", LENGTH_CASES, ids=LENGTH_IDS)
def test_axis_lengths_strides_and_guards(method, kind, n, dtype, last, other):
    """Ragged chunks and the tile's unused lanes; out_stride and jac_stride above their minima; nothing written outside."""
    k = 3
    lens = [other] * (n - 1) + [last]
    case, fields = _fields_case(method, kind, SHAPES[n], dtype, k, seed=11)
    axes = _axes(case, lens, seed=last + other)
    want = _single(case, fields, axes, None, {"lattice": 1})
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 1)
        for mk in _guard_makers(dtype):
            _guarded(fs, axes, want, mk, dtype)
            assert fs.last_lattice_path == "fused"
    finally:
        fs.close()


@pytest.mark.parametrize("method,kind,n,dtype,n_last", [("linear", "regular", 3, np.float64, 2), ("linear", "rectilinear", 2, np.float32, 2),
                                                          ("cubic", "rectilinear", 3, np.float64, 4), ("cubic", "regular", 2, np.float32, 4),
                                                          ("linear", "regular", 3, np.float64, 65), ("cubic", "rectilinear", 2, np.float32, 65)])
def test_last_grid_axis_lengths(method, kind, n, dtype, n_last):
    """A last grid axis of 2 (multilinear: a `b` line of one entry), of 4 (the multicubic minimum) and of 65 (the column loop
    runs twice)."""
    k = 3
    shape = SHAPES[n][:-1] + [n_last]
    case, fields = _fields_case(method, kind, shape, dtype, k, seed=19)
    axes = _axes(case, LATTICE[n], seed=n_last)
    want = _single(case, fields, axes, None, {"lattice": 1})
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 1)
        for field_axis in LAYOUTS:
            _assert_pair(_eval(fs, axes, field_axis), want, ("n_last", method, n_last, field_axis))
            assert fs.last_lattice_path == "fused"
    finally:
        fs.close()


@pytest.mark.parametrize("method,kind", [("linear", "regular"), ("cubic", "rectilinear")])
def test_a_wave_takes_more_than_one_row(method, kind):
    """A 2-D lattice of 8200 rows: more than the 256 x 8 x 4 waves of the largest launch, so that a wave's row loop, its
    group loop inside and the wave_sync between them run a second time."""
    k = 3
    lens = [8200, 9]
    case, fields = _fields_case(method, kind, SHAPES[2], np.float64, k, seed=5)
    axes = _axes(case, lens, seed=2)
    want = _single(case, fields, axes, None, {"lattice": 1})
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 1)
        fs.set_option("axis_lds_kb", 7)  # fields-last: the lines and the tile of one field fit, of two do not: G = 1 < K
        for field_axis in LAYOUTS:
            _assert_pair(_eval(fs, axes, field_axis), want, ("rows", method, field_axis))
            assert fs.last_lattice_path == "fused"
    finally:
        fs.close()


def test_last_axis_at_the_lds_budget():
    """1 KiB, 3-D f64 multilinear: four waves x four lines x 8 columns x 8 bytes fill it, so a last grid axis of 8 is fused
    (field-major, G = 1) and one of 9 goes per field, with the same bits as K single handles either way."""
    k = 2
    for n_last, path in ((8, "fused"), (9, "per_field")):
        case, fields = _fields_case("linear", "regular", [7, 6, n_last], np.float64, k, seed=8)
        axes = _axes(case, [6, 5, 70], seed=13)
        want = _single(case, fields, axes)
        fs = _make(case, fields)
        try:
            fs.set_option("lattice", 1)
            fs.set_option("axis_lds_kb", 1)
            _assert_pair(_eval(fs, axes, 0), want, ("field-major", n_last))
            assert fs.last_lattice_path == path
            if path == "fused":
                assert fs.get_option("last_lattice_group") == 1
            _assert_pair(_eval(fs, axes, -1), want, ("fields-last", n_last))
            assert fs.last_lattice_path == "per_field"  # the tile of one field does not fit beside the lines
        finally:
            fs.close()


# ---- 4. per-field path ----------------------------------------------------------------------------------------------------
PER_FIELD = [  # method, shape, lattice, options, whether a fused result exists
    ("linear", [7, 6, 5], [11, 13, 71], {"lattice": 0}, True),
    ("cubic", [9, 8], [41, 67], {"lattice": 0}, True),
    ("linear", [31], [777], {"lattice": 1}, False),
    ("cubic", [5, 6, 4, 7], [4, 3, 5, 33], {"lattice": 1}, False),
    ("linear", [7, 6, 9], [6, 5, 70], {"lattice": 1, "axis_lds_kb": 1}, False),
    ("linear", [7, 6, 5], [11, 13, 71], {"lattice": 1, "force_generic": 1}, False),
    ("cubic", [9, 8], [41, 67], {"lattice": 1, "force_generic": 1}, False),
]


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("method,shape,lens,options,both", PER_FIELD,
                         ids=["lattice0-linear3", "lattice0-cubic2", "N1", "N4", "beyond-budget", "generic-linear3", "generic-cubic2"])
def test_per_field_path(method, shape, lens, options, both, kind):
    k = 3
    case, fields = _fields_case(method, kind, shape, np.float64, k, seed=len(shape) + 5)
    axes = _axes(case, lens, seed=13)
    want = _single(case, fields, axes, None, options)
    fs = _make(case, fields)
    try:
        for name, value in options.items():
            fs.set_option(name, value)
        fs.set_option("points_slice", max(256, 3 * int(np.prod(lens[1:]))))  # fields-last: several slices of leading indices
        for field_axis in LAYOUTS:
            got = _eval(fs, axes, field_axis)
            assert fs.last_lattice_path == "per_field" and fs.get_option("last_lattice_path") == 1
            _assert_pair(got, want, ("per field", method, shape, field_axis))
            _assert_pair(_eval_host(fs, axes, field_axis), want, ("per field host", method, shape, field_axis))
            if both:
                fs.set_option("lattice", 1)
                fused = _eval(fs, axes, field_axis)
                assert fs.last_lattice_path == "fused"
                _assert_pair(fused, got, ("fused vs per field", method, field_axis))
                fs.set_option("lattice", 0)
    finally:
        fs.close()


def test_guards_on_the_per_field_path():
    """The strided views of test_axis_lengths_strides_and_guards through the join kernels: several slices, nothing outside."""
    k = 3
    case, fields = _fields_case("cubic", "regular", SHAPES[3], np.float64, k, seed=11)
    axes = _axes(case, [7, 5, 65], seed=3)
    want = _single(case, fields, axes)
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 0)
        fs.set_option("points_slice", 2 * 5 * 65)
        for mk in _guard_makers(np.float64):
            _guarded(fs, axes, want, mk, np.float64)
            assert fs.last_lattice_path == "per_field"
    finally:
        fs.close()


def test_nearest_sets_are_unsupported_and_the_order_of_the_checks():
    import interpn_amd

    lib = interpn_amd._lib.load()
    dev, host = lib.interpn_hip_fields_eval_lattice_grad_device, lib.interpn_hip_fields_eval_lattice_grad_host
    lens = [5, 9]
    m = (ctypes.c_size_t * 2)(*lens)
    m0 = (ctypes.c_size_t * 2)(0, 9)
    case, fields = _fields_case("nearest", "regular", [9, 11], np.float64, 2, seed=3)
    axes = _axes(case, lens, seed=1)
    ax_t = _tensors(axes)
    vp = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ax_t])
    import torch

    out = torch.zeros(2 * 45, dtype=torch.float64, device="cuda:0")
    jac = torch.zeros(2 * 2 * 45, dtype=torch.float64, device="cuda:0")
    po, pj = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(jac.data_ptr())
    fs = _make(case, fields)
    try:
        assert dev(fs._h, vp, m, 2, po, 45, pj, 45, 0, None, 0, None) == 33          # INTERPN_HIP_ERR_UNSUPPORTED
        assert dev(fs._h, vp, m, 2, po, 1, None, 1, 7, None, 0, None) == 33          # ... before jac, layout and strides
        assert dev(fs._h, vp, m, 3, po, 45, pj, 45, 0, None, 0, None) == 1           # ... behind the lattice's own checks
        assert dev(fs._h, vp, m0, 2, None, 0, None, 0, 0, None, 0, None) == 0        # an empty axis comes first: nothing to do
        assert host(fs._h, vp, m, 2, po, 45, pj, 45, 0, None) == 33
        with pytest.raises(Exception, match="[Uu]nsupported"):
            fs.eval_lattice_grad_tensors(ax_t)
        assert lib.interpn_hip_fields_reserve_lattice_grad(fs._h, m, 2, 1) == 33
        assert (out == 0).all() and (jac == 0).all()
    finally:
        fs.close()
    case, fields = _fields_case("linear", "regular", [9, 11], np.float64, 2, seed=3)
    fs = _make(case, fields)
    try:
        assert dev(fs._h, vp, m, 2, po, 45, pj, 45, 0, None, 0, None) == 0
        assert fs.finish() is None
        assert dev(fs._h, vp, m, 2, po, 45, None, 45, 0, None, 0, None) == 32        # jac NULL
        assert dev(fs._h, vp, m, 2, po, 45, pj, 45, 3, None, 0, None) == 32          # no such layout
        assert dev(fs._h, vp, m, 2, po, 44, pj, 45, 0, None, 0, None) == 32          # out_stride below prod(m)
        assert dev(fs._h, vp, m, 2, po, 45, pj, 44, 0, None, 0, None) == 32          # jac_stride below prod(m)
        assert dev(fs._h, vp, m, 2, po, 1, pj, 4, 1, None, 0, None) == 32            # out_stride below K
        assert dev(fs._h, vp, m, 2, po, 2, pj, 3, 1, None, 0, None) == 32            # jac_stride below K N
        assert dev(fs._h, vp, m, 2, po, 2, pj, 4, 1, None, 0, None) == 0
        assert fs.finish() is None
        assert dev(fs._h, vp, m, 2, None, 45, pj, 45, 0, None, 0, None) == 32        # out NULL
        assert dev(fs._h, vp, m, 2, po, 45, pj, 45, 0, None, 2, None) == 32          # unknown flag
        assert dev(fs._h, vp, m, 3, po, 1, None, 1, 3, None, 0, None) == 1           # the lattice's checks come first
        assert dev(fs._h, None, m, 2, po, 1, None, 1, 3, None, 0, None) == 32
        assert dev(fs._h, vp, m0, 2, None, 0, None, 0, 3, None, 0, None) == 0        # an empty axis, whatever the rest says
        assert host(fs._h, vp, m, 3, po, 1, None, 1, 3, None) == 1
        assert host(fs._h, vp, m, 2, po, 45, None, 45, 0, None) == 32
        assert host(fs._h, vp, m, 2, po, 45, pj, 44, 0, None) == 32
    finally:
        fs.close()


# ---- 5. failing points on regular grids -----------------------------------------------------------------------------------
def _formula(lens, bad):
    """min over bad (d, j) of j * prod(lens[e], e > d)."""
    return min(j * int(np.prod(lens[d + 1:], dtype=object)) for d, j in bad)


BAD_SETS = [[(0, 5)], [(1, 3)], [(2, 7)], [(0, 6), (2, 2)]]
FAIL_LENS = [9, 8, 45]


@pytest.fixture(scope="module")
def failing_refs():
    refs = {}
    for method in ("linear", "cubic"):
        case, fields = _fields_case(method, "regular", SHAPES[3], np.float64, 3, seed=23)
        clean = _axes(case, FAIL_LENS, seed=9)
        refs[method] = (case, fields, clean, _single(case, fields, clean))
    return refs


@pytest.mark.parametrize("bad", BAD_SETS, ids=["axis0", "middle", "last", "two"])
@pytest.mark.parametrize("method,mode", [("linear", 1), ("cubic", 1), ("linear", 0)], ids=["linear-fused", "cubic-fused", "linear-per-field"])
def test_failing_points_on_regular_grids(failing_refs, method, mode, bad):
    lens = FAIL_LENS
    case, fields, clean, want = failing_refs[method]
    k, nd, count = fields.shape[0], 3, int(np.prod(lens))
    axes = [a.copy() for a in clean]
    for d, j in bad:
        axes[d][j] = np.nan
    first = _formula(lens, bad)
    if all(d == 0 for d, _ in bad):  # a failing leading coordinate: behind the host form's first chunk and the first slice
        assert first >= 2 * lens[1] * lens[2]
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", mode)
        fs.set_option("points_slice", 2 * lens[1] * lens[2])  # per-field, fields-last: five slices of leading indices
        fs.set_option("host_chunk", 2 * lens[1] * lens[2] + 7)  # host form: five chunks
        for field_axis in LAYOUTS:
            fs.eval_lattice_grad_tensors(_tensors(axes), field_axis=field_axis)
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
                fs.finish()
            assert e.value.first_bad_index == first, (e.value.first_bad_index, first, field_axis)
            assert fs.last_lattice_path == ("fused" if mode else "per_field")
            # host form: exactly the prefix of every field and component, the rest as it was
            out = np.full([k] + lens if field_axis == 0 else lens + [k], SENTINEL)
            jac = np.full([k, nd] + lens if field_axis == 0 else lens + [k, nd], SENTINEL)
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as e:
                fs.eval_lattice_grad_host(axes, out, jac, field_axis=field_axis)
            assert e.value.first_bad_index == first
            o, j = _field_major(out, jac, field_axis)
            o, j = o.reshape(k, count), j.reshape(k, nd, count)
            _assert_bits(o[:, :first], want[0].reshape(k, count)[:, :first], ("prefix", bad, field_axis))
            _assert_bits(j[:, :, :first], want[1].reshape(k, nd, count)[:, :, :first], ("jacobian prefix", bad, field_axis))
            assert (o[:, first:] == SENTINEL).all() and (j[:, :, first:] == SENTINEL).all()
            # the status words are cleared: a clean lattice afterwards is clean
            _assert_pair(_eval(fs, clean, field_axis), want, ("clean after failure", bad, field_axis))
    finally:
        fs.close()


@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "per_field"])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_rectilinear_grids_propagate_nan(method, mode):
    lens = [9, 8, 45]
    case, fields = _fields_case(method, "rectilinear", SHAPES[3], np.float64, 2, seed=29)
    axes = _axes(case, lens, seed=4)
    axes[0][2] = np.nan
    axes[2][31] = np.nan
    ref = _single(case, fields, axes, None, {"lattice": mode})
    assert np.isnan(ref[0][:, 2]).all() and np.isnan(ref[0][:, :, :, 31]).all()
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", mode)
        for field_axis in LAYOUTS:
            got = _eval(fs, axes, field_axis)  # finish() inside: no failure reported
            host = _eval_host(fs, axes, field_axis)
            for res in (got, host):
                for r, w in zip(res, ref):
                    assert np.array_equal(np.isnan(r), np.isnan(w))
                    _assert_bits(r[~np.isnan(w)], w[~np.isnan(w)], ("beside the NaN planes", field_axis))
    finally:
        fs.close()


# ---- 6. streams, reserve, capture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_axis", LAYOUTS, ids=["field-major", "fields-last"])
@pytest.mark.parametrize("mode", [1, 0], ids=["fused", "per_field"])
def test_streams_and_reserve(mode, field_axis):
    import torch

    import interpn_amd

    lens = [12, 9, 130]
    k = 3
    case, fields = _fields_case("linear", "rectilinear", SHAPES[3], np.float64, k, seed=31)
    axes = [_axes(case, lens, seed=6), _axes(case, lens, seed=7)]
    want = [_single(case, fields, a) for a in axes]
    oshape = [k] + lens if field_axis == 0 else lens + [k]
    jshape = [k, 3] + lens if field_axis == 0 else lens + [k, 3]
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", mode)
        # no_alloc without a reserved block: the out-of-memory status, not a silent allocation and not another failure
        with pytest.raises(interpn_amd._lib.InterpnHipError, match="[Oo]ut of memory|memory"):
            fs.eval_lattice_grad_tensors(_tensors(axes[0]), field_axis=field_axis, no_alloc=True)
        torch.cuda.synchronize()
        fs.reserve_lattice_grad(lens, 2)
        allocs = fs.get_option("scratch_allocs")
        assert allocs >= 1
        _assert_pair(_eval(fs, axes[0], field_axis, no_alloc=True), want[0], "no_alloc after reserve")
        # two side streams at once
        ax_t = [_tensors(a) for a in axes]
        outs = [torch.zeros(oshape, dtype=torch.float64, device="cuda:0") for _ in range(2)]
        jacs = [torch.zeros(jshape, dtype=torch.float64, device="cuda:0") for _ in range(2)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for rep in range(3):
            for i in range(2):
                fs.eval_lattice_grad_tensors(ax_t[i], outs[i], jacs[i], field_axis=field_axis, stream=streams[i], no_alloc=True)
        fs.finish()
        assert fs.get_option("scratch_allocs") == allocs
        for i in range(2):
            _assert_pair(_field_major(outs[i], jacs[i], field_axis), want[i], ("side stream", i))
    finally:
        fs.close()


@pytest.mark.parametrize("field_axis", LAYOUTS, ids=["field-major", "fields-last"])
def test_fused_evaluation_in_a_graph(field_axis):
    """One fused evaluation (two kernels on one stream: a single-branch graph), replayed twice on new axis contents."""
    import torch

    lens = [12, 9, 130]
    k = 3
    case, fields = _fields_case("cubic", "regular", SHAPES[3], np.float64, k, seed=37)
    axes = _axes(case, lens, seed=6)
    fs = _make(case, fields)
    try:
        fs.set_option("lattice", 1)
        fs.reserve_lattice_grad(lens, 1)
        ax_t = _tensors(axes)
        out = torch.zeros([k] + lens if field_axis == 0 else lens + [k], dtype=torch.float64, device="cuda:0")
        jac = torch.zeros([k, 3] + lens if field_axis == 0 else lens + [k, 3], dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fs.eval_lattice_grad_tensors(ax_t, out, jac, field_axis=field_axis)
        assert fs.last_lattice_path == "fused"
        for rep in range(2):
            fresh = _axes(case, lens, seed=50 + rep)
            for d in range(3):
                ax_t[d].copy_(torch.from_numpy(fresh[d]))
            out.zero_()
            jac.zero_()
            graph.replay()
            torch.cuda.synchronize()
            _assert_pair(_field_major(out, jac, field_axis), _single(case, fields, fresh), ("replay", rep))
        fs.finish()
    finally:
        fs.close()


# ---- 7. one-call form, dispatch, autograd ---------------------------------------------------------------------------------
def _exact_grids(kind, shape, rng):
    grids = []
    for n in shape:
        g = -1.0 + 0.125 * np.arange(n)  # exactly equal spacings: the one-call forms take the grid for regular
        if kind == "rectilinear":
            g[1:-1] += rng.uniform(-0.03, 0.03, n - 2)
        grids.append(g)
    return grids


@pytest.mark.parametrize("method", ["linear", "cubic"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_interpn_fields_lattice_grad_entry_point(kind, method):
    import torch

    import interpn_amd

    rng = np.random.default_rng(41)
    shape, lens, k = [9, 12, 17], [6, 5, 70], 3
    grids = _exact_grids(kind, shape, rng)
    vals = rng.uniform(-1, 1, [k] + shape)
    axes = [np.sort(rng.uniform(g[0], g[-1], m)) for g, m in zip(grids, lens)]
    axes[1][2] = grids[1][-1] + 0.5
    single = [interpn_amd.interpn_lattice_grad(axes, grids, vals[f], method=method) for f in range(k)]
    want = np.stack([s[0] for s in single]), np.stack([s[1] for s in single])
    got = interpn_amd.interpn_fields_lattice_grad(axes, grids, vals, method=method)
    _assert_pair(got, want, ("fields first", kind, method))
    vals_last = np.ascontiguousarray(np.moveaxis(vals, 0, -1))
    got = interpn_amd.interpn_fields_lattice_grad(axes, grids, vals_last, method=method, field_axis=-1)
    assert got[0].shape == tuple(lens) + (k,) and got[1].shape == tuple(lens) + (k, 3)
    _assert_pair(_field_major(got[0], got[1], -1), want, ("fields last", kind, method))
    for field_axis, v in ((0, vals), (-1, vals_last)):
        got_t = interpn_amd.interpn_fields_lattice_grad(_tensors(axes), grids, torch.from_numpy(v).to("cuda:0"), method=method,
                                                        field_axis=field_axis)
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in got_t)
        _assert_pair(_field_major(got_t[0], got_t[1], field_axis), want, ("torch input", field_axis))
    with pytest.raises(Exception, match="[Uu]nsupported"):
        interpn_amd.interpn_fields_lattice_grad(axes, grids, vals, method="nearest")


def test_eval_lattice_grad_dispatch():
    k, lens = 2, [5, 9]
    case, fields = _fields_case("linear", "regular", [9, 11], np.float64, k, seed=3)
    axes = _axes(case, lens, seed=1)
    want = _single(case, fields, axes)
    fs = _make(case, fields)
    try:
        _assert_pair(fs.eval_lattice_grad(axes), want, "numpy")
        out, jac = np.zeros(lens + [k]), np.zeros(lens + [k, 2])
        back = fs.eval_lattice_grad(axes, out, jac, field_axis=-1)
        assert back[0] is out and back[1] is jac
        _assert_pair(_field_major(out, jac, -1), want, "numpy out=")
        res = fs.eval_lattice_grad(_tensors(axes), field_axis=-1)
        fs.finish()
        _assert_pair(_field_major(res[0], res[1], -1), want, "torch")
    finally:
        fs.close()


@pytest.mark.parametrize("field_axis", LAYOUTS, ids=["field-major", "fields-last"])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_autograd_interp_fields_lattice(method, field_axis):
    """Tables of small integers on a unit-step grid, axes at dyadic fractions inside it, integer weights: every product and
    sum of the forward and the backward pass is exact, so the sums over the fields and the other lattice dimensions cannot
    depend on their order."""
    import torch

    import interpn_amd
    from interpn_amd import autograd

    rng = np.random.default_rng(3)
    shape, k = [6, 7, 9], 3
    vals = rng.integers(-4, 5, [k] + shape).astype(np.float64)
    fs = interpn_amd.Fields.regular(method, shape, np.zeros(3), np.ones(3), vals, dtype=np.float64)
    try:
        fs.set_option("lattice", 1)
        lens = [5, 4, 70]
        axes = [torch.from_numpy(rng.integers(8, 8 * (n - 2), m) / 8.0).to("cuda:0").requires_grad_(True) for n, m in zip(shape, lens)]
        mesh = [a.detach().clone().requires_grad_(True) for a in axes]
        weights = torch.from_numpy(rng.integers(-3, 4, [k] + lens).astype(np.float64)).to("cuda:0")
        res = autograd.interp_fields_lattice(fs, axes, field_axis=field_axis)
        assert fs.last_lattice_path == "fused"
        assert tuple(res.shape) == ((k,) + tuple(lens) if field_axis == 0 else tuple(lens) + (k,))
        (res * (weights if field_axis == 0 else weights.permute(1, 2, 3, 0))).sum().backward()
        ref = autograd.interp_fields(fs, torch.meshgrid(*mesh, indexing="ij"))
        (ref * weights).sum().backward()
        assert torch.equal(res.detach() if field_axis == 0 else res.detach().permute(3, 0, 1, 2), ref.detach())
        for d in range(3):
            assert axes[d].grad is not None and axes[d].grad.shape == axes[d].shape
            assert torch.equal(axes[d].grad, mesh[d].grad), (d, axes[d].grad, mesh[d].grad)
        assert any(bool((a.grad != 0).any()) for a in axes)
    finally:
        fs.close()
