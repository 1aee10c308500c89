"""Every kernel family on the anisotropic workload (tests/helpers.py::anisotropic_case: every axis with its own origin, step
and spacing; rectilinear axes growing, shrinking or clustered), forced onto its path the way its own test forces it, and
compared BIT FOR BIT (a NaN need only be a NaN on both sides) with the oracle itself — the gradient families with
tests/grad_restatement.py / tests/cubic_grad_restatement.py — never with another evaluation of the same handle.  Every test
asserts the kernel or path it ran.  On `synthetic_case` (every axis linspace(-1, 1, n)) a start, first node or scale taken
from the wrong axis gives identical bits; here it moves nearly every point (tests/test_anisotropic_cpu.py).

Both element types under fma, and the other flavour once per family (f64).  The shapes are the smallest at which a path
still has all its structure: those of tests/test_anisotropic_cpu.py wherever the path can be forced on them, one with a
70-point axis, and the shapes of the forced sweep and bucket-record tests (the sweep kernels need their tables, the records
axes longer than a wave) on anisotropic axes."""

import dataclasses

import numpy as np
import pytest

from tests import cubic_grad_restatement as cg
from tests import grad_restatement as gr
from tests.helpers import anisotropic_axis, anisotropic_case, anisotropic_points, run_oracle

pytestmark = pytest.mark.gpu

S2, S3, S4 = [9, 7], [6, 5, 7], [5, 6, 4, 5]  # the shapes of tests/test_anisotropic_cpu.py
S5, S6 = [4, 3, 5, 3, 4], [3, 4, 2, 5, 3, 4]
LONG3, LONG2 = [70, 9, 7], [9, 130]           # one axis longer than a wave (rectilinear: searched in LDS, not across lanes)
NPTS = 2001
VARIANTS = [(np.float64, True), (np.float32, True), (np.float64, False)]
VIDS = ["f64-fma", "f32-fma", "f64-nofma"]
KINDS = ["regular", "rectilinear"]
KNOBS = ("BRICKS", "FORCE_GENERIC", "GENERIC_RUNTIME", "GENERIC_VEC", "AXIS_REGS", "PPL", "POINTS_PATH", "POINTS_LOAD", "POINTS_STORE",
         "POINTS_SLICE", "SWEEP", "SWEEP_PERIOD", "BINNED", "COLUMN", "LATTICE", "FIELDS_FUSED", "HOST_CHUNK", "DEAL")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv("INTERPN_HIP_" + name, raising=False)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist(), got[~same][:4], want[~same][:4])


def _case(method, kind, shape, dtype, nobs=NPTS, linearize=False, seed=0):
    """kind "jittered": rectilinear axes that keep the table's origins and steps but are near-uniform — the regular
    anisotropic axis with its interior nodes moved by up to a quarter step, `synthetic_case`'s jitter.  Per-bucket search
    records exist only where no two nodes share one of an axis's 2n uniform buckets (all axes or none): the growing,
    shrinking and clustered axes never qualify, these always do (intervals of at least half a step)."""
    seed = 6100 + 7 * len(shape) + seed
    if kind != "jittered":
        return anisotropic_case(method, kind, shape, nobs, seed, dtype, linearize=linearize)
    case = anisotropic_case(method, "regular", shape, nobs, seed, dtype, linearize=linearize)
    rng = np.random.default_rng(seed + 1)
    dt = case.vals.dtype.type
    for d, g in enumerate(case.grids):
        g64 = g.astype(np.float64)
        j = (rng.random(g.size) - 0.5) * 0.5 * (g64[1] - g64[0])
        j[0] = j[-1] = 0.0
        case.grids[d] = (g64 + j).astype(dt)
        assert np.all(np.diff(case.grids[d]) > 0)
        case.obs[d] = anisotropic_points(case.grids[d], nobs, rng, dt)
    case.kind = "rectilinear"
    return case


def _handle(case, fma, monkeypatch=None, bricks=None):
    """A resident handle, INTERPN_HIP_BRICKS = `bricks` while it is created (the table layouts are chosen then)."""
    import interpn_amd

    if bricks:
        monkeypatch.setenv("INTERPN_HIP_BRICKS", bricks)
    dt = case.vals.dtype
    if case.kind == "regular":
        it = interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, case.vals,
                                              linearize_extrapolation=case.linearize, dtype=dt, fma=fma)
    else:
        it = interpn_amd.Interpolator.rectilinear(case.method, case.grids, case.vals, linearize_extrapolation=case.linearize,
                                                  dtype=dt, fma=fma)
    if bricks:
        monkeypatch.delenv("INTERPN_HIP_BRICKS", raising=False)
    return it


def _fields_handle(case, fields, fma):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Fields.regular(case.method, case.dims, case.starts, case.steps, fields,
                                          linearize_extrapolation=case.linearize, dtype=fields.dtype, fma=fma)
    return interpn_amd.Fields.rectilinear(case.method, case.grids, fields, linearize_extrapolation=case.linearize,
                                          dtype=fields.dtype, fma=fma)


def _fields(case, k, seed):
    rng = np.random.default_rng(1000 + seed)
    return np.stack([rng.uniform(-1.0, 1.0, case.vals.size).astype(case.vals.dtype) for _ in range(k)])


def _fields_want(oracle, case, fields, fma, obs=None):
    """(K, n): the oracle on every field alone."""
    obs = case.obs if obs is None else obs
    return np.stack([run_oracle(oracle, dataclasses.replace(case, vals=f, obs=obs), fma=fma, out=np.zeros(obs[0].size, dtype=f.dtype))
                     for f in fields])


def _tensors(arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def _rows(obs):
    return np.ascontiguousarray(np.stack(obs, axis=1))


def _eval(it, obs):
    out = it.eval_tensors(_tensors(obs))
    it.finish()
    return out.cpu().numpy()


def _linear_bricks(n):
    return "on" if n == 2 else "11"  # the layouts the multilinear handles build regardless of the grid's size


def _grad_want(case, fma):
    out, grad, ok = (gr if case.method == "linear" else cg).eval_grad_case(case, fma=fma)
    assert ok.all()
    return out, np.ascontiguousarray(grad)


def _lattice_axes(case, lens, seed):
    """One coordinate vector per axis, by the generator's point rule."""
    rng = np.random.default_rng(seed)
    return [anisotropic_points(g, m, rng, case.vals.dtype.type) for g, m in zip(case.grids, lens)]


def _expand(axes):
    return [np.ascontiguousarray(m.ravel()) for m in np.meshgrid(*axes, indexing="ij")]


# ---- 1. multilinear N = 2..6: the C-order kernels and the brick kernels (test_linear_brick_layouts, test_linear2_brick) -------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("shape,layout", [(s, l) for s in (S2, S3, S4, S5, S6, LONG3) for l in ("off", "bricks", "c4") if l != "c4" or len(s) >= 4],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))  # (the 4-D cell bricks exist for N >= 4)
@pytest.mark.parametrize("kind", KINDS)
def test_multilinear_c_order_and_bricks(oracle, monkeypatch, kind, shape, layout, dtype, fma):
    n = len(shape)
    case = _case("linear", kind, shape, dtype)
    want = run_oracle(oracle, case, fma)
    it = _handle(case, fma, monkeypatch, {"off": "off", "bricks": _linear_bricks(n), "c4": "c4"}[layout])
    try:
        assert (it.table_layout()[0] > 0) == (layout != "off")
        got = _eval(it, case.obs)
        name = it.kernel_name()
        assert it.last_path == "in_place"
        if layout == "off":
            assert name.startswith(f"interpn::k_linear_{kind}<"), name
        else:
            assert name.startswith("interpn::k_linear2_brick<" if n == 2 else "interpn::k_linear_brick<"), name
        _assert_same(got, want, name)
        _assert_same(it.eval_host(case.obs, np.zeros(NPTS, dtype=dtype)), want, "host")
    finally:
        it.close()


# ---- 2. multicubic N = 2..4: the C-order kernels and the tiled kernel (test_cubic_tile_layouts) -----------------------------------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("linearize", [False, True], ids=["quad", "lin"])
@pytest.mark.parametrize("layout", ["off", "44", "24", "11"])
@pytest.mark.parametrize("shape", [S2, S3, S4, LONG3], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_multicubic_c_order_and_tiles(oracle, monkeypatch, kind, shape, layout, linearize, dtype, fma):
    case = _case("cubic", kind, shape, dtype, linearize=linearize)
    want = run_oracle(oracle, case, fma)
    it = _handle(case, fma, monkeypatch, layout)
    try:
        got = _eval(it, case.obs)
        name = it.kernel_name()
        assert it.last_path == "in_place"
        if layout == "off":
            assert it.table_layout()[0] == 0 and name.startswith(f"interpn::k_cubic_{kind}<"), name
        else:
            assert it.table_layout()[1:] == (int(layout[0]), int(layout[1])) and name.startswith("interpn::k_cubic_brick<"), name
        _assert_same(got, want, name)
    finally:
        it.close()


# ---- 3. sorted and column multicubic (test_binned_multicubic_evaluation, test_column_evaluation_of_sorted_{4d,3d}_multicubic) ------
SORTED = [("sorted", S2, "11", "interpn::k_cubic_brick<"), ("sorted", S3, "44", "interpn::k_cubic_brick<"),
          ("sorted", S4, "11", "interpn::k_cubic_brick<"), ("column", S4, "11", "interpn::k_cubic_column<"),
          ("column", S3, "11", "interpn::k_cubic3_column<")]


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("form,shape,layout,kernel", SORTED, ids=[f"{f}-N{len(s)}" for f, s, _, _ in SORTED])
@pytest.mark.parametrize("kind", KINDS)
def test_sorted_and_column_multicubic(oracle, monkeypatch, kind, form, shape, layout, kernel, dtype, fma):
    nobs = 5000  # more than one chunk of the sort (4096)
    case = _case("cubic", kind, shape, dtype, nobs=nobs, linearize=(len(shape) == 3))
    want = run_oracle(oracle, case, fma)
    it = _handle(case, fma, monkeypatch, layout)
    try:
        it.set_option("binned", 1)
        it.set_option("column", 1 if form == "column" else 0)
        for deal in (1, 0):
            it.set_option("deal", deal)
            got = _eval(it, case.obs)
            assert it.last_path == "binned" and it.get_option("last_binned") == 1
            assert it.kernel_name().startswith(kernel), it.kernel_name()
            _assert_same(got, want, (form, deal))
    finally:
        it.close()


# ---- 4. the sweep family (test_sweep_evaluation, test_linear2_sweep_evaluation, test_nearest_sweep_evaluation,
#         test_cubic_sweep_evaluation, test_cubic2_sweep_evaluation): their grids, 3001 points = several ragged rounds -----------------
SWEEPS = [("linear", "regular", [20, 17, 33], {}, "interpn::k_linear_sweep<{t}, false"),
          ("linear", "rectilinear", [24, 11, 40], {}, "interpn::k_linear_sweep<{t}, true"),
          ("linear", "rectilinear", [24, 11, 40], {"axis_regs": 1}, "interpn::k_linear_sweep<{t}, true"),
          ("linear", "rectilinear", [70, 33, 90], {}, "interpn::k_linear_sweep<{t}, true"),
          ("linear", "jittered", [70, 33, 90], {}, "interpn::k_linear_sweep<{t}, true"),  # the only rows with bucket records
          ("linear", "jittered", [70, 33, 90], {"axis_records": 0}, "interpn::k_linear_sweep<{t}, true"),
          ("linear", "rectilinear", [33, 30, 31], {"axis_regs": 0}, "interpn::k_linear_sweep<{t}, true"),
          ("linear", "regular", [70, 90], {}, "interpn::k_linear2_sweep<{t}, "),
          ("nearest", "regular", [70, 90], {}, "interpn::k_nearest_sweep<{t}, 2, "),
          ("nearest", "regular", [20, 17, 33], {}, "interpn::k_nearest_sweep<{t}, 3, "),
          ("cubic", "regular", [20, 17, 33], {}, "interpn::k_cubic_sweep<{t}, false"),
          ("cubic", "rectilinear", [24, 11, 40], {}, "interpn::k_cubic_sweep<{t}, true"),
          ("cubic", "rectilinear", [8, 70, 90], {}, "interpn::k_cubic_sweep<{t}, true"),
          ("cubic", "regular", [150, 140], {}, "interpn::k_cubic_sweep<{t}, false"),
          ("cubic", "rectilinear", [130, 160], {}, "interpn::k_cubic_sweep<{t}, true")]


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,kind,shape,options,kernel", SWEEPS,
                         ids=[f"{m}{len(s)}-{k}-{'x'.join(map(str, s))}" + "".join(f"-{a}{b}" for a, b in o.items()) for m, k, s, o, _ in SWEEPS])
def test_sweep_family(oracle, monkeypatch, method, kind, shape, options, kernel, dtype, fma):
    nobs = 3001
    for linearize in ((False, True) if method == "cubic" else (False,)):
        case = _case(method, kind, shape, dtype, nobs=nobs, linearize=linearize)
        want = run_oracle(oracle, case, fma)
        it = _handle(case, fma, monkeypatch)
        try:
            if kind != "regular" and method == "linear":
                assert (it.get_option("axis_rec_mode") in (1, 2)) == (kind == "jittered"), it.get_option("axis_rec_mode")
            for k, v in options.items():
                it.set_option(k, v)
            if method == "linear" and len(shape) == 3:
                assert it.get_option("sweep_table_bytes") > 0 and it.get_option("sweep_layout") in (11, 12)
            elif method != "nearest":
                assert it.table_layout()[0] > 0
            it.set_option("sweep", 1)
            for period in (0, 1):
                it.set_option("sweep_period", period)
                got = _eval(it, case.obs)
                assert it.last_path == "sweep", (it.last_path, it.last_path_reason)
                name = it.kernel_name()
                assert name.startswith(kernel.format(t="double" if dtype == np.float64 else "float")), name
                if method == "cubic":
                    assert name.endswith(", 2>") == (len(shape) == 2), name  # the 2-D form carries its N last
                _assert_same(got, want, (name, period, linearize))
            assert it.get_option("evals_sweep") == 2
        finally:
            it.close()


# ---- 5. rectilinear search forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("axis_regs", ["0", "1", "2"])
@pytest.mark.parametrize("method,shape", [("linear", S2), ("linear", [64, 7]), ("linear", S3), ("linear", S4), ("linear", S6),
                                          ("linear", LONG3), ("nearest", [64]), ("nearest", S2), ("nearest", S3), ("nearest", S6),
                                          ("nearest", LONG2)], ids=str)
def test_lane_resident_axis_search(oracle, monkeypatch, method, shape, axis_regs, dtype, fma):
    """INTERPN_HIP_AXIS_REGS = 0 (LDS), 1 (probe sequence across lanes), 2 (lane tables), as
    test_lane_resident_axes_everywhere sets it: the brick kernels and the nearest kernel; a 70-point axis keeps the LDS search."""
    monkeypatch.setenv("INTERPN_HIP_AXIS_REGS", axis_regs)
    n = len(shape)
    case = _case(method, "rectilinear", shape, dtype)
    want = run_oracle(oracle, case, fma)
    it = _handle(case, fma, monkeypatch, _linear_bricks(n) if method == "linear" else None)
    try:
        got = _eval(it, case.obs)
        name = it.kernel_name()
        in_lanes = max(shape) <= 64 and axis_regs != "0"
        modes = {"0": (0,), "1": (1,), "2": (2, 3)}[axis_regs] if in_lanes else (0,)
        args = [x.strip() for x in name[name.index("<") + 1:-1].split(",")]
        if method == "nearest":
            assert name.startswith("interpn::k_nearest<") and int(args[-2]) in modes, name       # ..., AXR, PPL>
        elif n == 2:
            assert name.startswith("interpn::k_linear2_brick<") and int(args[-2]) in modes, name  # ..., AXR, PPL>
        else:
            assert name.startswith("interpn::k_linear_brick<") and int(args[-3]) in modes, name   # ..., AXR, ABL, CELL>
        _assert_same(got, want, name)
    finally:
        it.close()


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape", [("linear", [65, 130]), ("linear", [70, 9, 81]), ("linear", [7, 90, 5, 6]),
                                          ("linear", [128, 120, 100]), ("nearest", [80, 70, 90])], ids=str)
@pytest.mark.parametrize("spacing", ["jittered", "rectilinear"])
def test_bucket_records_and_lds_search(oracle, monkeypatch, spacing, method, shape, dtype, fma):
    """Axes longer than a wave (test_rectilinear_bucket_records).  "jittered": near-uniform axes with the table's origins and
    steps, on which the per-bucket records are built (axis_rec_mode 1 = full, 2 = compact) — searched through them, without
    them (option axis_records = 0: coordinates + tables) and with the LDS search forced (axis_regs = 0).  "rectilinear": the
    generator's growing / shrinking / clustered axes hold several nodes in one bucket, so no records exist (mode 0, as on the
    clustered axis of the existing test) and the same three settings search coordinates + tables; nearest never has any."""
    n = len(shape)
    case = _case(method, spacing, shape, dtype)
    want = run_oracle(oracle, case, fma)
    obs = _tensors(case.obs)
    for records, axis_regs in ((1, -1), (0, -1), (1, 0)):
        it = _handle(case, fma, monkeypatch)
        try:
            mode = it.get_option("axis_rec_mode")
            if method == "linear" and spacing == "jittered":
                assert mode in (1, 2) and it.get_option("axis_rec_bytes") > 0, mode
            else:
                assert mode == 0, mode
            it.set_option("axis_records", records)
            it.set_option("axis_regs", axis_regs)
            got = it.eval_tensors(obs).cpu().numpy()
            it.finish()
            name = it.kernel_name()
            kernel = "interpn::k_nearest<" if method == "nearest" else "interpn::k_linear2_brick<" if n == 2 else "interpn::k_linear_brick<"
            assert it.last_path == "in_place" and name.startswith(kernel), name
            _assert_same(got, want, (name, mode, records, axis_regs))
        finally:
            it.close()


@pytest.mark.parametrize("dtype,fma", VARIANTS + [(np.float32, False)], ids=VIDS + ["f32-nofma"])
@pytest.mark.parametrize("d,n", [(0, 300), (1, 300), (2, 300), (0, 9), (2, 3), (1, 2)])
def test_linear_1d_records(oracle, monkeypatch, d, n, dtype, fma):
    """1-D multilinear from one record per search bucket (test_linear_1d_rectilinear_records: INTERPN_HIP_BRICKS=on), on each
    of the three spacings: growing, shrinking, clustered (twenty intervals at 1e-3 of the others)."""
    import interpn_amd

    rng = np.random.default_rng(40 + d)
    g = anisotropic_axis(d, n, "rectilinear", dtype, rng)
    vals = rng.uniform(-1, 1, n).astype(dtype)
    x = anisotropic_points(g, NPTS, rng, dtype)
    want = np.zeros(NPTS, dtype=dtype)
    oracle.linear_rectilinear([g], vals, [x], want, fma=fma)
    monkeypatch.setenv("INTERPN_HIP_BRICKS", "on")
    it = interpn_amd.Interpolator.rectilinear("linear", [g], vals, dtype=dtype, fma=fma)
    try:
        got = it.eval_host([x], np.zeros(NPTS, dtype=dtype))
        name = it.kernel_name()
        assert name.startswith("interpn::k_linear1_records<"), name
        _assert_same(got, want, name)
        _assert_same(_eval(it, [x]), want, "device")
    finally:
        it.close()


# ---- 6. the recursive arm: N = 7 multilinear, N = 5 multicubic, both forms of k_generic_n (test_recursive_arm_forms) and the
#         runtime-N kernel (test_recursive_arms) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("form", ["onetree", "rowvec", "runtime"])
@pytest.mark.parametrize("method,shape", [("linear", [3, 2, 3, 2, 3, 2, 3]), ("cubic", [4, 5, 4, 5, 4])], ids=["linear7", "cubic5"])
@pytest.mark.parametrize("kind", KINDS)
def test_recursive_arm(oracle, monkeypatch, kind, method, shape, form, dtype, fma):
    if form == "runtime":
        monkeypatch.setenv("INTERPN_HIP_GENERIC_RUNTIME", "1")
    else:
        monkeypatch.setenv("INTERPN_HIP_GENERIC_VEC", "1" if form == "rowvec" else "0")
    for linearize in ((False, True) if method == "cubic" else (False,)):
        case = _case(method, kind, shape, dtype, linearize=linearize)
        want = run_oracle(oracle, case, fma)
        it = _handle(case, fma, monkeypatch)
        try:
            got = _eval(it, case.obs)
            name = it.kernel_name()
            assert it.last_path == "in_place"
            if form == "runtime":
                assert name.startswith("interpn::k_generic<"), name
            else:
                assert name.startswith("interpn::k_generic_n<") and name.endswith(", true>") == (form == "rowvec"), name
            _assert_same(got, want, (name, linearize))
        finally:
            it.close()


# ---- 7. value and gradient: eval_grad / eval_cubic_grad, the fused kernels (N = 2, 3) and the runtime-N ones --------------------------
GRADS = [("linear", S2, "on"), ("linear", S3, "11"), ("linear", LONG3, "12"), ("linear", S4, None), ("linear", S6, None),
         ("cubic", S2, "22"), ("cubic", S3, "44"), ("cubic", LONG3, "11"), ("cubic", S4, None)]


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape,bricks", GRADS, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s, _ in GRADS])
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_fused_and_runtime_n(monkeypatch, kind, method, shape, bricks, dtype, fma):
    n = len(shape)
    fused, generic = (f"interpn::k_{method}_grad<", f"interpn::k_{method}_grad_n<")
    for linearize in ((False, True) if method == "cubic" else (False,)):
        case = _case(method, kind, shape, dtype, linearize=linearize)
        want_out, want_grad = _grad_want(case, fma)
        it = _handle(case, fma, monkeypatch, bricks)
        try:
            call = it.eval_cubic_grad_tensors if method == "cubic" else it.eval_grad_tensors
            for force in ((0, 1) if n <= 3 else (0,)):
                it.set_option("force_generic", force)
                out, grad = call(_tensors(case.obs))
                it.finish()
                name = it.kernel_name()
                assert name.startswith(fused if n <= 3 and not force else generic), name
                _assert_same(out.cpu().numpy(), want_out, (name, linearize, "out"))
                _assert_same(grad.cpu().numpy(), want_grad, (name, linearize, "grad"))
            it.set_option("force_generic", 0)
            hout, hgrad = (it.eval_cubic_grad_host if method == "cubic" else it.eval_grad_host)(case.obs)
            _assert_same(hout, want_out, "host out")
            _assert_same(hgrad, want_grad, "host grad")
        finally:
            it.close()


# ---- 8. point-major points: eval_points and eval_points_grad, fused and split ----------------------------------------------------------
POINTS = [("linear", S2, "on"), ("linear", S3, "11"), ("linear", LONG3, "11"), ("linear", S4, None), ("cubic", S2, "11"),
          ("cubic", S3, "44"), ("cubic", S4, None), ("nearest", S3, None)]


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape,bricks", POINTS, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s, _ in POINTS])
@pytest.mark.parametrize("kind", KINDS)
def test_point_major_values(oracle, monkeypatch, kind, method, shape, bricks, dtype, fma):
    import torch

    n = len(shape)
    case = _case(method, kind, shape, dtype, linearize=(method == "cubic"))
    want = run_oracle(oracle, case, fma)
    pts = _rows(case.obs)
    has_fused = method == "linear" and n in (2, 3)
    it = _handle(case, fma, monkeypatch, bricks)
    try:
        for path in ((1, 2) if has_fused else (0,)):
            it.set_option("points_path", path)
            if path == 2:
                it.set_option("points_slice", 512)  # four slices, the last one ragged
            got = it.eval_points_tensors(torch.from_numpy(pts).to("cuda:0"))
            it.finish()
            name = it.kernel_name()
            assert it.last_points_path() == ("fused" if path == 1 else "split"), (path, it.last_points_path())
            assert name.startswith("interpn::k_linear_points<") == (path == 1), name
            _assert_same(got.cpu().numpy(), want, (name, path))
            _assert_same(it.eval_points_host(pts), want, ("host", path))
    finally:
        it.close()


POINTS_GRAD = [("linear", S2, "on"), ("linear", S3, "11"), ("linear", LONG3, "22"), ("linear", S4, None), ("cubic", S2, "11"),
               ("cubic", S3, "24"), ("cubic", LONG3, "44"), ("cubic", S4, None)]


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape,bricks", POINTS_GRAD, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s, _ in POINTS_GRAD])
@pytest.mark.parametrize("kind", KINDS)
def test_point_major_gradients(monkeypatch, kind, method, shape, bricks, dtype, fma):
    import torch

    n = len(shape)
    fused = f"interpn::k_{method}_points_grad<"
    for linearize in ((False, True) if method == "cubic" and n <= 3 else (False,)):
        case = _case(method, kind, shape, dtype, linearize=linearize)
        want_out, want_grad = _grad_want(case, fma)
        want_grad = np.ascontiguousarray(want_grad.T)  # (n, N)
        pts = _rows(case.obs)
        it = _handle(case, fma, monkeypatch, bricks)
        try:
            for path in ((1, 2) if n <= 3 else (0,)):
                it.set_option("points_path", path)
                if path == 2:
                    it.set_option("points_slice", 512)
                out, grad = it.eval_points_grad_tensors(torch.from_numpy(pts).to("cuda:0"))
                it.finish()
                name = it.kernel_name()
                assert it.last_points_path() == ("fused" if path == 1 else "split"), (path, it.last_points_path())
                assert name.startswith(fused) == (path == 1) and ("points_grad" in name) == (path == 1), name
                _assert_same(out.cpu().numpy(), want_out, (name, path, "out"))
                _assert_same(grad.cpu().numpy(), want_grad, (name, path, "grad"))
                hout, hgrad = it.eval_points_grad_host(pts)
                _assert_same(hout, want_out, ("host out", path))
                _assert_same(hgrad, want_grad, ("host grad", path))
        finally:
            it.close()


# ---- 9. field sets: Fields.eval and Fields.eval_points, fused and per-field / split ----------------------------------------------------
FIELD_SHAPES = [("linear", S2), ("linear", S3), ("linear", LONG3), ("linear", LONG2), ("cubic", S3), ("nearest", S2), ("linear", S4)]


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape", FIELD_SHAPES, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s in FIELD_SHAPES])
@pytest.mark.parametrize("kind", KINDS)
def test_field_sets(oracle, kind, method, shape, dtype, fma):
    n, k = len(shape), 3
    case = _case(method, kind, shape, dtype, linearize=(method == "cubic"))
    fields = _fields(case, k, 5 + n)
    want = _fields_want(oracle, case, fields, fma)
    has_fused = method == "linear" and n in (2, 3)
    tname = "double" if dtype == np.float64 else "float"
    flags = f"{tname}, {n}, {'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>"
    fs = _fields_handle(case, fields, fma)
    try:
        assert (fs.get_option("fused_table_bytes") > 0) == has_fused
        for fused in ((1, 0) if has_fused else (0,)):
            fs.set_option("fused", fused)
            dev = fs.eval_tensors(_tensors(case.obs))
            fs.finish()
            assert fs.last_path == ("fused" if fused else "per_field")
            name = fs.kernel_name()
            assert (name == "interpn::k_linear_fields<" + flags) if fused else not name.startswith("interpn::k_linear_fields"), name
            _assert_same(dev.cpu().numpy(), want, (name, "device"))
            _assert_same(fs.eval_host(case.obs), want, (name, "host"))
        # point-major: (n, N) in, (n, K) out
        fs.set_option("fused", -1)
        pts = _rows(case.obs)
        for path in ((1, 2) if has_fused else (2,)):
            fs.set_option("points_path", path)
            fs.set_option("points_slice", 512)
            got = fs.eval_points_tensors(_tensors([pts])[0])
            fs.finish()
            assert fs.last_points_path == ("fused" if path == 1 else "split")
            name = fs.kernel_name()
            assert (name == "interpn::k_linear_fields_points<" + flags) if path == 1 else not name.startswith("interpn::k_linear_fields_points"), name
            _assert_same(got.cpu().numpy(), np.ascontiguousarray(want.T), (name, "points device"))
            _assert_same(fs.eval_points_host(pts), np.ascontiguousarray(want.T), (name, "points host"))
    finally:
        fs.close()


# ---- 10. lattices: eval_lattice (fused / expanded) and Fields.eval_lattice (fused / per-field, field-major and fields-last) ---------
LATTICES = [("linear", S2, [7, 65], False), ("linear", S3, [2, 7, 63], False), ("linear", LONG3, [7, 2, 64], False),
            ("cubic", S2, [7, 1000], False), ("cubic", S2, [7, 65], True), ("cubic", S3, [7, 1, 65], True),
            ("cubic", LONG3, [7, 7, 63], False), ("cubic", S4, [2, 3, 7, 63], True), ("linear", S4, [3, 2, 7, 65], False),
            ("nearest", S3, [7, 2, 65], False)]


def _lattice_kernel(prefix, dtype, method, n, kind, fma, tail=""):
    return (f"{prefix}{'double' if dtype == np.float64 else 'float'}, {0 if method == 'linear' else 1}, {n}, "
            f"{'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}{tail}>")


@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape,lens,linearize", LATTICES,
                         ids=[f"{m}-{'x'.join(map(str, s))}-{'lin' if lin else 'quad'}-{l[-1]}" for m, s, l, lin in LATTICES])
@pytest.mark.parametrize("kind", KINDS)
def test_lattices(oracle, kind, method, shape, lens, linearize, dtype, fma):
    n, k = len(shape), 3
    case = _case(method, kind, shape, dtype, nobs=16, linearize=linearize)
    axes = _lattice_axes(case, lens, 300 + n + lens[-1])
    points = _expand(axes)
    fields = np.concatenate([case.vals[None], _fields(case, k - 1, 9 + n)])
    want = _fields_want(oracle, case, fields, fma, obs=points).reshape((k,) + tuple(lens))
    has_fused = method != "nearest" and n in (2, 3)
    it = _handle(case, fma)
    try:
        for mode in ((1, 0) if has_fused else (0,)):
            it.set_option("lattice", mode)
            dev = it.eval_lattice_tensors(_tensors(axes))
            it.finish()
            assert it.last_lattice_path == ("fused" if mode else "expanded")
            name = it.kernel_name()
            if mode:
                assert name == _lattice_kernel("interpn::k_lattice_rows<", dtype, method, n, kind, fma), name
            else:
                assert not name.startswith("interpn::k_lattice"), name
            _assert_same(dev.cpu().numpy(), want[0], (name, "device"))
            _assert_same(it.eval_lattice_host(axes), want[0], (name, "host"))
    finally:
        it.close()
    fs = _fields_handle(case, fields, fma)
    try:
        for mode in ((1, 0) if has_fused else (0,)):
            fs.set_option("lattice", mode)
            for field_axis in (0, -1):
                dev = fs.eval_lattice_tensors(_tensors(axes), field_axis=field_axis)
                fs.finish()
                assert fs.last_lattice_path == ("fused" if mode else "per_field")
                name = fs.kernel_name()
                if mode:
                    assert name == _lattice_kernel("interpn::k_lattice_fields_rows<", dtype, method, n, kind, fma,
                                                   ", true" if field_axis else ", false"), name
                else:
                    assert not name.startswith("interpn::k_lattice_fields"), name
                w = want if field_axis == 0 else np.ascontiguousarray(np.moveaxis(want, 0, -1))
                _assert_same(dev.cpu().numpy(), w, (name, field_axis, "device"))
                _assert_same(fs.eval_lattice_host(axes, field_axis=field_axis), w, (name, field_axis, "host"))
    finally:
        fs.close()

