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

import numpy as np
import pytest

from tests import cubic_grad_restatement as cg
from tests import family_runs as fr
from tests import grad_restatement as gr
from tests.family_runs import KNOBS, LONG2, LONG3, NPTS, S2, S3, S4, S5, S6
from tests.helpers import anisotropic_axis, anisotropic_points, run_oracle

pytestmark = pytest.mark.gpu

VARIANTS = [(np.float64, True), (np.float32, True), (np.float64, False)]
VIDS = ["f64-fma", "f32-fma", "f64-nofma"]
KINDS = ["regular", "rectilinear"]
SORTED, SWEEPS, POINTS, FIELD_SHAPES, LATTICES = fr.SORTED, fr.SWEEPS, fr.POINTS, fr.FIELD_SHAPES, fr.LATTICES
# The value families' bodies (layouts, options, kernel-name and path assertions) are in tests/family_runs.py, shared with
# tests/test_table_nonfinite_gpu.py.
_assert_same, _case, _handle, _tensors, _rows = fr.assert_same, fr.make_case, fr.make_handle, fr.tensors, fr.rows


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv("INTERPN_HIP_" + name, raising=False)


def _grad_want(case, fma):
    out, grad, ok = (gr if case.method == "linear" else cg).eval_grad_case(case, fma=fma)
    assert ok.all()
    return out, np.ascontiguousarray(grad)


# ---- 1. multilinear N = 2..6: the C-order kernels and the brick kernels (test_linear_brick_layouts, test_linear2_brick) -------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("shape,layout", [(s, l) for s in (S2, S3, S4, S5, S6, LONG3) for l in ("off", "bricks", "c4") if l != "c4" or len(s) >= 4],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))  # (the 4-D cell bricks exist for N >= 4)
@pytest.mark.parametrize("kind", KINDS)
def test_multilinear_c_order_and_bricks(oracle, monkeypatch, kind, shape, layout, dtype, fma):
    case = _case("linear", kind, shape, dtype)
    fr.multilinear_c_order_and_bricks(case, run_oracle(oracle, case, fma), fma, monkeypatch, kind, layout)


# ---- 2. multicubic N = 2..4: the C-order kernels and the tiled kernel (test_cubic_tile_layouts) -----------------------------------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("linearize", [False, True], ids=["quad", "lin"])
@pytest.mark.parametrize("layout", ["off", "44", "24", "11"])
@pytest.mark.parametrize("shape", [S2, S3, S4, LONG3], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_multicubic_c_order_and_tiles(oracle, monkeypatch, kind, shape, layout, linearize, dtype, fma):
    case = _case("cubic", kind, shape, dtype, linearize=linearize)
    fr.multicubic_c_order_and_tiles(case, run_oracle(oracle, case, fma), fma, monkeypatch, kind, layout)


# ---- 3. sorted and column multicubic (test_binned_multicubic_evaluation, test_column_evaluation_of_sorted_{4d,3d}_multicubic) ------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("form,shape,layout,kernel", SORTED, ids=[f"{f}-N{len(s)}" for f, s, _, _ in SORTED])
@pytest.mark.parametrize("kind", KINDS)
def test_sorted_and_column_multicubic(oracle, monkeypatch, kind, form, shape, layout, kernel, dtype, fma):
    case = _case("cubic", kind, shape, dtype, nobs=fr.SORTED_NOBS, linearize=(len(shape) == 3))
    fr.sorted_and_column_multicubic(case, run_oracle(oracle, case, fma), fma, monkeypatch, form, layout, kernel)


# ---- 4. the sweep family (test_sweep_evaluation, test_linear2_sweep_evaluation, test_nearest_sweep_evaluation,
#         test_cubic_sweep_evaluation, test_cubic2_sweep_evaluation): their grids, 3001 points = several ragged rounds -----------------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,kind,shape,options,kernel", SWEEPS,
                         ids=[f"{m}{len(s)}-{k}-{'x'.join(map(str, s))}" + "".join(f"-{a}{b}" for a, b in o.items()) for m, k, s, o, _ in SWEEPS])
def test_sweep_family(oracle, monkeypatch, method, kind, shape, options, kernel, dtype, fma):
    for linearize in ((False, True) if method == "cubic" else (False,)):
        case = _case(method, kind, shape, dtype, nobs=fr.SWEEP_NOBS, linearize=linearize)
        fr.sweep_family(case, run_oracle(oracle, case, fma), fma, monkeypatch, kind, options, kernel)


# ---- 5. rectilinear search forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("axis_regs", ["0", "1", "2"])
@pytest.mark.parametrize("method,shape", [("linear", S2), ("linear", [64, 7]), ("linear", S3), ("linear", S4), ("linear", S6),
                                          ("linear", LONG3), ("nearest", [64]), ("nearest", S2), ("nearest", S3), ("nearest", S6),
                                          ("nearest", LONG2)], ids=str)
def test_lane_resident_axis_search(oracle, monkeypatch, method, shape, axis_regs, dtype, fma):
    """INTERPN_HIP_AXIS_REGS = 0 (LDS), 1 (probe sequence across lanes), 2 (lane tables), as
    test_lane_resident_axes_everywhere sets it: the brick kernels and the nearest kernel; a 70-point axis keeps the LDS search."""
    case = _case(method, "rectilinear", shape, dtype)
    fr.lane_resident_axis_search(case, run_oracle(oracle, case, fma), fma, monkeypatch, axis_regs)


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
    case = _case(method, spacing, shape, dtype)
    fr.bucket_records_and_lds_search(case, run_oracle(oracle, case, fma), fma, monkeypatch, spacing)


@pytest.mark.parametrize("dtype,fma", VARIANTS + [(np.float32, False)], ids=VIDS + ["f32-nofma"])
@pytest.mark.parametrize("d,n", [(0, 300), (1, 300), (2, 300), (0, 9), (2, 3), (1, 2)])
def test_linear_1d_records(oracle, monkeypatch, d, n, dtype, fma):
    """1-D multilinear from one record per search bucket (test_linear_1d_rectilinear_records: INTERPN_HIP_BRICKS=on), on each
    of the three spacings: growing, shrinking, clustered (twenty intervals at 1e-3 of the others)."""
    rng = np.random.default_rng(40 + d)
    g = anisotropic_axis(d, n, "rectilinear", dtype, rng)
    vals = rng.uniform(-1, 1, n).astype(dtype)
    x = anisotropic_points(g, NPTS, rng, dtype)
    want = np.zeros(NPTS, dtype=dtype)
    oracle.linear_rectilinear([g], vals, [x], want, fma=fma)
    fr.linear_1d_records(g, vals, x, want, fma, monkeypatch)


# ---- 6. the recursive arm: N = 7 multilinear, N = 5 multicubic, both forms of k_generic_n (test_recursive_arm_forms) and the
#         runtime-N kernel (test_recursive_arms) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("form", ["onetree", "rowvec", "runtime"])
@pytest.mark.parametrize("method,shape", [("linear", [3, 2, 3, 2, 3, 2, 3]), ("cubic", [4, 5, 4, 5, 4])], ids=["linear7", "cubic5"])
@pytest.mark.parametrize("kind", KINDS)
def test_recursive_arm(oracle, monkeypatch, kind, method, shape, form, dtype, fma):
    fr.recursive_arm_env(monkeypatch, form)
    for linearize in ((False, True) if method == "cubic" else (False,)):
        case = _case(method, kind, shape, dtype, linearize=linearize)
        fr.recursive_arm(case, run_oracle(oracle, case, fma), fma, monkeypatch, form)


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
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape,bricks", POINTS, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s, _ in POINTS])
@pytest.mark.parametrize("kind", KINDS)
def test_point_major_values(oracle, monkeypatch, kind, method, shape, bricks, dtype, fma):
    case = _case(method, kind, shape, dtype, linearize=(method == "cubic"))
    fr.point_major_values(case, run_oracle(oracle, case, fma), fma, monkeypatch, bricks)


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
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape", FIELD_SHAPES, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s in FIELD_SHAPES])
@pytest.mark.parametrize("kind", KINDS)
def test_field_sets(oracle, kind, method, shape, dtype, fma):
    case = _case(method, kind, shape, dtype, linearize=(method == "cubic"))
    fields = fr.random_fields(case, 3, 5 + len(shape))
    fr.field_sets(case, fields, fr.fields_want(oracle, case, fields, fma), fma, kind)


# ---- 10. lattices: eval_lattice (fused / expanded) and Fields.eval_lattice (fused / per-field, field-major and fields-last) ---------
@pytest.mark.parametrize("dtype,fma", VARIANTS, ids=VIDS)
@pytest.mark.parametrize("method,shape,lens,linearize", LATTICES,
                         ids=[f"{m}-{'x'.join(map(str, s))}-{'lin' if lin else 'quad'}-{l[-1]}" for m, s, l, lin in LATTICES])
@pytest.mark.parametrize("kind", KINDS)
def test_lattices(oracle, kind, method, shape, lens, linearize, dtype, fma):
    n, k = len(shape), 3
    case = _case(method, kind, shape, dtype, nobs=16, linearize=linearize)
    axes = fr.lattice_axes(case, lens, 300 + n + lens[-1])
    fields = np.concatenate([case.vals[None], fr.random_fields(case, k - 1, 9 + n)])
    want = fr.fields_want(oracle, case, fields, fma, obs=fr.expand(axes)).reshape((k,) + tuple(lens))
    fr.lattices(case, axes, fields, want, fma, kind)
