"""Every value family of tests/test_anisotropic_gpu.py (§1 - 6, §8 values, §9, §10) on tables with NaN and ±inf nodes,
forced exactly as there: the bodies, with their layouts, options and kernel-name / path assertions, are those of
tests/family_runs.py.  Every finite node stays U(-1, 1) (tests/helpers.py::poison_table).

Most kernels do not evaluate a point from its own loads alone: brick and tile gathers are shared between lanes, the sweep
kernels reorder 1024 points per wave, the column kernels rewrite table lines as coefficients shared by a part, the lattice
kernels keep per-row partials in LDS, a field set keeps K fields in one line, the cubic node form computes every saturation
class and selects one.  A value "discarded" by a multiply instead of a select, a neighbour lane's or field's NaN coming
through a shuffle, or a fallback taken for the wrong lane leaks a NaN into a point that must stay finite, or loses one; a
finite table cannot show it.  So every result gets three assertions (tests/family_runs.py::assert_same with an Expect):

  - bit-identical to the oracle on the same poisoned table (a NaN need only be a NaN; the sign of an infinity counts);
  - non-finite exactly where tests/helpers.py::footprint_poisoned says (linear and cubic; nearest has oracle parity only);
  - at every other point, the bits of the oracle on the CLEAN table.

tests/test_table_nonfinite_cpu.py shows the oracle and the rule to agree on these tables.  A status other than success —
on regular grids "Unrepresentable coordinate value", which is about coordinates only — raises in the bodies' calls.

The "nan" table on f64-fma, f32-fma and f64-nofma, the "mixed" one (NaN / +inf / -inf) on f64-fma; "plane" tables (one whole
hyperplane NaN, index 3 of the longest axis: the unused fourth node of the saturated first cell) on f64-fma, for the brick
layouts of §1 and the cubic families of §2 - 4.  Field sets: field 0 clean, fields 1 and 2 poisoned at different nodes."""

import dataclasses

import numpy as np
import pytest

from tests import family_runs as fr
from tests.family_runs import KNOBS, LONG3, NPTS, S2, S3, S4, S5, S6
from tests.helpers import anisotropic_axis, anisotropic_points, footprint_cells, footprint_poisoned, poison_table, run_hip_raw
from tests.kat import Case

pytestmark = pytest.mark.gpu

TABLES = [("nan", np.float64, True), ("nan", np.float32, True), ("nan", np.float64, False), ("mixed", np.float64, True)]
TIDS = ["nan-f64-fma", "nan-f32-fma", "nan-f64-nofma", "mixed-f64-fma"]
KINDS = ["regular", "rectilinear"]
tables = pytest.mark.parametrize("table,dtype,fma", TABLES, ids=TIDS)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv("INTERPN_HIP_" + name, raising=False)


def _poisoned(oracle, clean, table, fma, seed=0):
    """(case, want): `clean` with its table poisoned, and the Expect of it; the inputs are checked to probe both sides."""
    case = fr.poisoned_case(clean, table, seed)
    want = fr.expect(oracle, case, clean, fma)
    bad = ~np.isfinite(want.oracle)
    assert bad.any() and not bad.all(), (int(bad.sum()), bad.size)
    return case, want


def _field_set(oracle, clean, fields, table, fma, obs=None):
    """K = 3 tables: field 0 as it is, fields 1 and 2 poisoned at different nodes.  (fields, want) with want of (K, n).
    A lattice has few distinct coordinates per axis, and two poisoned nodes can lie where none of its points reaches them: each
    field takes the first of its ten placement seeds at which the oracle has points of both sorts."""
    obs = clean.obs if obs is None else obs
    at = lambda vals: dataclasses.replace(clean, vals=vals, obs=obs)
    out, wants = [fields[0]], [fr.expect(oracle, at(fields[0]), at(fields[0]), fma)]
    for i, before in enumerate(fields[1:]):
        for seed in range(10):
            f = poison_table(before, clean.dims, clean.method, fr.POISON_SEED + 50 + 10 * i + seed, table)
            want = fr.expect(oracle, at(f), at(before), fma)
            bad = ~np.isfinite(want.oracle)
            if bad.any() and not bad.all():
                break
        else:
            raise AssertionError("no placement reaches some but not all points")
        out.append(f)
        wants.append(want)
    assert np.isfinite(out[0]).all() and not np.array_equal(np.isfinite(out[1]), np.isfinite(out[2]))
    return np.stack(out), fr.stacked(wants)


# ---- 1. multilinear N = 2..6: the C-order kernels and the brick kernels ------------------------------------------------------------------
@tables
@pytest.mark.parametrize("shape,layout", [(s, l) for s in (S2, S3, S4, S5, S6, LONG3) for l in ("off", "bricks", "c4") if l != "c4" or len(s) >= 4],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
@pytest.mark.parametrize("kind", KINDS)
def test_multilinear_c_order_and_bricks(oracle, monkeypatch, kind, shape, layout, table, dtype, fma):
    case, want = _poisoned(oracle, fr.make_case("linear", kind, shape, dtype), table, fma)
    fr.multilinear_c_order_and_bricks(case, want, fma, monkeypatch, kind, layout)


# ---- 2. multicubic N = 2..4: the C-order kernels and the tiled kernel --------------------------------------------------------------------
@tables
@pytest.mark.parametrize("linearize", [False, True], ids=["quad", "lin"])
@pytest.mark.parametrize("layout", ["off", "44", "24", "11"])
@pytest.mark.parametrize("shape", [S2, S3, S4, LONG3], ids=str)
@pytest.mark.parametrize("kind", KINDS)
def test_multicubic_c_order_and_tiles(oracle, monkeypatch, kind, shape, layout, linearize, table, dtype, fma):
    case, want = _poisoned(oracle, fr.make_case("cubic", kind, shape, dtype, linearize=linearize), table, fma)
    fr.multicubic_c_order_and_tiles(case, want, fma, monkeypatch, kind, layout)


# ---- 3. sorted and column multicubic -------------------------------------------------------------------------------------------------------
@tables
@pytest.mark.parametrize("form,shape,layout,kernel", fr.SORTED, ids=[f"{f}-N{len(s)}" for f, s, _, _ in fr.SORTED])
@pytest.mark.parametrize("kind", KINDS)
def test_sorted_and_column_multicubic(oracle, monkeypatch, kind, form, shape, layout, kernel, table, dtype, fma):
    clean = fr.make_case("cubic", kind, shape, dtype, nobs=fr.SORTED_NOBS, linearize=(len(shape) == 3))
    case, want = _poisoned(oracle, clean, table, fma)
    fr.sorted_and_column_multicubic(case, want, fma, monkeypatch, form, layout, kernel)


# ---- 4. the sweep family ----------------------------------------------------------------------------------------------------------------------
@tables
@pytest.mark.parametrize("method,kind,shape,options,kernel", fr.SWEEPS, ids=fr.SWEEP_IDS)
def test_sweep_family(oracle, monkeypatch, method, kind, shape, options, kernel, table, dtype, fma):
    for linearize in ((False, True) if method == "cubic" else (False,)):
        clean = fr.make_case(method, kind, shape, dtype, nobs=fr.SWEEP_NOBS, linearize=linearize)
        case, want = _poisoned(oracle, clean, table, fma)
        fr.sweep_family(case, want, fma, monkeypatch, kind, options, kernel)


# ---- 5. rectilinear search forms ------------------------------------------------------------------------------------------------------------
@tables
@pytest.mark.parametrize("axis_regs", ["0", "1", "2"])
@pytest.mark.parametrize("method,shape", fr.AXIS_SEARCH, ids=str)
def test_lane_resident_axis_search(oracle, monkeypatch, method, shape, axis_regs, table, dtype, fma):
    case, want = _poisoned(oracle, fr.make_case(method, "rectilinear", shape, dtype), table, fma)
    fr.lane_resident_axis_search(case, want, fma, monkeypatch, axis_regs)


@tables
@pytest.mark.parametrize("method,shape", fr.BUCKETS, ids=str)
@pytest.mark.parametrize("spacing", ["jittered", "rectilinear"])
def test_bucket_records_and_lds_search(oracle, monkeypatch, spacing, method, shape, table, dtype, fma):
    case, want = _poisoned(oracle, fr.make_case(method, spacing, shape, dtype), table, fma)
    fr.bucket_records_and_lds_search(case, want, fma, monkeypatch, spacing)


@tables
@pytest.mark.parametrize("d,n", [(0, 300), (1, 300), (2, 300), (0, 9), (2, 3), (1, 2)])
def test_linear_1d_records(oracle, monkeypatch, d, n, table, dtype, fma):
    """The axes, tables and points of the anisotropic test; one bucket record holds a node pair, so a non-finite node sits
    in two records.  On the axes of 2 and 3 nodes one poisoned node can reach every point; the longer ones have both sorts."""
    rng = np.random.default_rng(40 + d)
    g = anisotropic_axis(d, n, "rectilinear", dtype, rng)
    vals = rng.uniform(-1, 1, n).astype(dtype)
    x = anisotropic_points(g, NPTS, rng, dtype)
    clean = Case("aniso_linear_records", "linear", "rectilinear", [g], vals, [x], np.zeros(NPTS, dtype=dtype), 0.0)
    case = fr.poisoned_case(clean, table, d)
    want = fr.expect(oracle, case, clean, fma)
    assert want.touched.any() and (n <= 3 or not want.touched.all())
    fr.linear_1d_records(g, case.vals, x, want, fma, monkeypatch)


# ---- 6. the recursive arm: both forms of k_generic_n and the runtime-N kernel ----------------------------------------------------------
@tables
@pytest.mark.parametrize("form", ["onetree", "rowvec", "runtime"])
@pytest.mark.parametrize("method,shape", fr.RECURSIVE, ids=["linear7", "cubic5"])
@pytest.mark.parametrize("kind", KINDS)
def test_recursive_arm(oracle, monkeypatch, kind, method, shape, form, table, dtype, fma):
    fr.recursive_arm_env(monkeypatch, form)
    for linearize in ((False, True) if method == "cubic" else (False,)):
        case, want = _poisoned(oracle, fr.make_case(method, kind, shape, dtype, linearize=linearize), table, fma)
        fr.recursive_arm(case, want, fma, monkeypatch, form)


# ---- 8. point-major points: eval_points, fused and split ---------------------------------------------------------------------------------
@tables
@pytest.mark.parametrize("method,shape,bricks", fr.POINTS, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s, _ in fr.POINTS])
@pytest.mark.parametrize("kind", KINDS)
def test_point_major_values(oracle, monkeypatch, kind, method, shape, bricks, table, dtype, fma):
    case, want = _poisoned(oracle, fr.make_case(method, kind, shape, dtype, linearize=(method == "cubic")), table, fma)
    fr.point_major_values(case, want, fma, monkeypatch, bricks)


# ---- 9. field sets: a NaN must not cross fields inside one line of the fused table ----------------------------------------------------
@tables
@pytest.mark.parametrize("method,shape", fr.FIELD_SHAPES, ids=[f"{m}-{'x'.join(map(str, s))}" for m, s in fr.FIELD_SHAPES])
@pytest.mark.parametrize("kind", KINDS)
def test_field_sets(oracle, kind, method, shape, table, dtype, fma):
    clean = fr.make_case(method, kind, shape, dtype, linearize=(method == "cubic"))
    fields, want = _field_set(oracle, clean, fr.random_fields(clean, 3, 5 + len(shape)), table, fma)
    assert np.isfinite(want.oracle[0]).all() and (~np.isfinite(want.oracle[1:])).any(axis=1).all()
    fr.field_sets(clean, fields, want, fma, kind)


# ---- 10. lattices: eval_lattice on a poisoned table; Fields.eval_lattice on a clean field and two poisoned ones ----------------------
@tables
@pytest.mark.parametrize("method,shape,lens,linearize", fr.LATTICES, ids=fr.LATTICE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_lattices(oracle, kind, method, shape, lens, linearize, table, dtype, fma):
    n, k = len(shape), 3
    clean = fr.make_case(method, kind, shape, dtype, nobs=16, linearize=linearize)
    axes = fr.lattice_axes(clean, lens, 300 + n + lens[-1])
    fields = np.concatenate([fr.random_fields(clean, 1, 8 + n), clean.vals[None], fr.random_fields(clean, 1, 9 + n)])
    fields, want = _field_set(oracle, clean, fields, table, fma, obs=fr.expand(axes))
    want = fr.arranged(want, lambda a: a.reshape((k,) + tuple(lens)))
    assert np.isfinite(want.oracle[0]).all() and (~np.isfinite(want.oracle[1:])).reshape(2, -1).any(axis=1).all()
    fr.lattices(dataclasses.replace(clean, vals=fields[1]), axes, fields, want, fma, kind, own=1)


# ---- one-shot and host entry points, once per method -----------------------------------------------------------------------------------
@tables
@pytest.mark.parametrize("method", ["linear", "cubic", "nearest"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_shot_and_host_calls(oracle, kind, method, table, dtype, fma):
    """The raw one-shot entry point (it builds its own handle; fma only) and `eval_host` of a resident handle."""
    case, want = _poisoned(oracle, fr.make_case(method, kind, S3, dtype, linearize=(method == "cubic")), table, fma)
    if fma:
        fr.assert_same(run_hip_raw(case), want, "raw")
    it = fr.make_handle(case, fma)
    try:
        fr.assert_same(it.eval_host(case.obs, np.zeros(NPTS, dtype=dtype)), want, "host")
    finally:
        it.close()


# ---- planes ------------------------------------------------------------------------------------------------------------------------------------
def _run_family(row, case, want, fma, monkeypatch):
    family, sub, method, kind = row[:4]
    if family == "bricks":
        fr.multilinear_c_order_and_bricks(case, want, fma, monkeypatch, kind, sub[0])
    elif family == "tiles":
        for layout in sub:
            fr.multicubic_c_order_and_tiles(case, want, fma, monkeypatch, kind, layout)
    elif family == "sorted":
        fr.sorted_and_column_multicubic(case, want, fma, monkeypatch, sub[0], sub[2], sub[3])
    else:
        fr.sweep_family(case, want, fma, monkeypatch, kind, sub[3], sub[4])


@pytest.mark.parametrize("row", list(fr.plane_cases()), ids=fr.plane_id)
def test_plane_tables(oracle, monkeypatch, row):
    """Every node with index 3 along the longest axis NaN (f64, fma).  Points in that axis's first cell, and below the grid,
    stay finite: for multicubic node 3 is the fourth node of the saturated cell, which a select drops.  The counts of finite
    and non-finite points are asserted on the oracle in tests/test_table_nonfinite_cpu.py::test_plane_tables."""
    family, sub, method, kind, shape, nobs, linearize = row
    clean = fr.make_case(method, kind, shape, np.float64, nobs=nobs, linearize=linearize)
    case, want = _poisoned(oracle, clean, "plane", True)
    first = footprint_cells(case)[int(np.argmax(shape))] == 0
    assert first.any() and not want.touched[first].any() and np.isfinite(want.oracle[first]).all()
    _run_family(row, case, want, True, monkeypatch)


BESIDE = [row for row in fr.plane_cases() if row[2] == "cubic" and row[3] == "rectilinear"]


@pytest.mark.parametrize("dtype,fma", [(np.float64, True), (np.float32, True), (np.float64, False)], ids=["f64-fma", "f32-fma", "f64-nofma"])
@pytest.mark.parametrize("row", BESIDE, ids=fr.plane_id)
def test_points_beside_a_plane(oracle, monkeypatch, row, dtype, fma):
    """The rectilinear multicubic brick and sweep kernels compute a node's spacing-ratio quotients in a short form and
    evaluate a WAVE again, as the reference writes it, when one of its lanes has a numerator that form does not take — a
    NaN among them.  On the tables above nearly every wave holds a lane that touches a non-finite node, and a touched
    lane next to an untouched one is what those runs test.  Here no point touches one: every point of the plane case
    whose footprint holds a non-finite node is moved, along the longest axis, into the first cell or below the grid —
    and, on axes of 7 nodes or more, where node n - 4 is NaN as well, into the last cell or above the grid.  Those lanes
    are of the saturated classes, and the node they do not use (the fourth of Low, the first of High) is NaN in every
    wave: its differences are computed and must be dropped by a select, in whichever of the two evaluations a wave ends.
    Every result is finite and has the clean table's bits.  (With `0 * v3` added to the Low class's result of
    `cubic_rect_node`, 42 of these 57 cases fail; the same in `cubic_rect_node_fast` fails none of this file's tests: a
    wave whose 4^N gathers hold a non-finite value, used or not, ends in the second evaluation.)"""
    family, sub, method, kind, shape, nobs, linearize = row
    clean = fr.make_case(method, kind, shape, dtype, nobs=nobs, linearize=linearize)
    d = int(np.argmax(shape))
    n, g = shape[d], clean.grids[d]
    vals = poison_table(clean.vals, shape, method, 0, "plane")
    if n >= 7:
        vals.reshape(shape)[(slice(None),) * d + (n - 4,)] = np.nan
    hit = np.flatnonzero(footprint_poisoned(dataclasses.replace(clean, vals=vals)))
    rng = np.random.default_rng(77 + n)
    w = 0.2 * (float(g[-1]) - float(g[0]))
    low = np.minimum(rng.uniform(float(g[0]) - w, float(g[1]), hit.size).astype(dtype), g[1])
    high = np.maximum(rng.uniform(float(g[-2]), float(g[-1]) + w, hit.size).astype(dtype), np.nextafter(g[-2], dtype(np.inf)))
    x = clean.obs[d].copy()
    x[hit] = np.where((rng.random(hit.size) < 0.5) & (n >= 7), high, low)
    obs = [x if e == d else o for e, o in enumerate(clean.obs)]
    clean = dataclasses.replace(clean, obs=obs)
    case = dataclasses.replace(clean, vals=vals)
    want = fr.expect(oracle, case, clean, fma)
    cells = footprint_cells(case)[d]
    assert hit.size >= 20 and (cells == 0).sum() >= 20 and (n < 7 or (cells == n - 2).sum() >= 20)
    assert not want.touched.any() and np.isfinite(want.oracle).all() and np.array_equal(fr.bits(want.oracle), fr.bits(want.clean))
    _run_family(row, case, want, fma, monkeypatch)
