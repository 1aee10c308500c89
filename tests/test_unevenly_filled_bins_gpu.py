"""The sorted multicubic path — the counting sort of k_bin_points.hip, k_cubic_brick on the sorted copy, the persistent column
kernels k_cubic_column / k_cubic3_column — on batches that are NOT spread evenly over its bins (tests/helpers.py::skewed_obs;
tests/test_skewed_batches_cpu.py shows that every generator delivers the occupancy it names).  Every other test of this
path draws its points i.i.d. over the grid's extent: every bin then holds count / nbins points, none is empty, every chunk
of the scatter holds a little of every bin and every part of a column kernel but a bin's last is full.  Here: one bin holds
everything, most bins hold one point or none, a bin's count sits at a part size's edge, whole chunks rank into one counter,
every point lies outside the grid, a part's local sort has one key, a batch is one point repeated.

The contract these tests pin: the results of the sorted path do not depend on how the points are distributed over bins,
parts or phases.  Every evaluation (`_run`) asserts that the path and the kernel were the forced ones, that the result has
the oracle's bits (a NaN need only be a NaN) and the bits of the same handle with `binned` = 0, that the element in front of
and the one behind the result keep their sentinel, and that finish() succeeds; a failing batch (`_run_failing`) that
finish() raises with the smallest failing original index and that the results in front of it are right.

No test here or elsewhere depends on the order of the suite: it passes with this file collected in front of
tests/test_step_commands_gpu.py as well as behind everything.  The file's name sorts behind every older test file's only so
that the older GPU tests keep their numbers in the suite's order, by which runs of the suite are compared.

Grids and tables are the anisotropic ones (family_runs.skewed_case), the forms family_runs.SKEWED_FORMS; both kinds and
element types under fma, and one row without per form.  A class pair fixes the bin wherever the sort classifies exactly or
on the grid's own steps (the column forms; the tiled form on regular grids).  The tiled form on rectilinear grids bins by
the uniform grid over each axis' span — a locality hint — so a pair's points may there fall into a few neighbouring bins.

What no test here can tell apart, because the path treats its bins, parts, flags and local keys as hints and sends every
point that is not where the hint said to the table in global memory: a part cut elsewhere (the tail rule), a flag set or
missed, a scatter that reserves a run of zero points, the second load batch of pass 1 run with every lane masked.  Such
changes keep every bit; only losing or duplicating a slot of the sorted copy changes results (a part's last points dropped,
the out-of-cell test weakened: both fail here and in the uniform tests)."""

import numpy as np
import pytest

from tests import family_runs as fr
from tests.family_runs import KNOBS
from tests.helpers import class_pairs, run_oracle, skewed_obs

pytestmark = pytest.mark.gpu

ROWS = [("regular", np.float64, True), ("regular", np.float32, True), ("rectilinear", np.float64, True),
        ("rectilinear", np.float32, True), ("regular", np.float64, False)]
ROW_IDS = ["regular-f64-fma", "regular-f32-fma", "rectilinear-f64-fma", "rectilinear-f32-fma", "regular-f64-nofma"]
FORMS, FORM_IDS = fr.SKEWED_FORMS, fr.SKEWED_IDS
COLUMNS = [f for f in FORMS if f[0] == "column"]
COLUMN_IDS = [i for f, i in zip(FORMS, FORM_IDS) if f[0] == "column"]
SENTINEL = -5.0

# Option rows, cycled over the evaluations of a test (every row of a list sets the same keys).  Over the file: `deal` 0 and 1,
# `scatter_staged` 0 and 1 (beyond 1024 bins the direct scatter runs whatever it says), `bin_scramble` 1 (every fifth point
# in the next bin: the kernels' out-of-cell path), `column_pad` -1, 0 and 1.
SORTED_ROWS = [{"deal": 1, "bin_scramble": 0}, {"deal": 0, "bin_scramble": 0}, {"deal": 1, "bin_scramble": 1}]
COLUMN4_ROWS = [{"scatter_staged": 1, "column_pad": -1, "bin_scramble": 0, "deal": 1},
                {"scatter_staged": 0, "column_pad": 0, "bin_scramble": 0, "deal": 0},
                {"scatter_staged": 1, "column_pad": 1, "bin_scramble": 1, "deal": 1}]
COLUMN3_ROWS = [{"scatter_staged": 1, "bin_scramble": 0}, {"scatter_staged": 0, "bin_scramble": 1}]


def _option_rows(form, shape):
    return SORTED_ROWS if form == "sorted" else COLUMN4_ROWS if len(shape) == 4 else COLUMN3_ROWS


def _set(it, row):
    for k, v in row.items():
        it.set_option(k, v)


def _lin(kind, dtype, flip=0):
    """`linearize_extrapolation` of a test's handle: both values occur among the rows of every form."""
    return (int(kind == "rectilinear") + int(dtype == np.float32) + flip) % 2 == 0


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv("INTERPN_HIP_" + name, raising=False)


def _buffers(obs):
    import torch

    dev = fr.tensors(obs)
    full = torch.full((obs[0].size + 2,), SENTINEL, dtype=dev[0].dtype, device="cuda:0")
    return dev, full, full[1:1 + obs[0].size]  # the result is a view into a longer buffer


def _run(it, obs, want, kernel, what):
    dev, full, out = _buffers(obs)
    it.eval_tensors(dev, out)
    fr.assert_sorted(it, kernel)
    it.finish()
    got = out.cpu().numpy()
    fr.assert_same(got, want, (what, "oracle"))
    assert float(full[0]) == SENTINEL and float(full[-1]) == SENTINEL, what  # nothing outside the batch was written
    it.set_option("binned", 0)
    try:
        ref = it.eval_tensors(dev)
        it.finish()
        assert it.get_option("last_binned") == 0 and it.last_path != "binned", it.last_path
        fr.assert_same(ref.cpu().numpy(), got, (what, "the same handle, binned = 0"))
    finally:
        it.set_option("binned", 1)


def _run_failing(it, oracle, case, obs, first, fma, kernel, what):
    """Regular grids: the batch's first NaN is at original index `first`."""
    dev, full, out = _buffers(obs)
    it.eval_tensors(dev, out)
    fr.assert_sorted(it, kernel)
    with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as err:
        it.finish()
    assert err.value.first_bad_index == first, (what, err.value.first_bad_index, first)
    if first:
        want = run_oracle(oracle, fr.with_obs(case, [np.ascontiguousarray(o[:first]) for o in obs]), fma)
        fr.assert_same(out[:first].cpu().numpy(), want, (what, "prefix"))
    assert float(full[0]) == SENTINEL and float(full[-1]) == SENTINEL, what


def _check(oracle, it, case, obs, fma, kernel, what):
    _run(it, obs, run_oracle(oracle, fr.with_obs(case, obs), fma), kernel, what)


# ---- one_pair: everything in one bin, over the class pairs (the tail bins among them) -----------------------------------------------
@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", FORMS, ids=FORM_IDS)
def test_one_pair(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """3001 points in ONE class pair: every point of a chunk ranks into one LDS counter, every other bin is empty (`mine ?`
    guards, scans over zeros, part_prefix flat but for one step), the column kernels cut one bin into all the parts there are.
    One handle per `linearize` value, one evaluation per pair of family_runs.swept_pairs."""
    rows = _option_rows(form, shape)
    for linearize in (False, True):
        case = fr.skewed_case(kind, shape, dtype, linearize)
        rng = fr.skewed_rng(shape, 10, int(linearize))
        it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
        try:
            for k, pair in enumerate(fr.swept_pairs(shape)):
                _set(it, rows[k % len(rows)])
                _check(oracle, it, case, skewed_obs(case, "one_pair", rng, pair=pair, count=3001), fma, kernel, (linearize, pair, rows[k % len(rows)]))
        finally:
            it.close()


# ---- heavy: one bin at the edges of a part size, every other bin with one point -------------------------------------------------------
@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", COLUMNS, ids=COLUMN_IDS)
def test_heavy_bin_at_forced_part_sizes(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """`column_part` q = 64 and 1000, the heavy bin with c = q - 1, q, q + 1, 2 q, 2 q + 1 points (per = ceil(c / nparts) at
    its edges), every other bin a part of one point; the heavy pair the low corner, the high corner and an interior one.  The
    3-D kernel's part size is fixed (the option is the 4-D kernel's): there these are small bins beside singletons, its own
    part edges are those of test_heavy_bin_at_the_default_part_size."""
    rows = _option_rows(form, shape)
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype))
    rng = fr.skewed_rng(shape, 11)
    it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
    try:
        k = 0
        for q in (64, 1000):
            it.set_option("column_part", q)
            for pair in fr.heavy_pairs(shape):
                for c in (q - 1, q, q + 1, 2 * q, 2 * q + 1):
                    _set(it, rows[k % len(rows)])
                    k += 1
                    _check(oracle, it, case, skewed_obs(case, "heavy", rng, pair=pair, c=c), fma, kernel, (q, pair, c))
    finally:
        it.close()


def _tail_part(part, tail):
    """Points per part in a tail bin, by the rule of the sort's scan (k_bin_points.hip::k_bin_scan): `tail` = `column_tail`, the
    last 1 / (tail >> 4) of the bins are cut (tail & 15) times finer, but not below 1024 points — so a part size of 1024 or
    less is the same in every bin."""
    if tail >> 4 == 0:
        return part
    fine = part // ((tail & 15) or 1)
    return fine if fine > 1024 else min(part, 1024)


@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("tail", [0x84, 0x22, 0], ids=["tail84", "tail22", "tail0"])
def test_heavy_bin_in_every_place_of_the_order(oracle, monkeypatch, tail, kind, dtype, fma):
    """[6, 7, 5, 6]: every one of the 30 class pairs is the heavy one in turn, so the heavy bin is the first, the last and a tail
    bin at least once, wherever the device's scramble puts it.  `column_tail` 0x84: the last eighth of the bins cut four times
    finer, 0x22: the last half twice, 0: no tail.  At `column_part` 64 (129 points: three parts) the three settings cut alike —
    the tail's parts never go below 1024 points, `_tail_part` —, so they differ only in which bins the scan treats as tail; at
    `column_part` 8192 the tail's part is 2048, 4096 or 8192 points, and the heavy bin holds one point more than that: two
    parts where it is a tail bin, one elsewhere."""
    form, shape, layout, kernel = COLUMNS[0]
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype, 1))
    rng = fr.skewed_rng(shape, 12, tail)
    it = fr.sorted_handle(case, fma, monkeypatch, form, layout, {"column_tail": tail})
    try:
        assert it.get_option("col_part_points") > 8192  # else `column_part` 8192 would not be what cuts
        for part in (64, 8192):
            it.set_option("column_part", part)
            c = 129 if part == 64 else _tail_part(part, tail) + 1
            for k, pair in enumerate(class_pairs(case)):
                _set(it, COLUMN4_ROWS[k % 3])
                _check(oracle, it, case, skewed_obs(case, "heavy", rng, pair=pair, c=c), fma, kernel, (tail, part, pair, c))
    finally:
        it.close()


@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", COLUMNS, ids=COLUMN_IDS)
def test_heavy_bin_at_the_default_part_size(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """P = the kernel's own part size (`col_part_points`; 3-D: 16 x 256).  c = P / 2 - 1, P / 2, P / 2 + 1 (P / 2 = HB * GT:
    where pass 1 of the 4-D kernel skips its second batch of loads, exactly at equality), P - 1, P, P + 1, 2 P + 1.  4-D, under
    the default `column_tail` (0x84): T - 1, T and T + 1 points, T = the tail's part size (P / 4), in each of
    family_runs.swept_pairs in turn, so that a tail bin is the heavy one at each of the three counts ([6, 7, 5, 6]: every pair
    is run, so this is certain; [41, 40, 5, 6]: 24 of 1560 pairs, 195 of them tail bins)."""
    rows = _option_rows(form, shape)
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype))
    rng = fr.skewed_rng(shape, 13)
    it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
    try:
        P = it.get_option("col_part_points") if len(shape) == 4 else fr.COLUMN3_PART
        assert P >= 1024 and P % 4 == 0, P
        k = 0
        for pair in fr.heavy_pairs(shape):
            for c in (P // 2 - 1, P // 2, P // 2 + 1, P - 1, P, P + 1, 2 * P + 1):
                _set(it, rows[k % len(rows)])
                k += 1
                _check(oracle, it, case, skewed_obs(case, "heavy", rng, pair=pair, c=c), fma, kernel, (P, pair, c))
        if len(shape) == 4:
            T = _tail_part(P, 0x84)
            assert T == P // 4, (P, T)  # the tail is really cut finer at this part size
            _set(it, rows[0])
            for pair in fr.swept_pairs(shape):
                for c in (T - 1, T, T + 1):
                    _check(oracle, it, case, skewed_obs(case, "heavy", rng, pair=pair, c=c), fma, kernel, (P, pair, c, "tail"))
    finally:
        it.close()


# ---- one_each: batches as small as nbins ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", FORMS, ids=FORM_IDS)
def test_one_each(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """Exactly one, exactly two points per class pair, and one per pair with one pair left empty: every part of a column
    kernel is a part of one or two points, K-range phases without any point, and one hole in the scans."""
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype, 1))
    pairs = class_pairs(case)
    rng = fr.skewed_rng(shape, 14)
    it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
    try:
        for row in _option_rows(form, shape):
            _set(it, row)
            for kw in ({"k": 1}, {"k": 2}, {"k": 1, "empty": pairs[0]}, {"k": 1, "empty": pairs[-1]}, {"k": 1, "empty": pairs[len(pairs) // 2]}):
                _check(oracle, it, case, skewed_obs(case, "one_each", rng, **kw), fma, kernel, (row, kw))
    finally:
        it.close()


# ---- ordered, reversed, striped: what a producer that sorts its batch hands over -----------------------------------------------------
@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", FORMS, ids=FORM_IDS)
def test_ordered_reversed_striped(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """20 011 points already in bin order, in the reverse order, and in chunks of 4096 that hold a single pair each (two pairs
    in turn): every chunk of the scatter sees a narrow band of bins or one.  `ordered` once more at 150 011 points in slices of
    2^16: every slice holds a narrow band of bins, and finds the counters as the previous slice's scan left them."""
    rows = _option_rows(form, shape)
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype))
    two = (fr.swept_pairs(shape)[1], fr.swept_pairs(shape)[-1])
    it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
    try:
        for k, (dist, kw) in enumerate((("ordered", {}), ("reversed", {}), ("striped", {"pairs": two}))):
            _set(it, rows[k % len(rows)])
            _check(oracle, it, case, skewed_obs(case, dist, fr.skewed_rng(shape, 15), count=20_011, **kw), fma, kernel, dist)
        _set(it, rows[0])
        it.set_option("bin_slice_log2", 16)
        _check(oracle, it, case, skewed_obs(case, "ordered", fr.skewed_rng(shape, 16), count=150_011), fma, kernel, "ordered, sliced")
    finally:
        it.close()


# ---- outside0, one_outside: the bins' `outside` flags, all set and one set by a single point ---------------------------------------
@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", COLUMNS, ids=COLUMN_IDS)
def test_outside_along_axis_0(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """Every point outside the grid along axis 0 (every non-empty bin flagged; without `linearize` none is), and 3000 points
    inside class 0 with ONE point below the grid, which alone sets its bin's flag.  `column_coef` 1 (saturated parts rewrite
    their tiles as Hermite coefficients unless flagged) and 0."""
    rows = _option_rows(form, shape)
    for linearize in (True, False):
        case = fr.skewed_case(kind, shape, dtype, linearize)
        it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
        try:
            for k, coef in enumerate((1, 0)):
                it.set_option("column_coef", coef)
                _set(it, rows[(k + int(linearize)) % len(rows)])
                rng = fr.skewed_rng(shape, 17, coef)
                _check(oracle, it, case, skewed_obs(case, "outside0", rng, count=3001), fma, kernel, ("outside0", linearize, coef))
                _check(oracle, it, case, skewed_obs(case, "one_outside", rng), fma, kernel, ("one_outside", linearize, coef))
        finally:
            it.close()


# ---- local_one, local_ends: the column kernels' local order with one key, with the two outermost ----------------------------------
LOCAL_ROWS = [{"column_cpp": 1, "column_keys": 0, "column_groups": 1, "column_threads": 768},
              {"column_cpp": 0, "column_keys": 1, "column_groups": 2, "column_threads": 768},
              {"column_cpp": 1, "column_keys": 1, "column_groups": 1, "column_threads": 384},
              {"column_cpp": 0, "column_keys": 0, "column_groups": 2, "column_threads": 256},
              {"column_cpp": 2, "column_keys": 0, "column_groups": 1, "column_threads": 256}]


@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", COLUMNS, ids=COLUMN_IDS)
def test_one_class_on_the_local_axes(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """Inside one class pair every point of one class on axis 2 (4-D: and on axis 3) — a local sort whose keys are all equal, one
    K-range phase with all the points and the others with none (`column_cpp` 1: one class of axis 2 per phase) — and points of
    the first and the last class of axis 2 only (every phase in between empty).  4-D: the column resident whole or by phases,
    the keys from the records or the index words, one or two wave groups, 768 / 384 / 256 threads."""
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype, 1))
    pair = fr.heavy_pairs(shape)[2]
    m2 = shape[2] - 1
    classes2 = sorted({0, 1, m2 // 2, m2 - 1})
    rng = fr.skewed_rng(shape, 18)
    it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
    try:
        for k, row in enumerate(LOCAL_ROWS if len(shape) == 4 else COLUMN3_ROWS):
            _set(it, row)
            for c2 in classes2:
                c3 = (c2 + k) % (shape[3] - 1) if len(shape) == 4 else None
                _check(oracle, it, case, skewed_obs(case, "local_one", rng, pair=pair, c2=c2, c3=c3, count=3001), fma, kernel, (row, c2, c3))
            _check(oracle, it, case, skewed_obs(case, "local_ends", rng, pair=pair, count=3001), fma, kernel, (row, "ends"))
    finally:
        it.close()


# ---- identical, on_nodes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", FORMS, ids=FORM_IDS)
def test_identical_points_and_points_on_nodes(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """One point 3001 times (inside an interior cell; a grid node on every axis; beyond the high corner), and 3001 points whose
    every coordinate is a node of its axis: the class boundaries, where the sort's estimate and the kernel's exact class may
    differ and the out-of-cell path runs."""
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype))
    rng = fr.skewed_rng(shape, 19)
    it = fr.sorted_handle(case, fma, monkeypatch, form, layout)
    try:
        for row in _option_rows(form, shape)[:2]:
            _set(it, row)
            for which in ("interior", "node", "beyond"):
                _check(oracle, it, case, skewed_obs(case, "identical", rng, which=which, count=3001), fma, kernel, (row, which))
            _check(oracle, it, case, skewed_obs(case, "on_nodes", rng, count=3001), fma, kernel, (row, "on_nodes"))
    finally:
        it.close()


# ---- nan0, half_nan0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form,shape,layout,kernel", FORMS, ids=FORM_IDS)
def test_nan_on_axis_0_propagates_on_rectilinear_grids(oracle, monkeypatch, form, shape, layout, kernel, dtype):
    """NaN on axis 0 for every point (one bin: the search puts NaN into the first class), and for every second point of the
    second half: rectilinear grids never fail per point."""
    case = fr.skewed_case("rectilinear", shape, dtype, _lin("rectilinear", dtype))
    it = fr.sorted_handle(case, True, monkeypatch, form, layout)
    try:
        for k, row in enumerate(_option_rows(form, shape)[:2]):
            _set(it, row)
            for dist in ("nan0", "half_nan0"):
                obs = skewed_obs(case, dist, fr.skewed_rng(shape, 20, k), count=3001)
                want = run_oracle(oracle, fr.with_obs(case, obs), True)
                assert np.array_equal(np.isnan(want), np.isnan(obs[0]))
                _run(it, obs, want, kernel, (row, dist))
    finally:
        it.close()


FAILING = [FORMS[2], FORMS[4], FORMS[6]]  # one sorted form and the two column kernels


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form,shape,layout,kernel", FAILING, ids=[FORM_IDS[2], FORM_IDS[4], FORM_IDS[6]])
def test_first_failing_index_on_regular_grids(oracle, monkeypatch, form, shape, layout, kernel, dtype):
    """Regular grids: finish() reports the smallest failing ORIGINAL index although the points were evaluated in bin order,
    and the results in front of it are right — every second point of the second half NaN, every point NaN (index 0), and a
    single NaN at index k of a batch that sits in one bin (k = 0, inside the first chunk, the last point)."""
    case = fr.skewed_case("regular", shape, dtype, _lin("regular", dtype))
    count = 5001
    it = fr.sorted_handle(case, True, monkeypatch, form, layout)
    try:
        for k, row in enumerate(_option_rows(form, shape)[:2]):
            _set(it, row)
            for dist, first in (("half_nan0", count // 2), ("nan0", 0)):
                obs = skewed_obs(case, dist, fr.skewed_rng(shape, 21, k), count=count)
                _run_failing(it, oracle, case, obs, first, True, kernel, (row, dist))
            pair = fr.heavy_pairs(shape)[k]
            for at in (0, 777, count - 1):
                obs = skewed_obs(case, "one_pair", fr.skewed_rng(shape, 22, k), pair=pair, count=count)
                obs[1 + at % (len(shape) - 1)][at] = np.nan
                _run_failing(it, oracle, case, obs, at, True, kernel, (row, "one_pair", at))
            # the handle is as good as before
            _check(oracle, it, case, skewed_obs(case, "one_pair", fr.skewed_rng(shape, 23, k), pair=pair, count=count), True, kernel, (row, "after"))
    finally:
        it.close()


# ---- the shared forcing of tests/family_runs.py, with further options, on skewed batches ---------------------------------------------
@pytest.mark.parametrize("kind,dtype,fma", ROWS, ids=ROW_IDS)
@pytest.mark.parametrize("form,shape,layout,kernel", FORMS, ids=FORM_IDS)
def test_dealt_out_or_not(oracle, monkeypatch, form, shape, layout, kernel, kind, dtype, fma):
    """family_runs.sorted_and_column_multicubic (`deal` 1 and 0, as tests/test_anisotropic_gpu.py runs it) with its `options`
    on a batch in bin order and on two points per bin; every evaluation is `_run`'s.  (`scatter_staged` and `column_pad` are
    the column forms' options: the tiled form has one scatter kernel.)"""
    case = fr.skewed_case(kind, shape, dtype, _lin(kind, dtype, 1))
    rng = fr.skewed_rng(shape, 24)
    for options, obs in (({"bin_scramble": 1, "scatter_staged": 0}, skewed_obs(case, "ordered", rng, count=5000)),
                         ({"scatter_staged": 1, "column_pad": 0}, skewed_obs(case, "one_each", rng, k=2))):
        batch = fr.with_obs(case, obs)
        fr.sorted_and_column_multicubic(batch, run_oracle(oracle, batch, fma), fma, monkeypatch, form, layout, kernel, options=options, run=_run)
