"""The slice paths on top of the large-batch paths.  Where no fused kernel exists, the point-major (`eval_points_*`), lattice
(`eval_lattice_*`, expanded) and field-set (per-field) entry points cut the batch into slices held in a scratch block of the
handle and hand every slice to `interpn_hip_eval_device_ex`, which may itself take the sweep kernels, the counting-sorted
multicubic evaluation or the LDS-column evaluation: a second scratch block of the same handle, the first-failing-index word
shifted by the outer slice and reported out of table order by the inner one, 16-byte alignment of `out + begin`, NO_ALLOC and
stream capture passed on.  The large-batch paths are forced at small sizes (options `sweep`, `binned`, `column`,
`bin_slice_log2`) under small outer slices (`points_path` = 2, `points_slice`; `lattice` = 0; `fused` = 0).

Every result is compared BIT FOR BIT (a NaN need only be a NaN on both sides) with the oracle on the de-interleaved or
expanded points, all of them, and with the same handle's `eval_tensors` with `sweep` = `binned` = `column` = 0.  No test may
pass by falling back: the handle's counters (`evals_sweep`, `evals_binned`, `evals_in_place`) say which path every slice took.

The two-slice lattices (3.4e6 f64 / 5.8e6 f32 points against the oracle) are the longest tests here: DESIGN.md section 10.
"""

import dataclasses

import numpy as np
import pytest

from tests.helpers import run_oracle, synthetic_case
from tests.test_lattice_gpu import _axes, _expand

pytestmark = pytest.mark.gpu

SLICE = 4096
NPTS = 3 * SLICE + 1001  # four slices of the split path, the last one ragged
COUNTERS = ("evals_sweep", "evals_binned", "evals_in_place")
KNOBS = ("BRICKS", "FORCE_GENERIC", "AXIS_REGS", "PPL", "POINTS_PATH", "POINTS_LOAD", "POINTS_SLICE", "SWEEP", "SWEEP_PERIOD",
         "SWEEP_PROBE", "BINNED", "COLUMN", "BIN_SLICE_LOG2", "LATTICE", "HOST_CHUNK", "DEAL")


@dataclasses.dataclass(frozen=True)
class Family:
    """One inner large-batch path: the grid, what forces the path, and the kernel it must end in."""
    name: str
    method: str
    kind: str
    axes: tuple
    inner: str               # "sweep" or "binned": the counter that must move, once per slice
    kernel: str              # the last slice's kernel
    options: tuple           # (name, value) pairs set on the handle
    bricks: str = None       # INTERPN_HIP_BRICKS at creation
    linearize: bool = False

    @property
    def n(self):
        return len(self.axes)


SWEEP = (("sweep", 1),)
SORTED = (("binned", 1), ("column", 0))
COLUMN = (("binned", 1), ("column", 1))
FAMILIES = [
    # grids of tests/test_gpu_parity.py's forced tests (test_sweep_evaluation, test_linear2_sweep_evaluation, ...)
    Family("linear3-reg", "linear", "regular", (20, 17, 33), "sweep", "interpn::k_linear_sweep<", SWEEP),
    Family("linear3-rect", "linear", "rectilinear", (24, 11, 40), "sweep", "interpn::k_linear_sweep<", SWEEP),
    Family("linear3-rect-lds", "linear", "rectilinear", (70, 33, 90), "sweep", "interpn::k_linear_sweep<", SWEEP),
    Family("linear2-reg", "linear", "regular", (70, 90), "sweep", "interpn::k_linear2_sweep<", SWEEP),
    Family("nearest2-reg", "nearest", "regular", (70, 90), "sweep", "interpn::k_nearest_sweep<", SWEEP),
    Family("nearest3-reg", "nearest", "regular", (20, 17, 33), "sweep", "interpn::k_nearest_sweep<", SWEEP),
    Family("cubic2-reg", "cubic", "regular", (150, 140), "sweep", "interpn::k_cubic_sweep<", SWEEP),
    Family("cubic2-reg-lin", "cubic", "regular", (150, 140), "sweep", "interpn::k_cubic_sweep<", SWEEP, linearize=True),
    Family("cubic2-rect", "cubic", "rectilinear", (130, 160), "sweep", "interpn::k_cubic_sweep<", SWEEP),
    Family("cubic3-reg", "cubic", "regular", (20, 17, 33), "sweep", "interpn::k_cubic_sweep<", SWEEP),
    Family("cubic3-reg-lin", "cubic", "regular", (20, 17, 33), "sweep", "interpn::k_cubic_sweep<", SWEEP, linearize=True),
    Family("cubic3-rect-lin", "cubic", "rectilinear", (24, 11, 40), "sweep", "interpn::k_cubic_sweep<", SWEEP, linearize=True),
    Family("sorted2-reg", "cubic", "regular", (9, 7), "binned", "interpn::k_cubic_brick<", SORTED, "11"),
    Family("sorted3-reg", "cubic", "regular", (6, 5, 7), "binned", "interpn::k_cubic_brick<", SORTED, "44", linearize=True),
    Family("sorted4-reg", "cubic", "regular", (5, 6, 4, 7), "binned", "interpn::k_cubic_brick<", SORTED, "11"),
    Family("sorted4-rect", "cubic", "rectilinear", (5, 6, 4, 7), "binned", "interpn::k_cubic_brick<", SORTED, "11", linearize=True),
    Family("column4-reg", "cubic", "regular", (6, 7, 5, 6), "binned", "interpn::k_cubic_column<", COLUMN, "11"),
    Family("column4-rect", "cubic", "rectilinear", (6, 7, 5, 6), "binned", "interpn::k_cubic_column<", COLUMN, "11", linearize=True),
    Family("column3-reg", "cubic", "regular", (6, 7, 5), "binned", "interpn::k_cubic3_column<", COLUMN, "11", linearize=True),
]
BY_NAME = {f.name: f for f in FAMILIES}
REGULAR = [f for f in FAMILIES if f.kind == "regular"]
# both element types under fma, and the other flavour once per family
VARIANTS = [(f, dt, fma) for f in FAMILIES for dt, fma in ((np.float64, True), (np.float32, True), (np.float64, False))]


def _vid(v):
    f, dt, fma = v
    return f"{f.name}-{'f64' if dt == np.float64 else 'f32'}-{'fma' if fma else 'nofma'}"


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


def _case(fam, dtype, nobs=NPTS, seed=0):
    # (the smallest tables carry no special rows, as in the forced tests they come from)
    return synthetic_case(fam.method, fam.kind, fam.n, list(fam.axes), nobs, 7100 + sum(fam.axes) + seed, dtype=dtype,
                          linearize=fam.linearize, extrap=0.3, specials=min(fam.axes) >= 8)


def _handle(fam, case, monkeypatch, fma=True):
    import interpn_amd

    if fam.bricks:
        monkeypatch.setenv("INTERPN_HIP_BRICKS", fam.bricks)
    dt = case.vals.dtype
    if case.kind == "regular":
        it = interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, case.vals,
                                              linearize_extrapolation=case.linearize, dtype=dt, fma=fma)
    else:
        it = interpn_amd.Interpolator.rectilinear(case.method, case.grids, case.vals, linearize_extrapolation=case.linearize,
                                                  dtype=dt, fma=fma)
    monkeypatch.delenv("INTERPN_HIP_BRICKS", raising=False)
    return it


def _force(it, fam, on=True):
    """The family's inner path, or (`on` false) the one-pass kernel whatever the batch."""
    for name, value in fam.options:
        it.set_option(name, value if on else 0)
    if not on:
        for name in ("sweep", "binned", "column"):
            it.set_option(name, 0)
    # The precondition of the forced sweep tests: the table the sweep kernel reads exists.  `sweep_table_bytes` is the 3-D
    # multilinear sweep's own table; the 2-D multilinear and the multicubic sweeps read the handle's one brick / tile table
    # (`table_layout`); the nearest-neighbour sweep reads the C-ordered grid and needs none.
    if fam.method == "linear" and fam.n == 3:
        assert it.get_option("sweep_table_bytes") > 0 and it.get_option("sweep_layout") in (11, 12)
    elif fam.inner == "sweep" and fam.method != "nearest":
        assert it.table_layout()[0] > 0, fam.name


def _split(it, slice_points=SLICE):
    it.set_option("points_path", 2)
    it.set_option("points_slice", slice_points)


def _counters(it):
    return {k: it.get_option(k) for k in COUNTERS}


def _moved(it, before):
    return {k: it.get_option(k) - before[k] for k in COUNTERS}


def _took(fam, slices):
    """What the counters must say after `slices` slices that all took the family's inner path."""
    return {"evals_sweep": slices if fam.inner == "sweep" else 0, "evals_binned": slices if fam.inner == "binned" else 0,
            "evals_in_place": 0}


IN_PLACE = lambda slices: {"evals_sweep": 0, "evals_binned": 0, "evals_in_place": slices}  # noqa: E731


def _assert_inner(it, fam, before, slices, what):
    assert _moved(it, before) == _took(fam, slices), (what, _moved(it, before))
    assert it.get_option("last_binned") == (1 if fam.inner == "binned" else 0), what
    assert it.kernel_name().startswith(fam.kernel), (what, it.kernel_name())
    assert it.last_points_path() == "split", what


def _rows(obs):
    return np.ascontiguousarray(np.stack(obs, axis=1))


def _tensors(arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _columns(it, fam, obs):
    """The second yardstick: the handle's one-pass kernels on the coordinate arrays."""
    _force(it, fam, on=False)
    before = _counters(it)
    out = it.eval_tensors(_tensors(obs))
    it.finish()
    assert _moved(it, before) == IN_PLACE(1)
    _force(it, fam)
    return out.cpu().numpy()


def _device(it, pts_t, out=None, **kw):
    out = it.eval_points_tensors(pts_t, out, **kw)
    it.finish()
    return out.cpu().numpy()


def _wide(pts, extra):
    """The rows as a view of a tensor whose rows are `extra` elements longer (a coordinate nobody may read behind them)."""
    import torch

    n, nd = pts.shape
    wide = torch.full((n, nd + extra), 1e30, dtype=torch.from_numpy(pts).dtype, device="cuda")
    wide[:, :nd] = torch.from_numpy(pts).cuda()
    return wide[:, :nd]


def _inject(case, where):
    """NaN / +inf / -inf at the given (dimension, index, value) triples."""
    for d, i, v in where:
        case.obs[d][i] = v


# ---- 1. points, split path x every inner family ------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_split_path_over_every_inner_family(oracle, monkeypatch, variant):
    """Four slices (the last ragged), packed rows and rows of a wider tensor, device and host form (chunks of 5000 points: the
    seams of chunks and slices do not coincide).  Rectilinear grids never fail per point: NaN, +inf and -inf in slices 0, 2
    and 3 propagate."""
    fam, dtype, fma = variant
    case = _case(fam, dtype)
    if fam.kind == "rectilinear":
        _inject(case, [(0, 1234, np.nan), (fam.n - 1, 2 * SLICE + 17, np.inf), (0, 3 * SLICE + 500, -np.inf), (fam.n - 1, NPTS - 1, np.nan)])
    want = run_oracle(oracle, case, fma=fma)
    it = _handle(fam, case, monkeypatch, fma)
    try:
        _force(it, fam)
        ref = _columns(it, fam, case.obs)
        _assert_same(ref, want, "the one-pass kernels against the oracle")
        _split(it)
        pts = _rows(case.obs)
        for extra in (0, 1):
            before = _counters(it)
            got = _device(it, _wide(pts, extra))
            _assert_inner(it, fam, before, 4, ("device", extra))
            _assert_same(got, want, ("device against the oracle", extra))
            _assert_same(got, ref, ("device against the one-pass kernels", extra))
        it.set_option("host_chunk", 5000)  # chunks of 5000, 5000 and 3289 points: 2 + 2 + 1 slices
        before = _counters(it)
        got = it.eval_points_host(pts)
        _assert_inner(it, fam, before, 5, "host")
        _assert_same(got, want, "host against the oracle")
    finally:
        it.close()


def test_inner_sub_slices_inside_one_outer_slice(oracle, monkeypatch):
    """Outer slices of 3 * 2^16 points over a sort that takes 2^16 points at a time: three inner sub-slices in the first outer
    slice, two (one ragged) in the second."""
    fam = BY_NAME["sorted4-reg"]
    npts = 3 * 65536 + 70_001
    case = _case(fam, np.float64, nobs=npts, seed=1)
    want = run_oracle(oracle, case)
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        it.set_option("bin_slice_log2", 16)
        ref = _columns(it, fam, case.obs)
        _split(it, 3 * 65536)
        before = _counters(it)
        got = _device(it, _wide(_rows(case.obs), 1))
        _assert_inner(it, fam, before, 2, "two outer slices")
        _assert_same(got, want, "against the oracle")
        _assert_same(got, ref, "against the one-pass kernels")
        # a failing point in the second sub-slice of the second outer slice: shifted twice
        first = 3 * 65536 + 65536 + 123
        bad = dataclasses.replace(case, obs=[o.copy() for o in case.obs])
        _inject(bad, [(2, first, np.nan), (0, npts - 1, np.inf)])
        res = it.eval_points_tensors(_tensors([_rows(bad.obs)])[0])
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
            it.finish()
        assert ei.value.first_bad_index == first
        _assert_same(res.cpu().numpy()[:first], want[:first], "prefix")
    finally:
        it.close()


# ---- 2. alignment -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_odd_element_out_makes_every_slice_fall_back(oracle, monkeypatch, dtype):
    """The sweep kernels take 16-byte aligned streams only.  The slices' coordinate arrays are aligned by construction; `out`
    is the caller's: one element off a 16-byte boundary, every slice runs the one-pass kernel, nothing around `out` is
    touched.  A points base one element off does not matter (the coordinate arrays are the scratch block's)."""
    import torch

    fam = BY_NAME["linear3-reg"]
    case = _case(fam, dtype, seed=2)
    want = run_oracle(oracle, case)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        _split(it)
        pts = _rows(case.obs)
        big = torch.zeros(NPTS * 3 + 3, dtype=tdt, device="cuda")
        big[1:1 + NPTS * 3] = torch.from_numpy(pts).cuda().reshape(-1)
        view = big[1:1 + NPTS * 3].view(NPTS, 3)
        assert view.data_ptr() % 16 == np.dtype(dtype).itemsize
        out_b = torch.full((NPTS + 2,), -7.0, dtype=tdt, device="cuda")
        out = out_b[1:NPTS + 1]
        assert out.data_ptr() % 16 == np.dtype(dtype).itemsize
        before = _counters(it)
        got = _device(it, view, out)
        assert _moved(it, before) == IN_PLACE(4), _moved(it, before)
        assert it.last_points_path() == "split" and not it.kernel_name().startswith(fam.kernel), it.kernel_name()
        _assert_same(got, want, "out + 1, base + 1")
        assert float(out_b[0]) == -7.0 and float(out_b[-1]) == -7.0
        # the same points, an aligned `out`: the sweep kernel again
        before = _counters(it)
        got = _device(it, view)
        _assert_inner(it, fam, before, 4, "base + 1")
        _assert_same(got, want, "base + 1")
    finally:
        it.close()


# ---- 3. failing points on regular grids ---------------------------------------------------------------------------------

def _failing(case, fam, where):
    """Plants the failures; returns the smallest failing index.  `mixed`: a NaN in slice 1, behind it in the same slice a
    point that fails too and sorts in front of it (the first cell of every other dimension against the last), an inf in
    slice 2 that sorts first as well, a NaN in the ragged slice."""
    last, lo, hi = fam.n - 1, [float(g[0]) for g in case.grids], [float(g[-1]) for g in case.grids]
    if where == "first":
        _inject(case, [(last, 0, np.nan)])
        return 0
    if where == "last":
        _inject(case, [(0, NPTS - 1, np.inf)])
        return NPTS - 1
    first = SLICE + 777
    for d in range(last):
        case.obs[d][first] = hi[d]
        case.obs[d][SLICE + 2000] = lo[d]
        case.obs[d][2 * SLICE + 5] = lo[d]
    _inject(case, [(last, first, np.nan), (last, SLICE + 2000, -np.inf), (last, 2 * SLICE + 5, np.inf), (0, 3 * SLICE + 500, np.nan)])
    return first


@pytest.mark.parametrize("where", ["mixed", "first", "last"])
@pytest.mark.parametrize("fam", REGULAR, ids=[f.name for f in REGULAR])
def test_first_failing_index_through_every_family(oracle, monkeypatch, fam, where):
    """The word is parked and shifted around every slice but the first, and the sorted paths meet the points out of index
    order: the smallest failing index of the whole call is reported, everything in front of it is written (the device form),
    and nothing from it on (the host form, chunks of 5000 points)."""
    clean = _case(fam, np.float64, seed=3)
    want = run_oracle(oracle, clean)
    case = dataclasses.replace(clean, obs=[o.copy() for o in clean.obs])
    first = _failing(case, fam, where)
    with pytest.raises(AssertionError) as oe:  # the oracle's own loop agrees on the index
        run_oracle(oracle, case)
    assert oe.value.first_bad == first
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        _split(it)
        pts = _rows(case.obs)
        before = _counters(it)
        got = it.eval_points_tensors(_wide(pts, 1))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
            it.finish()
        assert ei.value.first_bad_index == first, (ei.value.first_bad_index, first)
        _assert_inner(it, fam, before, 4, "device")
        _assert_same(got.cpu().numpy()[:first], want[:first], "device: the prefix")
        it.set_option("host_chunk", 5000)
        out = np.full(NPTS, -7.0)
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
            it.eval_points_host(pts, out)
        _assert_same(out[:first], want[:first], "host: the prefix")
        assert (out[first:] == -7.0).all(), "host: everything from the failing point on is left alone"
        # the status word was reset and the parked word did not leak: a clean batch through the same handle is clean
        before = _counters(it)
        _assert_same(_device(it, _wide(_rows(clean.obs), 0)), want, "clean again")
        _assert_inner(it, fam, before, 4, "clean again")
    finally:
        it.close()


# ---- 4. lattices, expanded path x inner families ------------------------------------------------------------------------

LATTICES = [("linear3-reg", [40, 30, 50]), ("linear3-rect", [40, 30, 50]), ("linear2-reg", [240, 250]), ("nearest3-reg", [40, 30, 50]),
            ("cubic2-reg-lin", [240, 250]), ("cubic3-reg", [40, 30, 50]), ("cubic3-rect-lin", [40, 30, 50]),
            ("sorted4-reg", [15, 16, 14, 17])]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,lens", LATTICES, ids=[n for n, _ in LATTICES])
def test_expanded_lattice_over_every_inner_family(oracle, monkeypatch, name, lens, dtype):
    """One slice of about 6e4 lattice points through the sweep kernel / the sorted evaluation; device and host form."""
    fam = BY_NAME[name]
    case = _case(fam, dtype, nobs=1, seed=4)
    axes = _axes(case, lens, seed=5)
    points = _expand(axes)
    want = run_oracle(oracle, dataclasses.replace(case, obs=points), out=np.zeros(points[0].size, dtype=dtype))
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        ref = _columns(it, fam, points)
        it.set_option("lattice", 0)
        before = _counters(it)
        got = it.eval_lattice_tensors(_tensors(axes))
        it.finish()
        assert _moved(it, before) == _took(fam, 1), _moved(it, before)
        assert it.last_lattice_path == "expanded" and it.kernel_name().startswith(fam.kernel), it.kernel_name()
        assert tuple(got.shape) == tuple(lens)
        _assert_same(got.cpu().numpy().ravel(), want, "device against the oracle")
        _assert_same(got.cpu().numpy().ravel(), ref, "device against the one-pass kernels")
        before = _counters(it)
        host = it.eval_lattice_host(axes)
        assert _moved(it, before) == _took(fam, 1), _moved(it, before)
        _assert_same(host.ravel(), want, "host against the oracle")
    finally:
        it.close()


@pytest.mark.parametrize("dtype,m", [(np.float64, 150), (np.float32, 180)], ids=["f64-150", "f32-180"])
def test_two_expanded_slices_through_the_sweep_kernel(oracle, monkeypatch, dtype, m):
    """The expanded slice is 64 MiB of coordinates: two slices.  A NaN in the last coordinate of the leading axis fails first
    at `last * m * m`, behind the first slice; the same lattice clean has the oracle's bits at every point."""
    fam = BY_NAME["linear3-reg"]
    lens = [m, m, m]
    assert m**3 > 64 * 2**20 // (3 * np.dtype(dtype).itemsize) > m**3 // 2
    case = _case(fam, dtype, nobs=1, seed=6)
    axes = _axes(case, lens, seed=7)
    points = _expand(axes)
    want = run_oracle(oracle, dataclasses.replace(case, obs=points), out=np.zeros(m**3, dtype=dtype))
    del points
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        it.set_option("lattice", 0)
        bad = [a.copy() for a in axes]
        bad[0][m - 1] = np.nan
        before = _counters(it)
        it.eval_lattice_tensors(_tensors(bad))
        with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as ei:
            it.finish()
        assert ei.value.first_bad_index == (m - 1) * m * m
        assert _moved(it, before) == _took(fam, 2), _moved(it, before)
        before = _counters(it)
        got = it.eval_lattice_tensors(_tensors(axes))
        it.finish()
        assert _moved(it, before) == _took(fam, 2), _moved(it, before)
        assert it.last_lattice_path == "expanded" and it.kernel_name().startswith(fam.kernel), it.kernel_name()
        _assert_same(got.cpu().numpy().ravel(), want, "two slices against the oracle")
    finally:
        it.close()


# ---- 5. field sets, per-field path x sweep ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["linear3-reg", "linear3-rect"])
def test_per_field_path_through_the_sweep_kernel(oracle, monkeypatch, name):
    """The K handles of a set latch their options at creation: INTERPN_HIP_SWEEP=1.  Every row has the oracle's bits; on the
    regular grid a NaN is reported with its index and every row's prefix is written (the contract of
    tests/test_fields_gpu.py::test_failing_point_contract).  The set's counters are those of its K handles, summed: with
    packed rows of an odd length every other row of `out` is not 16-byte aligned and that field alone runs in place."""
    import torch

    import interpn_amd

    fam = BY_NAME[name]
    npts, k = 40_007, 3
    case = _case(fam, np.float64, nobs=npts, seed=8)
    rng = np.random.default_rng(88)
    fields = np.stack([rng.uniform(-1.0, 1.0, case.vals.size) for _ in range(k)])

    def rows(obs):
        return np.stack([run_oracle(oracle, dataclasses.replace(case, vals=fields[f], obs=obs), out=np.zeros(obs[0].size)) for f in range(k)])

    want = rows(case.obs)
    monkeypatch.setenv("INTERPN_HIP_SWEEP", "1")
    if case.kind == "regular":
        fs = interpn_amd.Fields.regular("linear", case.dims, case.starts, case.steps, fields)
    else:
        fs = interpn_amd.Fields.rectilinear("linear", case.grids, fields)
    monkeypatch.delenv("INTERPN_HIP_SWEEP")
    try:
        assert fs.get_option("sweep") == 1
        fs.set_option("fused", 0)
        before = {c: fs.get_option(c) for c in COUNTERS}  # (a set reports these summed over its K handles)
        got = fs.eval_tensors(_tensors(case.obs))
        fs.finish()
        assert fs.get_option("sweep_table_bytes") > 0  # (a set with a fused table builds its handles' own at their first use)
        assert fs.last_path == "per_field" and fs.kernel_name().startswith(fam.kernel), fs.kernel_name()
        # packed rows of 40 007 f64 elements: row 1 begins 8 bytes off a 16-byte boundary and is left to the one-pass kernel
        assert {c: fs.get_option(c) - before[c] for c in COUNTERS} == {"evals_sweep": 2, "evals_binned": 0, "evals_in_place": 1}
        _assert_same(got.cpu().numpy(), want, "device rows")
        # rows of a wider tensor, every one 16-byte aligned: every field sweeps
        wide = torch.full((k, npts + 1), -7.0, dtype=torch.float64, device="cuda")
        before = {c: fs.get_option(c) for c in COUNTERS}
        fs.eval_tensors(_tensors(case.obs), wide[:, :npts])
        fs.finish()
        assert {c: fs.get_option(c) - before[c] for c in COUNTERS} == _took(fam, k)
        _assert_same(wide[:, :npts].cpu().numpy(), want, "device rows, aligned")
        assert bool((wide[:, npts] == -7.0).all())
        _assert_same(fs.eval_host(case.obs), want, "host rows")
        if case.kind == "regular":
            bad = 23_456
            obs = [o.copy() for o in case.obs]
            obs[1][bad] = np.nan
            obs[2][bad + 700] = np.inf  # a later failure must not be the one reported
            for chunk in (0, 10_000):
                fs.set_option("host_chunk", chunk)
                out = np.full((k, npts), 777.25)
                with pytest.raises(AssertionError, match="Unrepresentable coordinate value"):
                    fs.eval_host(obs, out)
                _assert_same(out[:, :bad], want[:, :bad], ("host head", chunk))
                assert np.all(out[:, bad:] == 777.25), chunk
            before = {c: fs.get_option(c) for c in COUNTERS}
            res = fs.eval_tensors(_tensors(obs), wide[:, :npts])
            with pytest.raises(AssertionError, match="Unrepresentable coordinate value") as err:
                fs.finish()
            assert err.value.first_bad_index == bad
            assert {c: fs.get_option(c) - before[c] for c in COUNTERS} == _took(fam, k)
            _assert_same(res[:, :bad].cpu().numpy(), want[:, :bad], "device head")
            # the status words are cleared: a clean batch afterwards is clean
            _assert_same(fs.eval_tensors(_tensors(case.obs)).cpu().numpy(), want, "clean again")
            fs.finish()
    finally:
        fs.close()


# ---- 6. reserved scratch, NO_ALLOC, capture, mixed reuse ----------------------------------------------------------------

def test_no_alloc_needs_a_block_for_each_level(oracle, monkeypatch):
    """`reserve_points` sizes the block of the slices; `reserve` counts ANY block that is large enough, so after both with one
    stream the handle owns ONE block.  The split path takes it, the inner call finds none and may make none: every slice runs
    the one-pass kernel, quietly and with the right bits.  With a second block (`reserve(npoints, 2)`, as
    include/interpn_hip.h says) the inner sweep runs, and nothing is allocated either way."""
    import interpn_amd

    fam = BY_NAME["linear3-reg"]
    case = _case(fam, np.float64, seed=9)
    want = run_oracle(oracle, case)
    pts_t = _tensors([_rows(case.obs)])[0]
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        _split(it)
        with pytest.raises(interpn_amd._lib.InterpnHipError):  # nothing reserved: an error, not a silent allocation
            it.eval_points_tensors(pts_t, no_alloc=True)
        it.reserve_points(NPTS, 1)
        it.reserve(NPTS, 1)
        allocs = it.get_option("scratch_allocs")
        assert allocs == 1
        before = _counters(it)
        got = _device(it, pts_t, no_alloc=True)
        moved = _moved(it, before)
        _assert_same(got, want, ("one block, no_alloc; the slices ran", moved))
        assert it.get_option("scratch_allocs") == allocs, moved
        assert moved == IN_PLACE(4), ("one block serves the slices only: the inner call has none", moved)
        it.reserve(NPTS, 2)
        allocs = it.get_option("scratch_allocs")
        assert allocs == 2
        before = _counters(it)
        got = _device(it, pts_t, no_alloc=True)
        _assert_inner(it, fam, before, 4, "two blocks, no_alloc")
        assert it.get_option("scratch_allocs") == allocs
        _assert_same(got, want, "two blocks, no_alloc")
    finally:
        it.close()


def test_capture_of_the_split_path_runs_one_kernel_per_slice(oracle, monkeypatch):
    """Under capture the split path takes a block the handle already owns, and the inner call falls back to the one-pass
    kernel (the sweep's block event cannot be recorded there): a single chain of kernels, replayed on fresh points."""
    import torch

    fam = BY_NAME["linear3-reg"]
    case = _case(fam, np.float64, seed=10)
    fresh = dataclasses.replace(case, obs=_case(fam, np.float64, seed=11).obs)  # the same grid, other points
    want = run_oracle(oracle, fresh)
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        _split(it)
        pts_t = _tensors([_rows(case.obs)])[0]
        out = torch.zeros(NPTS, dtype=torch.float64, device="cuda")
        before = _counters(it)
        it.eval_points_tensors(pts_t, out)  # warm: nothing is left to allocate or build
        it.finish()
        _assert_inner(it, fam, before, 4, "warm")
        _assert_same(out.cpu().numpy(), run_oracle(oracle, case), "warm")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        before = _counters(it)
        with torch.cuda.graph(graph, stream=side):
            it.eval_points_tensors(pts_t, out)
        assert _moved(it, before) == IN_PLACE(4), _moved(it, before)
        pts_t.copy_(torch.from_numpy(_rows(fresh.obs)))
        out.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        it.finish()
        _assert_same(out.cpu().numpy(), want, "replay")
    finally:
        it.close()


def _plain_block_bytes(fam, case, monkeypatch, count):
    """Bytes of the scratch block a plain forced evaluation of `count` points takes, measured on a fresh handle."""
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        it.eval_tensors([t[:count].clone() for t in _tensors(case.obs)])
        it.finish()
        assert it.get_option("scratch_allocs") == 1
        return it.get_option("scratch_bytes")
    finally:
        it.close()


@pytest.mark.parametrize("name,plain_points,reuses", [("sorted4-reg", 1500, True), ("sorted4-reg", NPTS, False), ("linear3-reg", NPTS, True)],
                         ids=["sorted-1500", "sorted-all", "sweep"])
def test_blocks_change_hands_between_the_slices_and_the_inner_paths(oracle, monkeypatch, name, plain_points, reuses):
    """A split-path call, a plain sorted / sweep evaluation, the split path again (three times over), all on one handle and
    stream.  The slices' block is the handle's first, and a plain evaluation takes the first block that is large enough: the
    sweep's 1.25 KiB of work words and the sort of 1500 points fit the slices' block (asserted below from the blocks' measured
    sizes), so they run in a block whose bin counters / work words are coordinates by then and must be reset (`claim_slot`),
    and the slices take it back afterwards: two blocks throughout.  The sort of all the points fits neither block and makes
    a third."""
    fam = BY_NAME[name]
    case = _case(fam, np.float64, seed=12)
    want = run_oracle(oracle, case)
    need = _plain_block_bytes(fam, case, monkeypatch, plain_points)
    inner = _plain_block_bytes(fam, case, monkeypatch, SLICE)  # what the first slice's inner call takes
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        _split(it)
        pts_t = _tensors([_rows(case.obs)])[0]
        obs_t = [t[:plain_points].clone() for t in _tensors(case.obs)]
        for rep in range(3):
            before = _counters(it)
            _assert_same(_device(it, pts_t), want, ("split", rep))
            _assert_inner(it, fam, before, 4, ("split", rep))
            if rep == 0:
                assert it.get_option("scratch_allocs") == 2
                slices = it.get_option("scratch_bytes") - inner  # the slices' block, made first
                assert (need <= slices) == reuses, (need, slices, inner)
            before = _counters(it)
            plain = it.eval_tensors(obs_t)
            it.finish()
            assert it.last_path == fam.inner and _moved(it, before) == _took(fam, 1), (rep, it.last_path, _moved(it, before))
            _assert_same(plain.cpu().numpy(), want[:plain_points], ("plain", rep))
        assert it.get_option("scratch_allocs") == (2 if reuses else 3)
    finally:
        it.close()


# ---- 7. two streams, one handle -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["linear3-reg", "column4-reg"])
def test_two_streams_share_the_blocks_of_both_levels(oracle, monkeypatch, name):
    """Four repetitions on each of two streams: every call holds a block for its slices and takes another for the sweep's work
    words / the sort, out of the handle's four, waiting on the device for whoever used it last."""
    import torch

    fam = BY_NAME[name]
    case = _case(fam, np.float64, seed=13)
    want = run_oracle(oracle, case)
    it = _handle(fam, case, monkeypatch)
    try:
        _force(it, fam)
        _split(it)
        pts_t = _tensors([_rows(case.obs)])[0]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        before = _counters(it)
        outs = []
        for rep in range(4):
            for s in (s1, s2):
                with torch.cuda.stream(s):
                    outs.append(it.eval_points_tensors(pts_t))
        torch.cuda.synchronize()
        it.finish()
        assert _moved(it, before) == _took(fam, 32), _moved(it, before)
        for i, o in enumerate(outs):
            _assert_same(o.cpu().numpy(), want, ("call", i))
    finally:
        it.close()
