"""The value families of tests/test_anisotropic_gpu.py, each as a function of (case, want, ...) that forces the family onto
its path (layout, options, environment), asserts the kernel or path that ran and compares every result with `want`.
tests/test_anisotropic_gpu.py runs them on clean tables, tests/test_table_nonfinite_gpu.py on tables with non-finite nodes:
one forcing, so that neither file can drift onto another kernel.

`want` is what `assert_same` compares with: an array (bit for bit; a NaN need only be a NaN on both sides), or an
`Expect`, which carries the three expectations of a table with non-finite nodes.  A family that needs `want` in another
arrangement (point-major, fields last, one field of a set) takes it through `arranged`."""

import dataclasses

import numpy as np

from tests.helpers import anisotropic_case, anisotropic_points, footprint_poisoned, poison_table, run_oracle

S2, S3, S4 = [9, 7], [6, 5, 7], [5, 6, 4, 5]  # the shapes of tests/test_anisotropic_cpu.py
S5, S6 = [4, 3, 5, 3, 4], [3, 4, 2, 5, 3, 4]
LONG3, LONG2 = [70, 9, 7], [9, 130]           # one axis longer than a wave (rectilinear: searched in LDS, not across lanes)
NPTS = 2001
KNOBS = ("BRICKS", "FORCE_GENERIC", "GENERIC_RUNTIME", "GENERIC_VEC", "AXIS_REGS", "PPL", "POINTS_PATH", "POINTS_LOAD", "POINTS_STORE",
         "POINTS_SLICE", "SWEEP", "SWEEP_PERIOD", "BINNED", "COLUMN", "LATTICE", "FIELDS_FUSED", "HOST_CHUNK", "DEAL")


@dataclasses.dataclass
class Expect:
    """What a result on a table with non-finite nodes must be.  `oracle`: the oracle on that table.  `touched`: per
    point, whether its footprint holds a non-finite node (tests/helpers.py::footprint_poisoned; None for nearest, which
    has oracle parity only).  `clean`: the oracle on the table before it was poisoned."""
    oracle: np.ndarray
    touched: np.ndarray
    clean: np.ndarray


def arranged(want, fn):
    """`want` (an array or an Expect) with `fn` applied to each of its arrays."""
    if not isinstance(want, Expect):
        return fn(want)
    return Expect(fn(want.oracle), None if want.touched is None else fn(want.touched), fn(want.clean))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def assert_same(got, want, what=""):
    """Bit for bit, a NaN need only be a NaN on both sides (the sign of an infinity counts).  With an Expect also: the
    result is non-finite exactly at the touched points, and at every other point it has the clean table's bits."""
    if isinstance(want, Expect):
        assert_same(got, want.oracle, (what, "oracle on the same table"))
        if want.touched is not None:
            got = np.asarray(got)
            assert want.touched.shape == got.shape, (what, want.touched.shape, got.shape)
            wrong = ~np.isfinite(got) != want.touched
            assert not wrong.any(), (what, "non-finite off the footprint rule", int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
            keep = ~want.touched
            differ = keep & (bits(got) != bits(want.clean))
            assert not differ.any(), (what, "clean-table bits lost", int(differ.sum()), np.argwhere(differ)[:4].tolist())
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist(), got[~same][:4], want[~same][:4])


def make_case(method, kind, shape, dtype, nobs=NPTS, linearize=False, seed=0):
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


def make_handle(case, fma, monkeypatch=None, bricks=None):
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


def fields_handle(case, fields, fma):
    import interpn_amd

    if case.kind == "regular":
        return interpn_amd.Fields.regular(case.method, case.dims, case.starts, case.steps, fields,
                                          linearize_extrapolation=case.linearize, dtype=fields.dtype, fma=fma)
    return interpn_amd.Fields.rectilinear(case.method, case.grids, fields, linearize_extrapolation=case.linearize,
                                          dtype=fields.dtype, fma=fma)


def random_fields(case, k, seed):
    rng = np.random.default_rng(1000 + seed)
    return np.stack([rng.uniform(-1.0, 1.0, case.vals.size).astype(case.vals.dtype) for _ in range(k)])


def fields_want(oracle, case, fields, fma, obs=None):
    """(K, n): the oracle on every field alone."""
    obs = case.obs if obs is None else obs
    return np.stack([run_oracle(oracle, dataclasses.replace(case, vals=f, obs=obs), fma=fma, out=np.zeros(obs[0].size, dtype=f.dtype))
                     for f in fields])


def tensors(arrs):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrs]


def rows(obs):
    return np.ascontiguousarray(np.stack(obs, axis=1))


def eval_device(it, obs):
    out = it.eval_tensors(tensors(obs))
    it.finish()
    return out.cpu().numpy()


def linear_bricks(n):
    return "on" if n == 2 else "11"  # the layouts the multilinear handles build regardless of the grid's size


def lattice_axes(case, lens, seed):
    """One coordinate vector per axis, by the generator's point rule."""
    rng = np.random.default_rng(seed)
    return [anisotropic_points(g, m, rng, case.vals.dtype.type) for g, m in zip(case.grids, lens)]


def expand(axes):
    return [np.ascontiguousarray(m.ravel()) for m in np.meshgrid(*axes, indexing="ij")]


def transposed(a):
    return np.ascontiguousarray(a.T)


# ---- 1. multilinear N = 2..6: the C-order kernels and the brick kernels -----------------------------------------------------------------
def multilinear_c_order_and_bricks(case, want, fma, monkeypatch, kind, layout):
    n = len(case.dims)
    dtype = case.vals.dtype.type
    it = make_handle(case, fma, monkeypatch, {"off": "off", "bricks": linear_bricks(n), "c4": "c4"}[layout])
    try:
        assert (it.table_layout()[0] > 0) == (layout != "off")
        got = eval_device(it, case.obs)
        name = it.kernel_name()
        assert it.last_path == "in_place"
        if layout == "off":
            assert name.startswith(f"interpn::k_linear_{kind}<"), name
        else:
            assert name.startswith("interpn::k_linear2_brick<" if n == 2 else "interpn::k_linear_brick<"), name
        assert_same(got, want, name)
        assert_same(it.eval_host(case.obs, np.zeros(NPTS, dtype=dtype)), want, "host")
    finally:
        it.close()


# ---- 2. multicubic N = 2..4: the C-order kernels and the tiled kernel -----------------------------------------------------------------------
def multicubic_c_order_and_tiles(case, want, fma, monkeypatch, kind, layout):
    it = make_handle(case, fma, monkeypatch, layout)
    try:
        got = eval_device(it, case.obs)
        name = it.kernel_name()
        assert it.last_path == "in_place"
        if layout == "off":
            assert it.table_layout()[0] == 0 and name.startswith(f"interpn::k_cubic_{kind}<"), name
        else:
            assert it.table_layout()[1:] == (int(layout[0]), int(layout[1])) and name.startswith("interpn::k_cubic_brick<"), name
        assert_same(got, want, name)
    finally:
        it.close()


# ---- 3. sorted and column multicubic ----------------------------------------------------------------------------------------------------------
SORTED = [("sorted", S2, "11", "interpn::k_cubic_brick<"), ("sorted", S3, "44", "interpn::k_cubic_brick<"),
          ("sorted", S4, "11", "interpn::k_cubic_brick<"), ("column", S4, "11", "interpn::k_cubic_column<"),
          ("column", S3, "11", "interpn::k_cubic3_column<")]
SORTED_NOBS = 5000  # more than one chunk of the sort (4096)


def sorted_handle(case, fma, monkeypatch, form, layout, options=None):
    """A handle forced onto the sorted path (`binned`), its column form or the tiled kernel; then `options`, in order."""
    it = make_handle(case, fma, monkeypatch, layout)
    try:
        it.set_option("binned", 1)
        it.set_option("column", 1 if form == "column" else 0)
        for k, v in (options or {}).items():
            it.set_option(k, v)
    except BaseException:
        it.close()
        raise
    return it


def assert_sorted(it, kernel):
    """The evaluation just made sorted its points and ran `kernel` on them."""
    assert it.last_path == "binned" and it.get_option("last_binned") == 1, (it.last_path, it.last_path_reason)
    assert it.kernel_name().startswith(kernel), it.kernel_name()


def sorted_and_column_multicubic(case, want, fma, monkeypatch, form, layout, kernel, options=None, run=None):
    """`options`: a mapping of further handle options, set after `binned` / `column`.  `run(it, obs, want, kernel, what)`: makes
    and checks each evaluation instead of the comparison with `want` alone (tests/test_unevenly_filled_bins_gpu.py)."""
    it = sorted_handle(case, fma, monkeypatch, form, layout, options)
    try:
        for deal in (1, 0):
            it.set_option("deal", deal)
            if run is not None:
                run(it, case.obs, want, kernel, (form, deal))
                continue
            got = eval_device(it, case.obs)
            assert_sorted(it, kernel)
            assert_same(got, want, (form, deal))
    finally:
        it.close()


# ---- 3b. the same path on skewed batches (tests/test_skewed_batches_cpu.py, tests/test_unevenly_filled_bins_gpu.py) ----------------------
# The smallest grids at which the code in question exists.  [40, 37, 5, 4]: 37 x 34 = 1258 footprint cells for 1024 bins (key
# shifts); [6, 7, 5, 6]: 30 class-pair bins; [41, 40, 5, 6]: 1560 (more than one per thread; the direct records scatter whatever
# `scatter_staged` says); [20, 17, 33]: 304.
SKEWED_FORMS = [("sorted", S2, "11", "interpn::k_cubic_brick<"), ("sorted", S3, "44", "interpn::k_cubic_brick<"),
                ("sorted", S4, "11", "interpn::k_cubic_brick<"), ("sorted", [40, 37, 5, 4], "11", "interpn::k_cubic_brick<"),
                ("column", [6, 7, 5, 6], "11", "interpn::k_cubic_column<"), ("column", [41, 40, 5, 6], "11", "interpn::k_cubic_column<"),
                ("column", S3, "11", "interpn::k_cubic3_column<"), ("column", [20, 17, 33], "11", "interpn::k_cubic3_column<")]
SKEWED_IDS = [f"{f}-{'x'.join(map(str, s))}" for f, s, _, _ in SKEWED_FORMS]
SKEWED_SHAPES = [S2, S3, S4, [40, 37, 5, 4], [6, 7, 5, 6], [41, 40, 5, 6], [20, 17, 33]]
COLUMN3_PART = 16 * 256  # points per part of the 3-D column kernel (k_cubic3_column.hip)


def skewed_case(kind, shape, dtype, linearize=False):
    """The anisotropic multicubic case on `shape` whose grids and table the skewed batches are evaluated on (its own points
    are not used)."""
    return make_case("cubic", kind, shape, dtype, nobs=16, linearize=linearize)


def skewed_rng(shape, *salt):
    return np.random.default_rng([7300, *shape, *salt])


def swept_pairs(shape):
    """The class pairs a `one_pair` batch is run on: all of them where there are at most 42, else 24 — the four corners, the
    four edge midpoints and 16 by a seeded choice among the rest.  The bin's number on the device is key * mult % nbins, which
    is not visible from here: running over pairs is what reaches the first and the last bins (the tail rule) anyway."""
    m0, m1 = shape[0] - 1, shape[1] - 1
    every = [(c0, c1) for c0 in range(m0) for c1 in range(m1)]
    if len(every) <= 42:
        return every
    fixed = [(0, 0), (0, m1 - 1), (m0 - 1, 0), (m0 - 1, m1 - 1), (0, m1 // 2), (m0 - 1, m1 // 2), (m0 // 2, 0), (m0 // 2, m1 - 1)]
    rest = [p for p in every if p not in fixed]
    pick = np.random.default_rng([7301, *shape]).choice(len(rest), 16, replace=False)
    return fixed + [rest[int(k)] for k in sorted(pick)]


def heavy_pairs(shape):
    """Low corner, high corner and one interior pair."""
    m0, m1 = shape[0] - 1, shape[1] - 1
    return [(0, 0), (m0 - 1, m1 - 1), (m0 // 2, m1 // 2)]


def with_obs(case, obs):
    return dataclasses.replace(case, obs=obs)


# ---- 4. the sweep family: their grids, 3001 points = several ragged rounds --------------------------------------------------------------
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
SWEEP_IDS = [f"{m}{len(s)}-{k}-{'x'.join(map(str, s))}" + "".join(f"-{a}{b}" for a, b in o.items()) for m, k, s, o, _ in SWEEPS]
SWEEP_NOBS = 3001


def sweep_family(case, want, fma, monkeypatch, kind, options, kernel):
    """`kind` as in SWEEPS ("jittered" cases are rectilinear ones)."""
    method, shape, dtype = case.method, case.dims, case.vals.dtype
    it = make_handle(case, fma, monkeypatch)
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
            got = eval_device(it, case.obs)
            assert it.last_path == "sweep", (it.last_path, it.last_path_reason)
            name = it.kernel_name()
            assert name.startswith(kernel.format(t="double" if dtype == np.float64 else "float")), name
            if method == "cubic":
                assert name.endswith(", 2>") == (len(shape) == 2), name  # the 2-D form carries its N last
            assert_same(got, want, (name, period, case.linearize))
        assert it.get_option("evals_sweep") == 2
    finally:
        it.close()


# ---- 5. rectilinear search forms ------------------------------------------------------------------------------------------------------------
AXIS_SEARCH = [("linear", S2), ("linear", [64, 7]), ("linear", S3), ("linear", S4), ("linear", S6), ("linear", LONG3),
               ("nearest", [64]), ("nearest", S2), ("nearest", S3), ("nearest", S6), ("nearest", LONG2)]
BUCKETS = [("linear", [65, 130]), ("linear", [70, 9, 81]), ("linear", [7, 90, 5, 6]), ("linear", [128, 120, 100]), ("nearest", [80, 70, 90])]


def lane_resident_axis_search(case, want, fma, monkeypatch, axis_regs):
    """INTERPN_HIP_AXIS_REGS = 0 (LDS), 1 (probe sequence across lanes), 2 (lane tables), as
    test_lane_resident_axes_everywhere sets it: the brick kernels and the nearest kernel; a 70-point axis keeps the LDS search."""
    monkeypatch.setenv("INTERPN_HIP_AXIS_REGS", axis_regs)
    method, shape = case.method, case.dims
    n = len(shape)
    it = make_handle(case, fma, monkeypatch, linear_bricks(n) if method == "linear" else None)
    try:
        got = eval_device(it, case.obs)
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
        assert_same(got, want, name)
    finally:
        it.close()


def bucket_records_and_lds_search(case, want, fma, monkeypatch, spacing):
    """Axes longer than a wave (test_rectilinear_bucket_records).  "jittered": near-uniform axes with the table's origins and
    steps, on which the per-bucket records are built (axis_rec_mode 1 = full, 2 = compact) — searched through them, without
    them (option axis_records = 0: coordinates + tables) and with the LDS search forced (axis_regs = 0).  "rectilinear": the
    generator's growing / shrinking / clustered axes hold several nodes in one bucket, so no records exist (mode 0, as on the
    clustered axis of the existing test) and the same three settings search coordinates + tables; nearest never has any."""
    method, n = case.method, len(case.dims)
    obs = tensors(case.obs)
    for records, axis_regs in ((1, -1), (0, -1), (1, 0)):
        it = make_handle(case, fma, monkeypatch)
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
            assert_same(got, want, (name, mode, records, axis_regs))
        finally:
            it.close()


def linear_1d_records(g, vals, x, want, fma, monkeypatch):
    """1-D multilinear from one record per search bucket (test_linear_1d_rectilinear_records: INTERPN_HIP_BRICKS=on)."""
    import interpn_amd

    dtype = vals.dtype.type
    monkeypatch.setenv("INTERPN_HIP_BRICKS", "on")
    it = interpn_amd.Interpolator.rectilinear("linear", [g], vals, dtype=dtype, fma=fma)
    try:
        got = it.eval_host([x], np.zeros(x.size, dtype=dtype))
        name = it.kernel_name()
        assert name.startswith("interpn::k_linear1_records<"), name
        assert_same(got, want, name)
        assert_same(eval_device(it, [x]), want, "device")
    finally:
        it.close()


# ---- 6. the recursive arm: both forms of k_generic_n and the runtime-N kernel ----------------------------------------------------------
RECURSIVE = [("linear", [3, 2, 3, 2, 3, 2, 3]), ("cubic", [4, 5, 4, 5, 4])]


def recursive_arm_env(monkeypatch, form):
    if form == "runtime":
        monkeypatch.setenv("INTERPN_HIP_GENERIC_RUNTIME", "1")
    else:
        monkeypatch.setenv("INTERPN_HIP_GENERIC_VEC", "1" if form == "rowvec" else "0")


def recursive_arm(case, want, fma, monkeypatch, form):
    """After `recursive_arm_env(monkeypatch, form)`."""
    it = make_handle(case, fma, monkeypatch)
    try:
        got = eval_device(it, case.obs)
        name = it.kernel_name()
        assert it.last_path == "in_place"
        if form == "runtime":
            assert name.startswith("interpn::k_generic<"), name
        else:
            assert name.startswith("interpn::k_generic_n<") and name.endswith(", true>") == (form == "rowvec"), name
        assert_same(got, want, (name, case.linearize))
    finally:
        it.close()


# ---- 8. point-major points: eval_points, fused and split ---------------------------------------------------------------------------------
POINTS = [("linear", S2, "on"), ("linear", S3, "11"), ("linear", LONG3, "11"), ("linear", S4, None), ("cubic", S2, "11"),
          ("cubic", S3, "44"), ("cubic", S4, None), ("nearest", S3, None)]


def point_major_values(case, want, fma, monkeypatch, bricks):
    import torch

    method, n = case.method, len(case.dims)
    pts = rows(case.obs)
    has_fused = method == "linear" and n in (2, 3)
    it = make_handle(case, fma, monkeypatch, bricks)
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
            assert_same(got.cpu().numpy(), want, (name, path))
            assert_same(it.eval_points_host(pts), want, ("host", path))
    finally:
        it.close()


# ---- 9. field sets: Fields.eval and Fields.eval_points, fused and per-field / split ------------------------------------------------------
FIELD_SHAPES = [("linear", S2), ("linear", S3), ("linear", LONG3), ("linear", LONG2), ("cubic", S3), ("nearest", S2), ("linear", S4)]


def field_sets(case, fields, want, fma, kind):
    """`want`: (K, n), the expectation of every field alone."""
    method, n, dtype = case.method, len(case.dims), fields.dtype
    has_fused = method == "linear" and n in (2, 3)
    tname = "double" if dtype == np.float64 else "float"
    flags = f"{tname}, {n}, {'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}>"
    fs = fields_handle(case, fields, fma)
    try:
        assert (fs.get_option("fused_table_bytes") > 0) == has_fused
        for fused in ((1, 0) if has_fused else (0,)):
            fs.set_option("fused", fused)
            dev = fs.eval_tensors(tensors(case.obs))
            fs.finish()
            assert fs.last_path == ("fused" if fused else "per_field")
            name = fs.kernel_name()
            assert (name == "interpn::k_linear_fields<" + flags) if fused else not name.startswith("interpn::k_linear_fields"), name
            assert_same(dev.cpu().numpy(), want, (name, "device"))
            assert_same(fs.eval_host(case.obs), want, (name, "host"))
        # point-major: (n, N) in, (n, K) out
        fs.set_option("fused", -1)
        pts = rows(case.obs)
        for path in ((1, 2) if has_fused else (2,)):
            fs.set_option("points_path", path)
            fs.set_option("points_slice", 512)
            got = fs.eval_points_tensors(tensors([pts])[0])
            fs.finish()
            assert fs.last_points_path == ("fused" if path == 1 else "split")
            name = fs.kernel_name()
            assert (name == "interpn::k_linear_fields_points<" + flags) if path == 1 else not name.startswith("interpn::k_linear_fields_points"), name
            assert_same(got.cpu().numpy(), arranged(want, transposed), (name, "points device"))
            assert_same(fs.eval_points_host(pts), arranged(want, transposed), (name, "points host"))
    finally:
        fs.close()


# ---- 10. lattices: eval_lattice (fused / expanded) and Fields.eval_lattice (fused / per-field, field-major and fields-last) ---------
LATTICES = [("linear", S2, [7, 65], False), ("linear", S3, [2, 7, 63], False), ("linear", LONG3, [7, 2, 64], False),
            ("cubic", S2, [7, 1000], False), ("cubic", S2, [7, 65], True), ("cubic", S3, [7, 1, 65], True),
            ("cubic", LONG3, [7, 7, 63], False), ("cubic", S4, [2, 3, 7, 63], True), ("linear", S4, [3, 2, 7, 65], False),
            ("nearest", S3, [7, 2, 65], False)]
LATTICE_IDS = [f"{m}-{'x'.join(map(str, s))}-{'lin' if lin else 'quad'}-{l[-1]}" for m, s, l, lin in LATTICES]


def lattice_kernel(prefix, dtype, method, n, kind, fma, tail=""):
    return (f"{prefix}{'double' if dtype == np.float64 else 'float'}, {0 if method == 'linear' else 1}, {n}, "
            f"{'true' if kind == 'rectilinear' else 'false'}, {'true' if fma else 'false'}{tail}>")


def lattices(case, axes, fields, want, fma, kind, own=0):
    """`fields`: (K, size), of which field `own` is the single handle's table (`case.vals`); `want`: (K, *lens)."""
    method, n, dtype = case.method, len(case.dims), case.vals.dtype
    has_fused = method != "nearest" and n in (2, 3)
    assert np.array_equal(bits(case.vals), bits(fields[own]))
    first = arranged(want, lambda a: a[own])
    it = make_handle(case, fma)
    try:
        for mode in ((1, 0) if has_fused else (0,)):
            it.set_option("lattice", mode)
            dev = it.eval_lattice_tensors(tensors(axes))
            it.finish()
            assert it.last_lattice_path == ("fused" if mode else "expanded")
            name = it.kernel_name()
            if mode:
                assert name == lattice_kernel("interpn::k_lattice_rows<", dtype, method, n, kind, fma), name
            else:
                assert not name.startswith("interpn::k_lattice"), name
            assert_same(dev.cpu().numpy(), first, (name, "device"))
            assert_same(it.eval_lattice_host(axes), first, (name, "host"))
    finally:
        it.close()
    fs = fields_handle(case, fields, fma)
    try:
        for mode in ((1, 0) if has_fused else (0,)):
            fs.set_option("lattice", mode)
            for field_axis in (0, -1):
                dev = fs.eval_lattice_tensors(tensors(axes), field_axis=field_axis)
                fs.finish()
                assert fs.last_lattice_path == ("fused" if mode else "per_field")
                name = fs.kernel_name()
                if mode:
                    assert name == lattice_kernel("interpn::k_lattice_fields_rows<", dtype, method, n, kind, fma,
                                                  ", true" if field_axis else ", false"), name
                else:
                    assert not name.startswith("interpn::k_lattice_fields"), name
                w = want if field_axis == 0 else arranged(want, lambda a: np.ascontiguousarray(np.moveaxis(a, 0, -1)))
                assert_same(dev.cpu().numpy(), w, (name, field_axis, "device"))
                assert_same(fs.eval_lattice_host(axes, field_axis=field_axis), w, (name, field_axis, "host"))
    finally:
        fs.close()


# ---- tables with non-finite nodes (tests/test_table_nonfinite_cpu.py, tests/test_table_nonfinite_gpu.py) -----------------------------
POISON_SEED = 9020


def poisoned_case(case, kind, seed=0):
    """`case` with `poison_table` applied to its table (kind "nan", "mixed" or "plane"); grids and points are shared.
    The small tables of many dimensions get one or two poisoned nodes only (`poison_count`: 1 on 4x5x4x5x4 multicubic, 5 on
    2x3x2x3x2x3x2 multilinear), and with those on the rim too few points reach them: the base of the placement seeds is one
    at which every case of tests/test_table_nonfinite_cpu.py has a non-finite share well inside the [0.25, 0.75] asked of
    the inputs there (0.34 - 0.64)."""
    return dataclasses.replace(case, vals=poison_table(case.vals, case.dims, case.method, POISON_SEED + seed, kind))


def expect(oracle, case, clean, fma):
    """The Expect of `case` (a `poisoned_case` of `clean`) under the oracle's flavour `fma`."""
    touched = None if case.method == "nearest" else footprint_poisoned(case)
    return Expect(run_oracle(oracle, case, fma), touched, run_oracle(oracle, clean, fma))


def stacked(expects):
    """One Expect of (K, ...) from K of (...): a field set's."""
    touched = None if expects[0].touched is None else np.stack([e.touched for e in expects])
    return Expect(np.stack([e.oracle for e in expects]), touched, np.stack([e.clean for e in expects]))


def plane_cases():
    """(family, row, method, kind, shape, nobs, linearize) of every run on a "plane" table: the brick layouts of family 1
    and the cubic families 2 - 4, on their own shapes and point counts; `row` is the family's parameter row."""
    for kind in ("regular", "rectilinear"):
        for shape in (S2, S3, S4, S5, S6, LONG3):
            for layout in ("bricks", "c4"):
                if layout != "c4" or len(shape) >= 4:
                    yield "bricks", (layout,), "linear", kind, shape, NPTS, False
        for shape in (S2, S3, S4, LONG3):
            for linearize in (False, True):
                yield "tiles", ("off", "44", "24", "11"), "cubic", kind, shape, NPTS, linearize
        for row in SORTED:
            yield "sorted", row, "cubic", kind, row[1], SORTED_NOBS, len(row[1]) == 3
    for row in SWEEPS:
        if row[0] == "cubic":
            for linearize in (False, True):
                yield "sweep", row, "cubic", row[1], row[2], SWEEP_NOBS, linearize


def plane_id(row):
    family, sub, method, kind, shape, nobs, linearize = row
    return f"{family}-{sub[0]}-{kind}-{'x'.join(map(str, shape))}-{'lin' if linearize else 'quad'}"
