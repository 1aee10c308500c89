"""Field sets on a lattice (interpn_hip_fields_eval_lattice_*, interpn_hip_fields_lattice_plan), the part that needs no GPU:
exported symbols, the plan against a restatement of the documented formula, its invariants, the unchanged single-field plan,
argument errors decided before any device work, and the build resources of the new translation unit."""

import ctypes
import itertools
import os
import shutil
import subprocess
import sys
from ctypes import c_int, c_size_t, c_void_p

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OK, INVALID, UNSUPPORTED = 0, 32, 33
LINEAR, CUBIC, NEAREST = 0, 1, 2
FUSED, PER_FIELD = 0, 1
FIELD_MAJOR, FIELDS_LAST = 0, 1
WAVES = 4            # rows in flight per workgroup of the row kernel
CAP = 8              # fields per pass at most
DEFAULT_CUS = 256    # the device the plan assumes
DEFAULT_LDS_PER_CU = 160 * 1024

SYMBOLS = ["interpn_hip_fields_eval_lattice_device", "interpn_hip_fields_eval_lattice_host", "interpn_hip_fields_reserve_lattice",
           "interpn_hip_fields_lattice_plan"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_AXIS_LDS_KB", "INTERPN_HIP_LATTICE", "INTERPN_HIP_FORCE_GENERIC"):
        monkeypatch.delenv(name, raising=False)


def _plan(lib, elem, method, dims, lens, k, layout):
    d = (c_size_t * max(len(dims), 1))(*[int(v) for v in dims])
    m = (c_size_t * max(len(lens), 1))(*[int(v) for v in lens])
    path, group, lds, npts = c_int(-1), c_size_t(99), c_size_t(99), c_size_t(0)
    st = lib.interpn_hip_fields_lattice_plan(elem, method, len(dims), d, m, k, layout, ctypes.byref(path), ctypes.byref(group),
                                             ctypes.byref(lds), ctypes.byref(npts))
    return st, path.value, group.value, lds.value, npts.value


def _single_plan(lib, elem, method, dims, lens):
    d = (c_size_t * max(len(dims), 1))(*[int(v) for v in dims])
    m = (c_size_t * max(len(lens), 1))(*[int(v) for v in lens])
    path, lds, npts = c_int(-1), c_size_t(0), c_size_t(0)
    st = lib.interpn_hip_lattice_plan(elem, method, len(dims), d, m, ctypes.byref(path), ctypes.byref(lds), ctypes.byref(npts))
    return st, path.value, lds.value, npts.value


def _round16(v):
    return (v + 15) // 16 * 16


def _wave_bytes(n_last, elem, g, layout):
    """lattice.h: g lines of n_last elements, and for fields-last results a [64][g | 1] tile."""
    return g * _round16(n_last * elem) + (_round16(64 * (g | 1) * elem) if layout == FIELDS_LAST else 0)


def _restated(elem, method, dims, lens, k, layout, budget, mode, force_generic):
    """(path, group, lds_bytes) by the rules written in lattice.h and include/interpn_hip.h."""
    n = len(dims)
    per_field = (PER_FIELD, 0, 0)
    if force_generic or mode == 0 or method not in (LINEAR, CUBIC) or n not in (2, 3):
        return per_field
    if int(np.prod(dims, dtype=object)) >= 0xFFFFFFFF or int(np.prod(lens, dtype=object)) == 0:
        return per_field
    if WAVES * _round16(dims[-1] * elem) > budget or any(m >= 2**31 for m in lens):
        return per_field
    if mode == -1:
        rows = int(np.prod(lens[:-1], dtype=object))
        if rows < WAVES * DEFAULT_CUS or dims[-1] > 4 * max(lens[-1], 64):
            return per_field
    g = 0
    while g < min(k, CAP) and WAVES * _wave_bytes(dims[-1], elem, g + 1, layout) <= budget:
        g += 1
    if g == 0:
        return per_field
    return FUSED, g, WAVES * _wave_bytes(dims[-1], elem, g, layout)


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in header, s
    for name in ("INTERPN_HIP_FIELDS_LATTICE_FIELD_MAJOR = 0", "INTERPN_HIP_FIELDS_LATTICE_FIELDS_LAST = 1",
                 "INTERPN_HIP_FIELDS_LATTICE_PATH_FUSED = 0", "INTERPN_HIP_FIELDS_LATTICE_PATH_PER_FIELD = 1", "Field sets on a lattice"):
        assert name in header, name
    import interpn_amd
    from interpn_amd import _lib

    for name in ("interpn_fields_lattice", "fields_lattice_plan"):
        assert name in interpn_amd.__all__ and callable(getattr(interpn_amd, name))
    for name in ("eval_lattice_host", "eval_lattice_tensors", "eval_lattice", "reserve_lattice", "last_lattice_path"):
        assert hasattr(interpn_amd.Fields, name), name
    assert _lib.FIELDS_LATTICE_PATHS == {0: "fused", 1: "per_field"}
    assert (_lib.FIELDS_LATTICE_FIELD_MAJOR, _lib.FIELDS_LATTICE_FIELDS_LAST) == (0, 1)
    assert len(interpn_amd.raw.__all__) == 16 and not [n for n in interpn_amd.raw.__all__ if "lattice" in n]
    for unit in ("k_lattice_fields.hip", "abi_fields_lattice.hip", "lattice_rows.h"):
        assert unit in open(os.path.join(ROOT, "interpn_amd", "csrc", "Makefile")).read(), unit


def _shapes(n):
    """Grids and lattices per N: enough rows for the automatic rule and too few, a last grid axis that is long against the
    last lattice axis, one that takes most of the default budget."""
    if n == 1:
        return [([50], [3000])]
    if n == 2:
        return [([37, 53], [2000, 67]), ([37, 53], [41, 67]), ([9, 600], [3000, 100]), ([9, 300], [3000, 70]), ([9, 1200], [1100, 400])]
    if n == 3:
        return [([17, 12, 23], [40, 40, 71]), ([17, 12, 23], [11, 13, 71]), ([5, 6, 640], [64, 64, 200]), ([5, 6, 300], [64, 64, 70])]
    return [([5, 6, 7, 8], [9, 9, 9, 9])]


@pytest.mark.parametrize("kb", [None, 1, 7, 60])
@pytest.mark.parametrize("mode", [None, 0, 1])
def test_plan_matches_the_documented_formula(lib, monkeypatch, kb, mode):
    budget = DEFAULT_LDS_PER_CU // 8 if kb is None else kb * 1024
    if kb is not None:
        monkeypatch.setenv("INTERPN_HIP_AXIS_LDS_KB", str(kb))
    if mode is not None:
        monkeypatch.setenv("INTERPN_HIP_LATTICE", str(mode))
    seen = set()
    for force in (False, True):
        if force:
            monkeypatch.setenv("INTERPN_HIP_FORCE_GENERIC", "1")
        for elem, method, n, k, layout in itertools.product((4, 8), (LINEAR, CUBIC, NEAREST), (1, 2, 3, 4), (1, 2, 3, 8, 9, 20),
                                                            (FIELD_MAJOR, FIELDS_LAST)):
            for dims, lens in _shapes(n):
                st, path, group, lds, npts = _plan(lib, elem, method, dims, lens, k, layout)
                assert st == OK
                assert npts == int(np.prod(lens, dtype=object))
                want = _restated(elem, method, dims, lens, k, layout, budget, -1 if mode is None else mode, force)
                assert (path, group, lds) == want, (elem, method, dims, lens, k, layout, kb, mode, force)
                # invariants
                if path == FUSED:
                    assert 1 <= group <= min(k, CAP) and 0 < lds <= budget
                    seen.add((group == k, layout))
                else:
                    assert group == 0 and lds == 0
    if mode != 0 and kb != 1:  # (1 KiB: 256 bytes per wave hold no tile)
        assert seen >= {(True, FIELD_MAJOR), (True, FIELDS_LAST), (False, FIELD_MAJOR)}, seen  # whole sets and several passes


def test_plan_examples(lib):
    """Hand-computed cases at the default 20 KiB budget (5120 bytes per wave)."""
    rows = [64, 64]
    # f64, n_last = 64: lines of 512 bytes; field-major takes the cap, fields-last 5 lines + a [64][5] tile = 5120
    assert _plan(lib, 8, LINEAR, [64, 64, 64], rows + [200], 20, FIELD_MAJOR)[1:4] == (FUSED, 8, 4 * 8 * 512)
    assert _plan(lib, 8, LINEAR, [64, 64, 64], rows + [200], 20, FIELDS_LAST)[1:4] == (FUSED, 5, 4 * 5120)
    assert _plan(lib, 8, LINEAR, [64, 64, 64], rows + [200], 3, FIELDS_LAST)[1:4] == (FUSED, 3, 4 * (3 * 512 + 64 * 3 * 8))
    # f32, n_last = 1000: a line of 4000 bytes and the tile of one field (256) fit, two lines do not
    assert _plan(lib, 4, CUBIC, [8, 1000], [4096, 1000], 1, FIELDS_LAST)[1:4] == (FUSED, 1, 4 * 4256)
    assert _plan(lib, 4, CUBIC, [8, 1000], [4096, 1000], 3, FIELD_MAJOR)[1:4] == (FUSED, 1, 4 * 4000)
    # ... K = 3 fields-last stores runs of one element per point in three passes: fused all the same (measured rule)
    assert _plan(lib, 4, CUBIC, [8, 1000], [4096, 1000], 3, FIELDS_LAST)[1:4] == (FUSED, 1, 4 * 4256)
    assert _plan(lib, 8, CUBIC, [8, 200], [4096, 1000], 3, FIELDS_LAST)[1:4] == (FUSED, 2, 4 * (2 * 1600 + 64 * 3 * 8))
    assert _plan(lib, 8, CUBIC, [8, 250], [4096, 1000], 3, FIELDS_LAST)[1:4] == (FUSED, 1, 4 * (2000 + 64 * 8))
    # the line fits alone but not with the tile of one field: per field for fields-last only
    n_last = 5120 // 8
    assert _plan(lib, 8, LINEAR, [8, n_last], [4096, 1000], 2, FIELD_MAJOR)[1:4] == (FUSED, 1, 4 * 5120)
    assert _plan(lib, 8, LINEAR, [8, n_last], [4096, 1000], 2, FIELDS_LAST)[1:4] == (PER_FIELD, 0, 0)


def test_single_field_plan_is_unchanged(lib):
    """The cases of test_lattice_cpu.py::test_plan_automatic_rules: interpn_hip_lattice_plan answers as before, and a set of
    one field in the field-major layout follows it."""
    rows_min = WAVES * DEFAULT_CUS
    cases = [(8, LINEAR, [64, 64], [rows_min, 100], True), (8, LINEAR, [64, 64], [rows_min - 1, 100], False),
             (8, CUBIC, [64, 64, 64], [32, 32, 100], True), (8, CUBIC, [64, 64, 64], [32, 31, 100], False),
             (8, LINEAR, [64, 64, 256], [64, 64, 1], True), (8, LINEAR, [64, 64, 257], [64, 64, 1], False),
             (8, LINEAR, [64, 64, 400], [64, 64, 100], True), (8, LINEAR, [64, 64, 401], [64, 64, 100], False),
             (4, LINEAR, [70000, 70000], [5000, 5000], False)]
    for elem, method, dims, lens, fused in cases:
        st, path, lds, npts = _single_plan(lib, elem, method, dims, lens)
        assert (st, path) == (OK, 0 if fused else 1), (dims, lens)
        assert lds == (WAVES * _round16(dims[-1] * elem) if fused else 0)
        st, fpath, group, flds, fnpts = _plan(lib, elem, method, dims, lens, 1, FIELD_MAJOR)
        assert (st, fpath, group, flds, fnpts) == (OK, FUSED if fused else PER_FIELD, 1 if fused else 0, lds, npts)


def test_plan_argument_errors(lib):
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [3, 0, 9], 2, FIELD_MAJOR) == (OK, PER_FIELD, 0, 0, 0)
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [2**31, 2**31, 2], 2, FIELD_MAJOR)[0] == UNSUPPORTED
    assert _plan(lib, 8, LINEAR, [5] * 8, [2**8] * 8, 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 2, LINEAR, [5, 6], [3, 3], 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 8, 7, [5, 6], [3, 3], 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 8, CUBIC, [5, 3], [3, 3], 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 8, LINEAR, [5, 6], [3, 3], 0, FIELD_MAJOR)[0] == INVALID   # no fields
    assert _plan(lib, 8, LINEAR, [5, 6], [3, 3], 2, 2)[0] == INVALID             # no such layout
    assert _plan(lib, 8, LINEAR, [5, 6], [3, 3], 2, -1)[0] == INVALID
    d = (c_size_t * 2)(5, 6)
    assert lib.interpn_hip_fields_lattice_plan(8, LINEAR, 2, None, d, 2, 0, None, None, None, None) == INVALID
    assert lib.interpn_hip_fields_lattice_plan(8, LINEAR, 2, d, None, 2, 0, None, None, None, None) == INVALID
    assert lib.interpn_hip_fields_lattice_plan(8, LINEAR, 9, d, d, 2, 0, None, None, None, None) == INVALID
    assert lib.interpn_hip_fields_lattice_plan(8, LINEAR, 2, d, d, 2, 0, None, None, None, None) == OK  # every output is optional


def test_null_and_bad_arguments(lib):
    """Without a device only the NULL set can be passed, which is refused by itself: that no argument combination gets past
    it is what these lines pin.  The layout, flag and stride checks proper, and their order, are tested on a real set in
    tests/test_fields_lattice_gpu.py::test_eval_lattice_dispatch_and_argument_errors_with_a_set."""
    lens = (c_size_t * 2)(3, 3)
    ptrs = (c_void_p * 2)()
    path = c_int(-7)
    dev, host = lib.interpn_hip_fields_eval_lattice_device, lib.interpn_hip_fields_eval_lattice_host
    assert dev(None, ptrs, lens, 2, None, 9, FIELD_MAJOR, None, 0, ctypes.byref(path)) == INVALID  # null set
    assert path.value == PER_FIELD
    assert dev(None, None, lens, 2, None, 9, FIELD_MAJOR, None, 0, None) == INVALID                # null axes
    assert dev(None, ptrs, lens, 2, None, 9, 2, None, 0, None) == INVALID                          # bad layout value
    assert dev(None, ptrs, lens, 2, None, 9, FIELD_MAJOR, None, 2, None) == INVALID                # unknown flag
    assert dev(None, ptrs, lens, 2, None, 8, FIELD_MAJOR, None, 0, None) == INVALID                # stride too small
    assert host(None, ptrs, lens, 2, None, 9, FIELDS_LAST, None) == INVALID
    assert host(None, None, lens, 2, None, 9, FIELDS_LAST, None) == INVALID
    assert host(None, ptrs, lens, 2, None, 9, 7, None) == INVALID
    assert lib.interpn_hip_fields_reserve_lattice(None, lens, 2, 1) == INVALID


def test_python_argument_errors():
    """Decided before a device is touched: a handle-less set is enough."""
    import interpn_amd

    fs = interpn_amd.Fields(0, np.float64, 3, 2)
    axes = [np.zeros(3), np.zeros(4), np.zeros(5)]
    with pytest.raises(ValueError, match="field_axis"):
        fs.eval_lattice_host(axes, field_axis=1)
    with pytest.raises(ValueError, match="field_axis"):
        fs.eval_lattice_tensors(axes, field_axis=2)
    with pytest.raises(TypeError, match=r"axes\[1\].*expected dtype float64"):
        fs.eval_lattice_host([axes[0], axes[1].astype(np.float32), axes[2]])
    with pytest.raises(TypeError, match="numpy array"):
        fs.eval_lattice_host([axes[0], axes[1], [0.0] * 5])
    with pytest.raises(ValueError, match=r"out: expected shape \(2, 3, 4, 5\)"):
        fs.eval_lattice_host(axes, np.zeros((3, 4, 5, 2)))
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 4, 5, 2\)"):
        fs.eval_lattice_host(axes, np.zeros((2, 3, 4, 5)), field_axis=-1)
    with pytest.raises(TypeError, match="argument 'out': expected dtype float64"):
        fs.eval_lattice_host(axes, np.zeros((2, 3, 4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="each field's block must be contiguous"):
        fs.eval_lattice_host(axes, np.zeros((2, 3, 4, 10))[..., ::2])
    with pytest.raises(ValueError, match="each field's block must be contiguous"):
        fs.eval_lattice_host(axes, np.zeros((2, 3, 8, 5))[:, :, ::2])
    with pytest.raises(ValueError, match="C-contiguous array, or a 2-D"):
        fs.eval_lattice_host(axes, np.zeros((3, 4, 5, 4))[..., :2], field_axis=-1)
    with pytest.raises(ValueError, match="every row must be contiguous"):
        fs.eval_lattice_host(axes, np.zeros((60, 4))[:, ::2], field_axis=-1)
    ro = np.zeros((2, 3, 4, 5))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        fs.eval_lattice_host(axes, ro)
    # accepted layouts reach the library, which refuses the null set: INTERPN_HIP_ERR_INVALID_ARGUMENT
    for out, axis in ((None, 0), (None, -1), (np.zeros((4, 3, 4, 5))[::2], 0), (np.zeros((2, 60)), 0), (np.zeros((60, 5))[:, :2], -1)):
        with pytest.raises(ValueError, match="[Ii]nvalid"):
            fs.eval_lattice_host(axes, out, field_axis=axis)
    with pytest.raises(TypeError, match=r"axes\[0\]: expected a contiguous 1-D"):
        fs.eval_lattice_tensors(axes)
    with pytest.raises(TypeError, match="takes no"):
        fs.eval_lattice(axes, no_alloc=True)
    fs._h = c_void_p(None)  # nothing to destroy

    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    vals = np.zeros((3, 4, 5))
    ax2 = [np.zeros(3), np.zeros(6)]
    with pytest.raises(ValueError, match="field_axis"):
        interpn_amd.interpn_fields_lattice(ax2, grids, vals, field_axis=1)
    with pytest.raises(ValueError, match="Unsupported interpolation configuration"):
        interpn_amd.interpn_fields_lattice(ax2, grids, vals, method="quintic")
    with pytest.raises(ValueError, match="expected 2 coordinate vectors"):
        interpn_amd.interpn_fields_lattice(ax2[:1], grids, vals)
    with pytest.raises(AssertionError, match="float32 and float64"):
        interpn_amd.interpn_fields_lattice(ax2, grids, vals.astype(np.int32))
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        interpn_amd.interpn_fields_lattice(ax2, grids, [[0.0] * 20] * 3)
    with pytest.raises(ValueError, match=r"vals: expected 5 x 20 values"):
        interpn_amd.interpn_fields_lattice(ax2, grids, vals, field_axis=-1)
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 3, 6\)"):
        interpn_amd.interpn_fields_lattice(ax2, grids, vals, out=np.zeros((3, 6, 3)))
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 6, 3\)"):
        interpn_amd.interpn_fields_lattice(ax2, grids, np.zeros((4, 5, 3)), field_axis=-1, out=np.zeros((3, 3, 6)))
    with pytest.raises(ValueError, match="expected 2 lengths"):
        interpn_amd.fields_lattice_plan(np.float64, "linear", [4, 5], [3], 2)
    with pytest.raises(ValueError, match="field_axis"):
        interpn_amd.fields_lattice_plan(np.float64, "linear", [4, 5], [3, 3], 2, field_axis=1)
    assert interpn_amd.fields_lattice_plan(np.float32, "cubic", [4, 5], [3000, 7], 3) == ("fused", 3, 4 * 3 * 32, 21000)
    assert interpn_amd.fields_lattice_plan(np.float32, "cubic", [4, 5], [3000, 7], 3, field_axis=-1) == (
        "fused", 3, 4 * (3 * 32 + 64 * 3 * 4), 21000)
    assert interpn_amd.fields_lattice_plan(np.float64, "nearest", [4, 5], [3000, 7], 3) == ("per_field", 0, 0, 21000)


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_fields_row_kernel_has_no_scratch_and_no_agprs(tmp_path):
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_lattice_fields.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_lattice_fields.o")],
            stderr=err, cwd=os.path.dirname(src))
    every = parse(str(remarks))
    rows = [r for r in every if "k_lattice_fields_rows<" in r["demangled"]]
    assert len(rows) == len(every) == 64  # the unit holds nothing else
    names = {r["demangled"].split("(")[0].replace("void ", "").replace("interpn::", "") for r in rows}
    want = {f"k_lattice_fields_rows<{t}, {method}, {n}, {rect}, {fma}, {last}>" for t, method, n, rect, fma, last in
            itertools.product(("double", "float"), (0, 1), (2, 3), ("false", "true"), ("false", "true"), ("false", "true"))}
    assert names == want, names ^ want
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 128 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]  # four waves per SIMD at least
