"""Field sets (interpn_hip_fields_*), the part that needs no GPU: exported symbols, every validation status of the
creators (returned before any device work), the layout helper against the closed formulas, the fused kernel's build
resources, and the argument handling of `interpn_fields`."""

import ctypes
import itertools
import os
import shutil
import subprocess
import sys
from ctypes import POINTER, c_double, c_float, c_size_t, c_void_p

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

OK, DIM_MISMATCH, MIN_TWO, MIN_2, MIN_FOUR, MIN_4, NOT_MONOTONIC = 0, 1, 2, 3, 4, 5, 6
TOO_MANY_DIMS, REFERENCE_PANIC, TOO_MANY_DIMS_6, INVALID, UNSUPPORTED = 8, 9, 10, 32, 33
LINEAR, CUBIC, NEAREST = 0, 1, 2

SYMBOLS = ["interpn_hip_create_fields_regular_f64", "interpn_hip_create_fields_regular_f32",
           "interpn_hip_create_fields_rectilinear_f64", "interpn_hip_create_fields_rectilinear_f32",
           "interpn_hip_fields_eval_device", "interpn_hip_fields_eval_host", "interpn_hip_fields_finish",
           "interpn_hip_fields_destroy", "interpn_hip_fields_count", "interpn_hip_fields_ndims", "interpn_hip_fields_elem_size",
           "interpn_hip_fields_device", "interpn_hip_fields_kernel_name", "interpn_hip_fields_set_option",
           "interpn_hip_fields_get_option", "interpn_hip_fields_layout"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in header or s.rsplit("_", 1)[0] + "_##SUFFIX" in header, s
    import interpn_amd

    for name in ("Fields", "interpn_fields", "fields_layout"):
        assert name in interpn_amd.__all__ and hasattr(interpn_amd, name)


def _regular(lib, dtype, method, dims, starts=None, steps=None, nvals=None, nfields=2, stride=None, vals="auto", mem=0,
             nstarts=None, nsteps=None, dims_null=False):
    ct = c_double if dtype == np.float64 else c_float
    sfx = "f64" if dtype == np.float64 else "f32"
    nd = len(dims)
    prod = int(np.prod(dims, dtype=object)) if nd else 1
    starts = np.zeros(nd, dtype) if starts is None else np.asarray(starts, dtype)
    steps = np.ones(nd, dtype) if steps is None else np.asarray(steps, dtype)
    stride = prod if stride is None else stride
    nvals = nfields * stride if nvals is None else nvals
    buf = np.zeros(min(max(nvals, 1), 1 << 16), dtype) if vals == "auto" else vals
    d = (c_size_t * max(nd, 1))(*[int(v) for v in dims])
    h = c_void_p()
    st = getattr(lib, f"interpn_hip_create_fields_regular_{sfx}")(
        method, None if dims_null else d, nd, starts.ctypes.data_as(POINTER(ct)), len(starts) if nstarts is None else nstarts,
        steps.ctypes.data_as(POINTER(ct)), len(steps) if nsteps is None else nsteps,
        None if buf is None else buf.ctypes.data_as(c_void_p), nvals, nfields, stride, mem, 0, -1, ctypes.byref(h))
    assert h.value is None or st == OK
    if h.value:
        lib.interpn_hip_fields_destroy(h)
    return st


def _rectilinear(lib, dtype, method, grids, nvals=None, nfields=2, stride=None, vals="auto", mem=0, grids_null=False):
    ct = c_double if dtype == np.float64 else c_float
    sfx = "f64" if dtype == np.float64 else "f32"
    grids = [None if g is None else np.asarray(g, dtype) for g in grids]
    ng = len(grids)
    lens_list = [0 if g is None else g.size for g in grids]
    prod = int(np.prod(lens_list, dtype=object)) if ng else 1
    stride = prod if stride is None else stride
    nvals = nfields * stride if nvals is None else nvals
    buf = np.zeros(min(max(nvals, 1), 1 << 16), dtype) if vals == "auto" else vals
    ptrs = (POINTER(ct) * max(ng, 1))()
    lens = (c_size_t * max(ng, 1))()
    for i, g in enumerate(grids):
        if g is not None:
            ptrs[i] = g.ctypes.data_as(POINTER(ct))
        lens[i] = lens_list[i]
    h = c_void_p()
    st = getattr(lib, f"interpn_hip_create_fields_rectilinear_{sfx}")(
        method, None if grids_null else ptrs, lens, ng, None if buf is None else buf.ctypes.data_as(c_void_p), nvals, nfields, stride, mem,
        0, -1, ctypes.byref(h))
    assert h.value is None or st == OK
    if h.value:
        lib.interpn_hip_fields_destroy(h)
    return st


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_fields_checks_come_first(lib, dtype):
    """nfields == 0, field_stride < prod(dims), nvals < (nfields - 1) * field_stride + prod(dims): INVALID_ARGUMENT, in front of
    every status of the single-field creators."""
    assert _regular(lib, dtype, LINEAR, [4, 5], nfields=0, nvals=20) == INVALID
    assert _regular(lib, dtype, LINEAR, [4, 5], stride=19) == INVALID
    assert _regular(lib, dtype, LINEAR, [4, 5], nfields=3, stride=25, nvals=69) == INVALID
    assert _regular(lib, dtype, LINEAR, [4, 5], nfields=3, stride=2**63, nvals=100) == INVALID  # the product overflows
    # ... also where the grid itself is invalid
    assert _regular(lib, dtype, LINEAR, [4, 1], stride=3) == INVALID
    assert _regular(lib, dtype, LINEAR, [4, 5], steps=[1, -1], nfields=0) == INVALID
    assert _regular(lib, dtype, LINEAR, [4, 5], nstarts=1, stride=19) == INVALID
    g = [np.arange(4.0), np.arange(5.0)]
    assert _rectilinear(lib, dtype, LINEAR, g, nfields=0, nvals=20) == INVALID
    assert _rectilinear(lib, dtype, LINEAR, g, stride=19) == INVALID
    assert _rectilinear(lib, dtype, LINEAR, g, nfields=3, stride=25, nvals=69) == INVALID
    assert _rectilinear(lib, dtype, CUBIC, [np.arange(3.0), np.arange(5.0)], stride=14) == INVALID
    # the smallest buffer that holds the fields passes these checks (and, without a GPU, stops at the device)
    st = _regular(lib, dtype, LINEAR, [4, 5], nfields=3, stride=25, nvals=70)
    assert st in (OK, 34), st


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_single_field_statuses_through_the_regular_creator(lib, dtype):
    R = lambda *a, **k: _regular(lib, dtype, *a, **k)
    # argument checks of create_regular, in its order
    assert R(LINEAR | 0x100 | 0x200, [4, 5]) == INVALID         # both flavour flags
    assert R(7, [4, 5]) == INVALID                              # unknown method
    assert R(LINEAR, [4, 5], mem=5) == INVALID                  # unknown memory kind
    # validate_regular
    assert R(LINEAR, [4, 5], nstarts=1) == DIM_MISMATCH
    assert R(LINEAR, [4, 5], nsteps=3) == DIM_MISMATCH
    assert R(NEAREST, [4, 5], nstarts=1) == DIM_MISMATCH
    assert R(LINEAR, [2] * 9) == TOO_MANY_DIMS
    assert R(LINEAR, []) == TOO_MANY_DIMS
    assert R(CUBIC, [4] * 9) == TOO_MANY_DIMS
    assert R(NEAREST, [2] * 7) == TOO_MANY_DIMS_6
    assert R(CUBIC, [4, 5], nstarts=1) == REFERENCE_PANIC       # the flattened arm's try_into().unwrap()
    assert R(CUBIC, [4] * 5, nstarts=4) == DIM_MISMATCH         # the recursive arm checks instead
    assert R(LINEAR, [4, 5], dims_null=True) == INVALID
    assert R(LINEAR, [2**40, 2**40], stride=0, nvals=0) == REFERENCE_PANIC  # prod(dims) overflows usize
    assert R(LINEAR, [4, 1]) == MIN_TWO
    assert R(NEAREST, [1, 4]) == MIN_TWO
    assert R(CUBIC, [4, 3]) == MIN_FOUR
    assert R(LINEAR, [4, 5], steps=[1, 0]) == NOT_MONOTONIC
    assert R(LINEAR, [4, 5], steps=[1, np.nan]) == NOT_MONOTONIC
    assert R(CUBIC, [4, 5], steps=[-1, 1]) == NOT_MONOTONIC
    too_long = 2147483392 if dtype == np.float64 else 16777217
    assert R(LINEAR, [too_long, 2], nfields=1) == UNSUPPORTED
    # the order: entries before monotonicity, dimension count before everything about the values
    assert R(LINEAR, [4, 1], steps=[1, 0]) == MIN_TWO
    assert R(LINEAR, [1] * 9, steps=[0] * 9) == TOO_MANY_DIMS
    assert R(LINEAR, [4, 5], vals=None) == INVALID               # behind the grid's validation, as in create_regular
    assert R(LINEAR, [4, 1], vals=None) == MIN_TWO


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_single_field_statuses_through_the_rectilinear_creator(lib, dtype):
    R = lambda *a, **k: _rectilinear(lib, dtype, *a, **k)
    a4, a5 = np.arange(4.0), np.arange(5.0)
    assert R(LINEAR | 0x300, [a4, a5]) == INVALID
    assert R(3, [a4, a5]) == INVALID
    assert R(LINEAR, [a4, a5], mem=2) == INVALID
    assert R(LINEAR, [a4] * 9) == TOO_MANY_DIMS
    assert R(CUBIC, []) == TOO_MANY_DIMS
    assert R(NEAREST, [a4] * 7) == TOO_MANY_DIMS_6
    assert R(LINEAR, [a4, a5], grids_null=True) == INVALID
    assert R(LINEAR, [a4, np.arange(1.0)]) == MIN_2
    assert R(NEAREST, [np.arange(1.0), a4]) == MIN_2
    assert R(CUBIC, [a4, np.arange(3.0)]) == MIN_4
    assert R(LINEAR, [a4, None], stride=0, nvals=0) == MIN_2     # a null axis has no entries
    assert R(LINEAR, [a4, np.array([1.0, 1.0, 2.0])]) == NOT_MONOTONIC
    assert R(LINEAR, [np.array([2.0, 1.0, 3.0]), a4]) == NOT_MONOTONIC
    assert R(CUBIC, [a4, np.array([0.0, np.nan, 2.0, 3.0])]) == NOT_MONOTONIC
    assert R(LINEAR, [a4, np.arange(1.0)], vals=None) == MIN_2
    assert R(LINEAR, [a4, a5], vals=None) == INVALID
    # only g[1] > g[0] is checked, as in the reference: an axis that is unsorted further up is accepted (stops at the device here)
    assert R(LINEAR, [a4, np.array([0.0, 1.0, 0.5, 2.0])]) in (OK, 34)


def test_strings_are_the_single_creators(lib):
    for code, msg in ((DIM_MISMATCH, "Dimension mismatch"), (MIN_TWO, "All grids must have at least two entries"),
                      (MIN_2, "All grids must have at least 2 entries"), (MIN_FOUR, "All grids must have at least four entries"),
                      (MIN_4, "All grids must have at least 4 entries"), (NOT_MONOTONIC, "All grids must be monotonically increasing")):
        assert lib.interpn_hip_strerror(code).decode() == msg


def test_null_set_arguments(lib):
    assert lib.interpn_hip_fields_eval_device(None, None, 0, None, 0, 0, None, 0, None) == INVALID
    assert lib.interpn_hip_fields_eval_host(None, None, None, 0, None, 0, 0) == INVALID
    assert lib.interpn_hip_fields_finish(None, None, None) == INVALID
    assert lib.interpn_hip_fields_count(None) == 0 and lib.interpn_hip_fields_ndims(None) == 0
    assert lib.interpn_hip_fields_elem_size(None) == 0 and lib.interpn_hip_fields_device(None) == -1
    assert lib.interpn_hip_fields_set_option(None, b"fused", 0) == INVALID
    lib.interpn_hip_fields_destroy(None)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_layout_closed_formulas(dtype, n, k):
    """P = 128 / (2^N sizeof(T)) fields per line, ceil(K / P) lines per cell, prod(n_d - 1) * ceil(K / P) * 128 bytes."""
    import interpn_amd

    dims = [64, 33, 17][:n]
    elem = np.dtype(dtype).itemsize
    per_line = 128 // (2**n * elem)
    assert per_line == {(8, 3): 2, (8, 2): 4, (4, 3): 4, (4, 2): 8}[(elem, n)]
    lines = -(-k // per_line)
    cells = int(np.prod([d - 1 for d in dims]))
    assert interpn_amd.fields_layout(dtype, dims, k) == (per_line, lines, cells * lines * 128)


def test_layout_rejects_what_has_no_fused_form(lib):
    import interpn_amd

    for dims in ([64], [8, 8, 8, 8], [8, 1], []):
        with pytest.raises(ValueError):
            interpn_amd.fields_layout(np.float64, dims, 4)
    with pytest.raises(ValueError):
        interpn_amd.fields_layout(np.float64, [8, 8], 0)
    d = (c_size_t * 2)(8, 8)
    assert lib.interpn_hip_fields_layout(2, 2, d, 4, None, None, None) == INVALID
    assert lib.interpn_hip_fields_layout(8, 2, None, 4, None, None, None) == INVALID
    assert lib.interpn_hip_fields_layout(8, 2, d, 4, None, None, None) == OK
    d = (c_size_t * 3)(2**30, 2**30, 2**30)
    assert lib.interpn_hip_fields_layout(8, 3, d, 4, None, None, None) == INVALID  # the size does not fit size_t


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_fused_kernel_has_no_scratch_and_no_agprs(tmp_path):
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_linear_fields.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_linear_fields.o")],
            stderr=err, cwd=os.path.dirname(src))
    rows = [r for r in parse(str(remarks)) if "k_linear_fields<" in r["demangled"]]
    names = {r["demangled"].split("(")[0].replace("void ", "") for r in rows}
    want = {f"k_linear_fields<{t}, {n}, {rect}, {fma}>" for t, n, rect, fma in
            itertools.product(("double", "float"), (2, 3), ("false", "true"), ("false", "true"))}
    assert names == want, names ^ want
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 128 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]  # four waves per SIMD at least
    build = [r for r in parse(str(remarks)) if "k_fields_build<" in r["demangled"]]
    assert len(build) == 4 and all(r["scratch"] == 0 for r in build)


def test_interpn_fields_argument_errors():
    """Everything here is decided before a device is touched."""
    import interpn_amd

    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    obs = [np.zeros(3), np.zeros(3)]
    vals = np.zeros((2, 4, 5))
    with pytest.raises(ValueError, match="field_axis"):
        interpn_amd.interpn_fields(obs, grids, vals, field_axis=1)
    with pytest.raises(ValueError, match="Unsupported interpolation configuration"):
        interpn_amd.interpn_fields(obs, grids, vals, method="quintic")
    with pytest.raises(ValueError, match="field axis"):
        interpn_amd.interpn_fields(obs, grids, np.zeros(20))
    with pytest.raises(ValueError, match="expected 2 x 20 values"):
        interpn_amd.interpn_fields(obs, grids, np.zeros((2, 4, 6)))
    with pytest.raises(ValueError, match="expected 5 x 20 values"):
        interpn_amd.interpn_fields(obs, grids, np.zeros((4, 6, 5)), field_axis=-1)
    with pytest.raises(AssertionError, match="float32 and float64"):
        interpn_amd.interpn_fields(obs, grids, np.zeros((2, 4, 5), dtype=np.int32))
    with pytest.raises(AssertionError, match="float32 and float64"):
        interpn_amd.interpn_fields(obs, grids, np.zeros((2, 4, 5), dtype=np.float16))
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        interpn_amd.interpn_fields(obs, grids, [[0.0] * 20] * 2)
    with pytest.raises(ValueError, match="out: expected shape"):
        interpn_amd.interpn_fields(obs, grids, vals, out=np.zeros((3, 2)))
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 2\)"):
        interpn_amd.interpn_fields(obs, grids, np.zeros((4, 5, 2)), field_axis=-1, out=np.zeros((2, 3)))


def test_fields_class_argument_errors():
    import interpn_amd

    starts, steps = np.zeros(2), np.ones(2)
    with pytest.raises(ValueError, match=r"\(K, \*dims\)"):
        interpn_amd.Fields.regular("linear", [4, 5], starts, steps, np.zeros(40))
    with pytest.raises(ValueError, match="20 values per field"):
        interpn_amd.Fields.regular("linear", [4, 5], starts, steps, np.zeros((2, 21)))
    with pytest.raises(TypeError, match="expected dtype float64"):
        interpn_amd.Fields.regular("linear", [4, 5], starts, steps, np.zeros((2, 20), dtype=np.float32))
    with pytest.raises(ValueError, match="at least one field"):
        interpn_amd.Fields.regular("linear", [4, 5], starts, steps, [])
    with pytest.raises(AssertionError, match="All grids must have at least two entries"):
        interpn_amd.Fields.regular("linear", [4, 1], starts, steps, np.zeros((2, 4)))
    with pytest.raises(AssertionError, match="All grids must have at least 4 entries"):
        interpn_amd.Fields.rectilinear("cubic", [np.arange(4.0), np.arange(3.0)], np.zeros((2, 12)))
