"""Field-set gradients on a lattice (interpn_hip_fields_eval_lattice_grad_*, interpn_hip_fields_lattice_grad_plan), the
part that needs no GPU: exported symbols, the plan against a restatement of the documented formula, the hand-computed cases,
the unchanged value and single-field plans, statuses and Python argument errors decided before any device work, and the
build resources of the new translation unit."""

import ctypes
import itertools
import os
import re
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
DEFAULT_BUDGET = 20 * 1024

SYMBOLS = ["interpn_hip_fields_eval_lattice_grad_device", "interpn_hip_fields_eval_lattice_grad_host",
           "interpn_hip_fields_reserve_lattice_grad", "interpn_hip_fields_lattice_grad_plan"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_AXIS_LDS_KB", "INTERPN_HIP_LATTICE", "INTERPN_HIP_FORCE_GENERIC"):
        monkeypatch.delenv(name, raising=False)


def _call_plan(fn, elem, method, dims, lens, k, layout):
    d = (c_size_t * max(len(dims), 1))(*[int(v) for v in dims])
    m = (c_size_t * max(len(lens), 1))(*[int(v) for v in lens])
    path, group, lds, npts = c_int(-1), c_size_t(99), c_size_t(99), c_size_t(0)
    st = fn(elem, method, len(dims), d, m, k, layout, ctypes.byref(path), ctypes.byref(group), ctypes.byref(lds), ctypes.byref(npts))
    return st, path.value, group.value, lds.value, npts.value


def _plan(lib, elem, method, dims, lens, k, layout):
    return _call_plan(lib.interpn_hip_fields_lattice_grad_plan, elem, method, dims, lens, k, layout)


def _round16(v):
    return (v + 15) // 16 * 16


def _lines(method, n):
    return n + 1 if method == LINEAR else n


def _wave_bytes(method, n, n_last, elem, g, layout):
    """lattice.h: g x L packed lines of n_last elements, and for fields-last results a [64] x ((g (N + 1)) | 1) tile."""
    tile = _round16(64 * ((g * (n + 1)) | 1) * elem) if layout == FIELDS_LAST else 0
    return _round16(g * _lines(method, n) * n_last * elem) + tile


def _restated(elem, method, dims, lens, k, layout, budget, mode, force_generic):
    """(path, group, lds_bytes) by the rules written in lattice.h and include/interpn_hip.h."""
    n = len(dims)
    per_field = (PER_FIELD, 0, 0)
    if force_generic or mode == 0 or method not in (LINEAR, CUBIC) or n not in (2, 3):
        return per_field
    if int(np.prod(dims, dtype=object)) >= 0xFFFFFFFF or int(np.prod(lens, dtype=object)) == 0:
        return per_field
    # the single handle's gradient plan: L lines of one field
    if WAVES * _round16(_lines(method, n) * dims[-1] * elem) > budget or any(m >= 2**31 for m in lens):
        return per_field
    if mode == -1:
        rows = int(np.prod(lens[:-1], dtype=object))
        if rows < WAVES * DEFAULT_CUS or dims[-1] > 4 * max(lens[-1], 64):
            return per_field
    g = 0
    while g < min(k, CAP) and WAVES * _wave_bytes(method, n, dims[-1], elem, g + 1, layout) <= budget:
        g += 1
    if g == 0:
        return per_field
    return FUSED, g, WAVES * _wave_bytes(method, n, dims[-1], elem, g, layout)


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in header, s
    assert "Field-set gradients on a lattice" in header
    import interpn_amd
    from interpn_amd import autograd

    for name in ("interpn_fields_lattice_grad", "fields_lattice_grad_plan"):
        assert name in interpn_amd.__all__ and callable(getattr(interpn_amd, name)), name
    for name in ("eval_lattice_grad_host", "eval_lattice_grad_tensors", "eval_lattice_grad", "reserve_lattice_grad"):
        assert hasattr(interpn_amd.Fields, name), name
    assert callable(autograd.interp_fields_lattice)
    assert len(interpn_amd.raw.__all__) == 16
    makefile = open(os.path.join(ROOT, "interpn_amd", "csrc", "Makefile")).read()
    for unit in ("k_lattice_fields_grad.hip", "abi_fields_lattice_grad.hip", "lattice_fields_grad.h"):
        assert unit in makefile, unit


def _shapes(n):
    """Grids and lattices per N: enough rows for the automatic rule and too few, a last grid axis that is long against the
    last lattice axis, ones that take most of a budget."""
    if n == 1:
        return [([50], [3000])]
    if n == 2:
        return [([37, 53], [2000, 67]), ([37, 53], [41, 67]), ([9, 600], [3000, 100]), ([9, 300], [3000, 70]), ([9, 1200], [1100, 400]),
                ([9, 8], [2000, 70])]
    if n == 3:
        return [([17, 12, 23], [40, 40, 71]), ([17, 12, 23], [11, 13, 71]), ([5, 6, 160], [64, 64, 200]), ([5, 6, 300], [64, 64, 70]),
                ([7, 6, 5], [40, 40, 9])]
    return [([5, 6, 7, 8], [9, 9, 9, 9])]


@pytest.mark.parametrize("kb", [None, 1, 7, 60])
@pytest.mark.parametrize("mode", [None, 0, 1])
def test_plan_matches_the_documented_formula(lib, monkeypatch, kb, mode):
    budget = DEFAULT_BUDGET if kb is None else kb * 1024
    if kb is not None:
        monkeypatch.setenv("INTERPN_HIP_AXIS_LDS_KB", str(kb))
    if mode is not None:
        monkeypatch.setenv("INTERPN_HIP_LATTICE", str(mode))
    seen = set()
    for force in (False, True):
        if force:
            monkeypatch.setenv("INTERPN_HIP_FORCE_GENERIC", "1")
        for elem, method, n, k, layout in itertools.product((4, 8), (LINEAR, CUBIC, NEAREST), (1, 2, 3, 4), (1, 2, 3, 8, 9),
                                                            (FIELD_MAJOR, FIELDS_LAST)):
            for dims, lens in _shapes(n):
                st, path, group, lds, npts = _plan(lib, elem, method, dims, lens, k, layout)
                if method == NEAREST:
                    assert st == UNSUPPORTED  # no gradient form
                    continue
                assert st == OK
                assert npts == int(np.prod(lens, dtype=object))
                want = _restated(elem, method, dims, lens, k, layout, budget, -1 if mode is None else mode, force)
                assert (path, group, lds) == want, (elem, method, dims, lens, k, layout, kb, mode, force)
                if path == FUSED:
                    assert 1 <= group <= min(k, CAP) and 0 < lds <= budget
                    seen.add((group == k, layout))
                else:
                    assert group == 0 and lds == 0
    if mode != 0 and kb != 1:  # (1 KiB: 256 bytes per wave hold no tile)
        assert seen >= {(True, FIELD_MAJOR), (True, FIELDS_LAST), (False, FIELD_MAJOR), (False, FIELDS_LAST)}, seen


def test_hand_computed_cases(lib, monkeypatch):
    """At the default 20 KiB budget (5120 bytes per wave) unless noted; lattices with enough rows for the automatic rules."""
    rows = [64, 64]
    # 3-D f64 multilinear, n_last = 64: L = 4 lines of 512 bytes per field; the tile of one field is 64 x 5 x 8 = 2560
    assert _plan(lib, 8, LINEAR, [8, 8, 64], rows + [200], 3, FIELD_MAJOR)[1:4] == (FUSED, 2, 16384)
    assert _plan(lib, 8, LINEAR, [8, 8, 64], rows + [200], 3, FIELDS_LAST)[1:4] == (FUSED, 1, 18432)
    # 3-D f64 multicubic, n_last = 64: L = 3
    assert _plan(lib, 8, CUBIC, [8, 8, 64], rows + [200], 8, FIELD_MAJOR)[1:4] == (FUSED, 3, 18432)
    assert _plan(lib, 8, CUBIC, [8, 8, 64], rows + [200], 8, FIELDS_LAST)[1:4] == (FUSED, 1, 16384)
    # 3-D f32 multilinear, n_last = 64: two fields' lines (2048) and a [64] x 9 tile (2304)
    assert _plan(lib, 4, LINEAR, [8, 8, 64], rows + [200], 4, FIELDS_LAST)[1:4] == (FUSED, 2, 17408)
    # 3-D f64 multilinear, n_last = 160: one field's lines take the whole budget; 161: not even those
    assert _plan(lib, 8, LINEAR, [8, 8, 160], rows + [200], 3, FIELD_MAJOR)[1:4] == (FUSED, 1, 20480)
    assert _plan(lib, 8, LINEAR, [8, 8, 160], rows + [200], 3, FIELDS_LAST)[1:4] == (PER_FIELD, 0, 0)
    assert _plan(lib, 8, LINEAR, [8, 8, 161], rows + [200], 3, FIELD_MAJOR)[1:4] == (PER_FIELD, 0, 0)
    assert _plan(lib, 8, LINEAR, [8, 8, 161], rows + [200], 3, FIELDS_LAST)[1:4] == (PER_FIELD, 0, 0)
    # at the default budget a fields-last f64 3-D call never has G > 2: three fields' tile alone is 64 x 13 x 8 = 6656 bytes
    for method, n_last in ((LINEAR, 2), (CUBIC, 4), (LINEAR, 8), (CUBIC, 10)):
        assert _plan(lib, 8, method, [8, 8, n_last], rows + [200], 8, FIELDS_LAST)[1:3] == (FUSED, 2)
    assert _plan(lib, 8, LINEAR, [8, 8, 9], rows + [200], 8, FIELDS_LAST)[1:3] == (FUSED, 1)
    # 2-D f32 multicubic, n_last = 960, 60 KiB (15360 bytes per wave): L = 2 lines of 3840 bytes per field
    monkeypatch.setenv("INTERPN_HIP_AXIS_LDS_KB", "60")
    assert _plan(lib, 4, CUBIC, [540, 960], [1080, 1920], 3, FIELD_MAJOR)[1:4] == (FUSED, 2, 4 * 15360)
    assert _plan(lib, 4, CUBIC, [540, 960], [1080, 1920], 3, FIELDS_LAST)[1:4] == (FUSED, 1, 4 * (7680 + 768))


def test_value_and_single_field_plans_unchanged(lib):
    """fields_lattice_plan and lattice_grad_plan answer what they answered before (the cases of
    test_fields_lattice_cpu.py::test_plan_examples and test_lattice_grad_cpu.py), and a field-major set of one field
    follows the single handle's gradient plan."""
    rows = [64, 64]
    value = lib.interpn_hip_fields_lattice_plan
    assert _call_plan(value, 8, LINEAR, [64, 64, 64], rows + [200], 20, FIELD_MAJOR)[1:4] == (FUSED, 8, 4 * 8 * 512)
    assert _call_plan(value, 8, LINEAR, [64, 64, 64], rows + [200], 20, FIELDS_LAST)[1:4] == (FUSED, 5, 4 * 5120)
    assert _call_plan(value, 4, CUBIC, [8, 1000], [4096, 1000], 3, FIELDS_LAST)[1:4] == (FUSED, 1, 4 * 4256)
    assert _call_plan(value, 8, LINEAR, [8, 640], [4096, 1000], 2, FIELDS_LAST)[1:4] == (PER_FIELD, 0, 0)
    rows_min = WAVES * DEFAULT_CUS
    cases = [(8, LINEAR, [64, 64], [rows_min, 100], True), (8, LINEAR, [64, 64], [rows_min - 1, 100], False),
             (8, CUBIC, [64, 64, 64], [32, 32, 100], True), (8, CUBIC, [64, 64, 64], [32, 31, 100], False),
             (8, LINEAR, [8, 8, 160], [64, 64, 500], True), (8, LINEAR, [8, 8, 161], [64, 64, 500], False),
             (8, CUBIC, [8, 8, 213], [64, 64, 500], True), (8, CUBIC, [8, 8, 214], [64, 64, 500], False)]
    for elem, method, dims, lens, fused in cases:
        d = (c_size_t * len(dims))(*dims)
        m = (c_size_t * len(lens))(*lens)
        path, lds, npts = c_int(-1), c_size_t(0), c_size_t(0)
        st = lib.interpn_hip_lattice_grad_plan(elem, method, len(dims), d, m, ctypes.byref(path), ctypes.byref(lds), ctypes.byref(npts))
        assert (st, path.value) == (OK, 0 if fused else 1), (dims, lens)
        assert lds.value == (WAVES * _round16(_lines(method, len(dims)) * dims[-1] * elem) if fused else 0)
        assert _plan(lib, elem, method, dims, lens, 1, FIELD_MAJOR) == (OK, FUSED if fused else PER_FIELD, 1 if fused else 0, lds.value,
                                                                        npts.value)


def test_plan_argument_errors(lib):
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [3, 0, 9], 2, FIELD_MAJOR) == (OK, PER_FIELD, 0, 0, 0)
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [2**31, 2**31, 2], 2, FIELD_MAJOR)[0] == UNSUPPORTED
    assert _plan(lib, 8, LINEAR, [5] * 8, [2**8] * 8, 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 2, LINEAR, [5, 6], [3, 3], 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 8, 7, [5, 6], [3, 3], 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 8, CUBIC, [5, 3], [3, 3], 2, FIELD_MAJOR)[0] == INVALID
    assert _plan(lib, 8, NEAREST, [5, 6], [3, 3], 2, FIELD_MAJOR)[0] == UNSUPPORTED  # no gradient form
    assert _plan(lib, 8, LINEAR, [5, 6], [3, 3], 0, FIELD_MAJOR)[0] == INVALID       # no fields
    assert _plan(lib, 8, LINEAR, [5, 6], [3, 3], 2, 2)[0] == INVALID                 # no such layout
    assert _plan(lib, 8, LINEAR, [5, 6], [3, 3], 2, -1)[0] == INVALID
    d = (c_size_t * 2)(5, 6)
    fn = lib.interpn_hip_fields_lattice_grad_plan
    assert fn(8, LINEAR, 2, None, d, 2, 0, None, None, None, None) == INVALID
    assert fn(8, LINEAR, 2, d, None, 2, 0, None, None, None, None) == INVALID
    assert fn(8, LINEAR, 9, d, d, 2, 0, None, None, None, None) == INVALID
    assert fn(8, LINEAR, 2, d, d, 2, 0, None, None, None, None) == OK  # every output is optional


def test_null_and_bad_arguments(lib):
    """Without a device only the NULL set can be passed, which is refused first: no argument combination gets past it.  The
    later checks and their order are tested on a real set in tests/test_zoomed_field_set_jacobian_gpu.py."""
    lens = (c_size_t * 2)(3, 3)
    ptrs = (c_void_p * 2)()
    path = c_int(-7)
    dev, host = lib.interpn_hip_fields_eval_lattice_grad_device, lib.interpn_hip_fields_eval_lattice_grad_host
    assert dev(None, ptrs, lens, 2, None, 9, None, 9, FIELD_MAJOR, None, 0, ctypes.byref(path)) == INVALID  # null set
    assert path.value == PER_FIELD
    assert dev(None, None, lens, 2, None, 9, None, 9, FIELD_MAJOR, None, 0, None) == INVALID   # null axes
    assert dev(None, ptrs, lens, 2, None, 9, None, 9, 2, None, 0, None) == INVALID             # bad layout value
    assert dev(None, ptrs, lens, 2, None, 9, None, 9, FIELD_MAJOR, None, 2, None) == INVALID   # unknown flag
    assert dev(None, ptrs, lens, 2, None, 9, None, 8, FIELD_MAJOR, None, 0, None) == INVALID   # stride too small
    assert host(None, ptrs, lens, 2, None, 9, None, 18, FIELDS_LAST, None) == INVALID
    assert host(None, None, lens, 2, None, 9, None, 18, FIELDS_LAST, None) == INVALID
    assert host(None, ptrs, lens, 2, None, 9, None, 18, 7, None) == INVALID
    assert lib.interpn_hip_fields_reserve_lattice_grad(None, lens, 2, 1) == INVALID


def test_python_argument_errors():
    """Decided before a device is touched: a handle-less set is enough."""
    import interpn_amd

    fs = interpn_amd.Fields(0, np.float64, 3, 2)
    axes = [np.zeros(3), np.zeros(4), np.zeros(5)]
    with pytest.raises(ValueError, match="field_axis"):
        fs.eval_lattice_grad_host(axes, field_axis=1)
    with pytest.raises(ValueError, match="field_axis"):
        fs.eval_lattice_grad_tensors(axes, field_axis=2)
    with pytest.raises(TypeError, match=r"axes\[1\].*expected dtype float64"):
        fs.eval_lattice_grad_host([axes[0], axes[1].astype(np.float32), axes[2]])
    with pytest.raises(ValueError, match=r"out: expected shape \(2, 3, 4, 5\)"):
        fs.eval_lattice_grad_host(axes, np.zeros((3, 4, 5, 2)))
    with pytest.raises(ValueError, match=r"jac: expected shape \(2, 3, 3, 4, 5\)"):
        fs.eval_lattice_grad_host(axes, None, np.zeros((3, 4, 5, 2, 3)))
    with pytest.raises(ValueError, match=r"jac: expected shape \(3, 4, 5, 2, 3\)"):
        fs.eval_lattice_grad_host(axes, None, np.zeros((2, 3, 3, 4, 5)), field_axis=-1)
    with pytest.raises(TypeError, match="argument 'jac': expected dtype float64"):
        fs.eval_lattice_grad_host(axes, None, np.zeros((2, 3, 3, 4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="each component's block must be contiguous"):
        fs.eval_lattice_grad_host(axes, None, np.zeros((2, 3, 3, 4, 10))[..., ::2])
    with pytest.raises(ValueError, match="one uniform stride"):
        fs.eval_lattice_grad_host(axes, None, np.zeros((2, 4, 3, 4, 5))[:, :3])
    with pytest.raises(ValueError, match="C-contiguous array, or a 3-D"):
        fs.eval_lattice_grad_host(axes, None, np.zeros((3, 4, 5, 2, 4))[..., :3], field_axis=-1)
    with pytest.raises(ValueError, match="every row of K \\* N elements must be contiguous"):
        fs.eval_lattice_grad_host(axes, None, np.zeros((60, 2, 6))[:, :, ::2], field_axis=-1)
    ro = np.zeros((2, 3, 3, 4, 5))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        fs.eval_lattice_grad_host(axes, None, ro)
    # accepted layouts reach the library, which refuses the null set: INTERPN_HIP_ERR_INVALID_ARGUMENT
    for out, jac, axis in ((None, None, 0), (None, None, -1), (np.zeros((4, 3, 4, 5))[::2], np.zeros((2, 3, 70))[:, :, :60], 0),
                           (np.zeros((2, 60)), np.zeros((2, 3, 60)), 0), (np.zeros((60, 5))[:, :2], np.zeros((60, 3, 3))[:, :2], -1)):
        with pytest.raises(ValueError, match="[Ii]nvalid"):
            fs.eval_lattice_grad_host(axes, out, jac, field_axis=axis)
    with pytest.raises(TypeError, match=r"axes\[0\]: expected a contiguous 1-D"):
        fs.eval_lattice_grad_tensors(axes)
    with pytest.raises(TypeError, match="takes no"):
        fs.eval_lattice_grad(axes, no_alloc=True)
    fs._h = c_void_p(None)  # nothing to destroy

    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    vals = np.zeros((3, 4, 5))
    ax2 = [np.zeros(3), np.zeros(6)]
    with pytest.raises(ValueError, match="field_axis"):
        interpn_amd.interpn_fields_lattice_grad(ax2, grids, vals, field_axis=1)
    with pytest.raises(ValueError, match="Unsupported interpolation configuration"):
        interpn_amd.interpn_fields_lattice_grad(ax2, grids, vals, method="quintic")
    with pytest.raises(ValueError, match="expected 2 coordinate vectors"):
        interpn_amd.interpn_fields_lattice_grad(ax2[:1], grids, vals)
    with pytest.raises(ValueError, match=r"vals: expected 5 x 20 values"):
        interpn_amd.interpn_fields_lattice_grad(ax2, grids, vals, field_axis=-1)
    with pytest.raises(ValueError, match="expected 2 lengths"):
        interpn_amd.fields_lattice_grad_plan(np.float64, "linear", [4, 5], [3], 2)
    with pytest.raises(ValueError, match="field_axis"):
        interpn_amd.fields_lattice_grad_plan(np.float64, "linear", [4, 5], [3, 3], 2, field_axis=1)
    # 2-D f32 multicubic, n_last = 5: L = 2 lines of 20 bytes per field; fields-last adds a [64] x 9 tile
    assert interpn_amd.fields_lattice_grad_plan(np.float32, "cubic", [4, 5], [3000, 7], 3) == ("fused", 3, 4 * 128, 21000)
    assert interpn_amd.fields_lattice_grad_plan(np.float32, "cubic", [4, 5], [3000, 7], 3, field_axis=-1) == (
        "fused", 3, 4 * (128 + 64 * 9 * 4), 21000)


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_row_kernel_build_resources(tmp_path):
    from tools.kernel_resources import parse

    csrc = os.path.join(ROOT, "interpn_amd", "csrc")
    src = os.path.join(csrc, "k_lattice_fields_grad.hip")
    for name in ("k_lattice_fields_grad.hip", "lattice_fields_grad.h"):  # no inline assembly in the new unit
        assert not re.search(r"\basm\b|__asm", open(os.path.join(csrc, name)).read()), name
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_lattice_fields_grad.o")],
            stderr=err, cwd=csrc)
    rows = parse(str(remarks))
    names = sorted(r["demangled"].split("(")[0].replace("void ", "").replace("interpn::", "") for r in rows)
    want = sorted(f"k_lattice_fields_grad_rows<{t}, {method}, {n}, {rect}, {fma}, {last}>" for t, method, n, rect, fma, last in
                  itertools.product(("double", "float"), (0, 1), (2, 3), ("false", "true"), ("false", "true"), ("false", "true")))
    assert names == want, set(names) ^ set(want)  # the 64 instantiations and no other kernel
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 128 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]  # the bar of DESIGN.md sections 16, 18
