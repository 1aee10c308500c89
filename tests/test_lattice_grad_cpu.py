"""Gradients on a lattice (interpn_hip_eval_lattice_grad_*, interpn_hip_lattice_grad_plan), the part that needs no GPU:
exported symbols, the path verdict against a Python restatement of the rule and against hand-computed cases, the value
plan left as it was, argument errors decided before any device work, and the row kernel's build resources."""

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
FUSED, EXPANDED = 0, 1
WAVES = 4            # rows in flight per workgroup of the row kernel
DEFAULT_CUS = 256    # the device the plan functions assume
DEFAULT_LDS_PER_CU = 160 * 1024

SYMBOLS = ["interpn_hip_eval_lattice_grad_device", "interpn_hip_eval_lattice_grad_host", "interpn_hip_lattice_grad_plan"]
ENV = ("INTERPN_HIP_AXIS_LDS_KB", "INTERPN_HIP_LATTICE", "INTERPN_HIP_FORCE_GENERIC")


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _call(fn, elem, method, dims, lens):
    d = (c_size_t * max(len(dims), 1))(*[int(v) for v in dims])
    m = (c_size_t * max(len(lens), 1))(*[int(v) for v in lens])
    path, lds, npts = c_int(-1), c_size_t(0), c_size_t(0)
    st = fn(elem, method, len(dims), d, m, ctypes.byref(path), ctypes.byref(lds), ctypes.byref(npts))
    return st, path.value, lds.value, npts.value


def _plan(lib, elem, method, dims, lens):
    return _call(lib.interpn_hip_lattice_grad_plan, elem, method, dims, lens)


def _value_plan(lib, elem, method, dims, lens):
    return _call(lib.interpn_hip_lattice_plan, elem, method, dims, lens)


def _lines(method, n):
    """Lines of a wave: the value's, one per component d < N-1, and for multilinear handles the differences along the last axis."""
    return n + 1 if method == LINEAR else n


def _wave_bytes(method, n, n_last, elem):
    """The L lines of a wave lie packed; the wave's part is rounded up to 16 bytes."""
    return (_lines(method, n) * n_last * elem + 15) // 16 * 16


def _restated(elem, method, dims, lens, kb=None, mode=None, force_generic=False):
    """(status, path, lds_bytes, npoints) of interpn_hip_lattice_grad_plan, restated."""
    if method == NEAREST:
        return UNSUPPORTED, None, None, None
    n = len(dims)
    npoints = int(np.prod(lens, dtype=object))
    budget = DEFAULT_LDS_PER_CU // 8 if kb is None else kb * 1024
    mode = -1 if mode is None else mode
    lds = WAVES * _wave_bytes(method, n, dims[-1], elem)
    fused = method in (LINEAR, CUBIC) and n in (2, 3) and lds <= budget and mode != 0 and not force_generic
    fused = fused and npoints > 0 and int(np.prod(dims, dtype=object)) < 0xFFFFFFFF and all(m < 2**31 for m in lens)
    if fused and mode == -1:
        rows = int(np.prod(lens[:-1], dtype=object))
        fused = rows >= WAVES * DEFAULT_CUS and dims[-1] <= 4 * max(lens[-1], 64)
    return OK, (FUSED if fused else EXPANDED), (lds if fused else 0), npoints


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s + "(" in header, s
    assert "Gradients on a lattice" in header and "interpn::k_lattice_grad_rows<T, method, N, rectilinear, fma>" in header
    assert "interpn_hip_reserve_lattice_grad" not in header  # interpn_hip_reserve_lattice serves gradient calls
    import interpn_amd
    from interpn_amd import autograd

    for name in ("interpn_lattice_grad", "lattice_grad_plan"):
        assert name in interpn_amd.__all__ and hasattr(interpn_amd, name), name
    for name in ("eval_lattice_grad_host", "eval_lattice_grad_tensors"):
        assert hasattr(interpn_amd.Interpolator, name), name
    for cls in ("MultilinearRegular", "MultilinearRectilinear", "MulticubicRegular", "MulticubicRectilinear"):
        assert hasattr(getattr(interpn_amd, cls), "eval_lattice_grad"), cls
    for cls in ("NearestRegular", "NearestRectilinear"):
        assert not hasattr(getattr(interpn_amd, cls), "eval_lattice_grad"), cls
    assert hasattr(autograd, "interp_lattice")
    assert len(interpn_amd.raw.__all__) == 16
    makefile = open(os.path.join(ROOT, "interpn_amd", "csrc", "Makefile")).read()
    for unit in ("abi_lattice_grad.hip", "k_lattice_grad.hip", "lattice_grad.h"):
        assert unit in makefile, unit


SHAPES_BY_N = {1: ([300], [5000]), 2: ([40, 90], [2000, 70]), 3: ([20, 30, 90], [40, 40, 70]), 4: ([5, 6, 7, 90], [9, 9, 40, 70])}


@pytest.mark.parametrize("force_generic", [False, True], ids=["", "force_generic"])
@pytest.mark.parametrize("mode", [None, 0, 1], ids=["auto", "never", "fused"])
@pytest.mark.parametrize("kb", [None, 1, 7, 60])
def test_plan_against_a_restatement(lib, monkeypatch, kb, mode, force_generic):
    if kb is not None:
        monkeypatch.setenv("INTERPN_HIP_AXIS_LDS_KB", str(kb))
    if mode is not None:
        monkeypatch.setenv("INTERPN_HIP_LATTICE", str(mode))
    if force_generic:
        monkeypatch.setenv("INTERPN_HIP_FORCE_GENERIC", "1")
    budget = DEFAULT_LDS_PER_CU // 8 if kb is None else kb * 1024
    seen = set()
    for elem, method, n in itertools.product((8, 4), (LINEAR, CUBIC, NEAREST), (1, 2, 3, 4)):
        dims, lens = SHAPES_BY_N[n]
        # the last grid axis: the method's minimum, the two lengths at the budget's edge for this (elem, method, N), a long one
        edge = budget // (WAVES * max(_lines(method, n), 1) * elem)
        for n_last in sorted({4, max(edge, 4), max(edge, 4) + 1, dims[-1], 4000}):
            # the last lattice axis decides the automatic rule n_last <= 4 max(m_last, 64) both ways; few rows as well
            for m in (lens, lens[:-1] + [1000], [3] * (n - 1) + [lens[-1]]):
                d = dims[:-1] + [n_last]
                got = _plan(lib, elem, method, d, m)
                want = _restated(elem, method, d, m, kb, mode, force_generic)
                if want[0] != OK:
                    assert got[0] == want[0], (elem, method, d, m, got)
                    continue
                assert got == want, (elem, method, d, m, got, want)
                seen.add(got[1])
    if mode == 1 and not force_generic:
        assert seen == {FUSED, EXPANDED}


def test_hand_computed_cases_at_20_kib(lib):
    lens = [64, 64, 500]
    # 3-D f64 multilinear: 4 waves x 4 lines x 160 x 8 bytes = 20480
    assert _plan(lib, 8, LINEAR, [8, 8, 160], lens)[:3] == (OK, FUSED, 20480)
    assert _plan(lib, 8, LINEAR, [8, 8, 161], lens)[:3] == (OK, EXPANDED, 0)
    # 3-D f64 multicubic: 3 lines; 213 x 8 x 3 = 5112 -> 5120 per wave, 214 -> 5136
    assert _plan(lib, 8, CUBIC, [8, 8, 213], lens)[:3] == (OK, FUSED, 20480)
    assert _plan(lib, 8, CUBIC, [8, 8, 214], lens)[:3] == (OK, EXPANDED, 0)
    # the value call of the same shapes keeps one line per wave
    assert _value_plan(lib, 8, LINEAR, [8, 8, 161], lens)[:3] == (OK, FUSED, 4 * 1296)
    assert _value_plan(lib, 8, CUBIC, [8, 8, 214], lens)[:3] == (OK, FUSED, 4 * 1712)


def test_value_plan_unchanged(lib):
    """The cases of test_lattice_cpu.py::test_plan_automatic_rules, with the gradient's verdict beside them."""
    rows_min = WAVES * DEFAULT_CUS
    cases = [(8, LINEAR, [64, 64], [rows_min, 100], FUSED), (8, LINEAR, [64, 64], [rows_min - 1, 100], EXPANDED),
             (8, CUBIC, [64, 64, 64], [32, 32, 100], FUSED), (8, CUBIC, [64, 64, 64], [32, 31, 100], EXPANDED),
             (8, LINEAR, [64, 64, 256], [64, 64, 1], FUSED), (8, LINEAR, [64, 64, 257], [64, 64, 1], EXPANDED),
             (8, LINEAR, [64, 64, 400], [64, 64, 100], FUSED), (8, LINEAR, [64, 64, 401], [64, 64, 100], EXPANDED),
             (4, LINEAR, [70000, 70000], [5000, 5000], EXPANDED)]
    for elem, method, dims, lens, path in cases:
        st, got, lds, npts = _value_plan(lib, elem, method, dims, lens)
        assert (st, got) == (OK, path), (dims, lens)
        assert lds == (WAVES * ((dims[-1] * elem + 15) // 16 * 16) if path == FUSED else 0)
        assert _plan(lib, elem, method, dims, lens) == _restated(elem, method, dims, lens), (dims, lens)
        if WAVES * _wave_bytes(method, len(dims), dims[-1], elem) <= DEFAULT_LDS_PER_CU // 8:
            assert _plan(lib, elem, method, dims, lens)[1] == path  # where L lines fit, the two automatic rules are the value's


def test_errors_without_a_device(lib):
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [3, 0, 9])[0::3] == (OK, 0)
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [3, 0, 9])[1] == EXPANDED
    assert _plan(lib, 8, NEAREST, [5, 6, 7], [3, 4, 9])[0] == UNSUPPORTED
    assert _plan(lib, 8, NEAREST, [5, 1, 7], [3, 4, 9])[0] == INVALID  # the value plan's checks come first
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [2**31, 2**31, 2])[0] == UNSUPPORTED
    assert _plan(lib, 8, LINEAR, [5] * 8, [2**8] * 8)[0] == INVALID
    assert _plan(lib, 2, LINEAR, [5, 6], [3, 3])[0] == INVALID
    assert _plan(lib, 8, 7, [5, 6], [3, 3])[0] == INVALID
    assert _plan(lib, 8, CUBIC, [5, 3], [3, 3])[0] == INVALID
    assert _plan(lib, 4, LINEAR, [5, 2**24 + 1], [3, 3])[0] == UNSUPPORTED
    d = (c_size_t * 2)(5, 6)
    assert lib.interpn_hip_lattice_grad_plan(8, LINEAR, 2, None, d, None, None, None) == INVALID
    assert lib.interpn_hip_lattice_grad_plan(8, LINEAR, 2, d, None, None, None, None) == INVALID
    assert lib.interpn_hip_lattice_grad_plan(8, LINEAR, 9, d, d, None, None, None) == INVALID
    assert lib.interpn_hip_lattice_grad_plan(8, LINEAR, 2, d, d, None, None, None) == OK  # every output is optional
    lens = (c_size_t * 2)(3, 3)
    ptrs = (c_void_p * 2)()
    path = c_int(-7)
    assert lib.interpn_hip_eval_lattice_grad_device(None, ptrs, lens, 2, None, ptrs, None, 0, ctypes.byref(path)) == INVALID
    assert path.value == EXPANDED
    assert lib.interpn_hip_eval_lattice_grad_device(None, ptrs, lens, 2, None, ptrs, None, 2, None) == INVALID  # unknown flag
    assert lib.interpn_hip_eval_lattice_grad_host(None, ptrs, lens, 2, None, ptrs, None) == INVALID


def test_python_argument_errors():
    """Decided before a device is touched: a handle-less Interpolator is enough."""
    import interpn_amd

    it = interpn_amd.Interpolator(0, np.float64, 3)
    axes = [np.zeros(3), np.zeros(4), np.zeros(5)]
    with pytest.raises(TypeError, match=r"axes\[1\].*expected dtype float64"):
        it.eval_lattice_grad_host([axes[0], axes[1].astype(np.float32), axes[2]])
    with pytest.raises(TypeError, match=r"axes\[2\].*1-D"):
        it.eval_lattice_grad_host([axes[0], axes[1], np.zeros((5, 1))])
    with pytest.raises(TypeError, match="numpy array"):
        it.eval_lattice_grad_host([axes[0], axes[1], [0.0] * 5])
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 4, 5\)"):
        it.eval_lattice_grad_host(axes, np.zeros((3, 5, 4)))
    with pytest.raises(TypeError, match="argument 'out': expected dtype float64"):
        it.eval_lattice_grad_host(axes, np.zeros((3, 4, 5), dtype=np.float32))
    ro = np.zeros((3, 4, 5))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="argument 'out': array is read-only"):
        it.eval_lattice_grad_host(axes, ro)
    with pytest.raises(ValueError, match=r"grad: expected shape \(3, 3, 4, 5\)"):
        it.eval_lattice_grad_host(axes, None, np.zeros((3, 4, 5)))
    with pytest.raises(TypeError, match="argument 'grad': expected dtype float64"):
        it.eval_lattice_grad_host(axes, None, np.zeros((3, 3, 4, 5), dtype=np.float32))
    with pytest.raises(TypeError, match="argument 'grad': expected a numpy array"):
        it.eval_lattice_grad_host(axes, None, [[0.0]])
    with pytest.raises(ValueError, match="grad\\[d\\] must be contiguous"):
        it.eval_lattice_grad_host(axes, None, np.zeros((3, 3, 4, 10))[:, :, :, ::2])
    rg = np.zeros((3, 3, 4, 5))
    rg.flags.writeable = False
    with pytest.raises(ValueError, match="argument 'grad': array is read-only"):
        it.eval_lattice_grad_host(axes, None, rg)
    with pytest.raises(ValueError):  # the null handle itself: INTERPN_HIP_ERR_INVALID_ARGUMENT
        it.eval_lattice_grad_host(axes)
    with pytest.raises(ValueError):  # two vectors for three axes: no shape to hold `out` to, the library decides
        it.eval_lattice_grad_host(axes[:2])
    with pytest.raises(TypeError, match=r"axes\[0\]: expected a contiguous 1-D"):
        it.eval_lattice_grad_tensors(axes)

    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    vals = np.zeros((4, 5))
    ax2 = [np.zeros(3), np.zeros(6)]
    with pytest.raises(ValueError, match='method must be "linear" or "cubic"'):
        interpn_amd.interpn_lattice_grad(ax2, grids, vals, method="nearest")
    with pytest.raises(ValueError, match="expected 2 coordinate vectors"):
        interpn_amd.interpn_lattice_grad(ax2[:1], grids, vals)
    with pytest.raises(AssertionError, match="float32 and float64"):
        interpn_amd.interpn_lattice_grad(ax2, grids, vals.astype(np.int32))
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 6\)"):
        interpn_amd.interpn_lattice_grad(ax2, grids, vals, out=np.zeros((6, 3)))
    with pytest.raises(ValueError, match="expected 2 lengths"):
        interpn_amd.lattice_grad_plan(np.float64, "linear", [4, 5], [3])
    assert interpn_amd.lattice_grad_plan(np.float32, "cubic", [4, 5], [3000, 7]) == ("fused", 4 * 48, 21000)
    assert interpn_amd.lattice_grad_plan(np.float32, "linear", [4, 5], [3000, 7]) == ("fused", 4 * 64, 21000)
    assert interpn_amd.lattice_plan(np.float32, "cubic", [4, 5], [3000, 7]) == ("fused", 4 * 32, 21000)


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_row_kernel_build_resources(tmp_path):
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_lattice_grad.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_lattice_grad.o")],
            stderr=err, cwd=os.path.dirname(src))
    rows = parse(str(remarks))
    names = sorted(r["demangled"].split("(")[0].replace("void ", "").replace("interpn::", "") for r in rows)
    want = sorted(f"k_lattice_grad_rows<{t}, {method}, {n}, {rect}, {fma}>" for t, method, n, rect, fma in
                  itertools.product(("double", "float"), (0, 1), (2, 3), ("false", "true"), ("false", "true")))
    assert names == want, set(names) ^ set(want)  # the 32 instantiations and no other kernel
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 128 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]
