"""Lattice evaluation (interpn_hip_eval_lattice_*, interpn_hip_lattice_plan), the part that needs no GPU: exported symbols,
the path verdict and its LDS boundary, the point count, argument errors decided before any device work, the closed formula
of the first failing index against a brute-force scan, and the row kernel's build resources."""

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
WAVES = 4            # rows in flight (= LDS lines) per workgroup of the row kernel
DEFAULT_CUS = 256    # the device interpn_hip_lattice_plan assumes
DEFAULT_LDS_PER_CU = 160 * 1024

SYMBOLS = ["interpn_hip_eval_lattice_device", "interpn_hip_eval_lattice_host", "interpn_hip_lattice_plan",
           "interpn_hip_reserve_lattice"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for name in ("INTERPN_HIP_AXIS_LDS_KB", "INTERPN_HIP_LATTICE", "INTERPN_HIP_FORCE_GENERIC"):
        monkeypatch.delenv(name, raising=False)


def _plan(lib, elem, method, dims, lens):
    d = (c_size_t * max(len(dims), 1))(*[int(v) for v in dims])
    m = (c_size_t * max(len(lens), 1))(*[int(v) for v in lens])
    path, lds, npts = c_int(-1), c_size_t(0), c_size_t(0)
    st = lib.interpn_hip_lattice_plan(elem, method, len(dims), d, m, ctypes.byref(path), ctypes.byref(lds), ctypes.byref(npts))
    return st, path.value, lds.value, npts.value


def _line(n_last, elem):
    return (n_last * elem + 15) // 16 * 16


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in header, s
    for name in ("INTERPN_HIP_LATTICE_PATH_FUSED", "INTERPN_HIP_LATTICE_PATH_EXPANDED", "Lattice evaluation"):
        assert name in header, name
    import interpn_amd

    for name in ("interpn_lattice", "lattice_plan"):
        assert name in interpn_amd.__all__ and hasattr(interpn_amd, name)
    for name in ("eval_lattice_host", "eval_lattice_tensors", "reserve_lattice", "last_lattice_path"):
        assert hasattr(interpn_amd.Interpolator, name), name
    for cls in ("MultilinearRegular", "MultilinearRectilinear", "MulticubicRegular", "MulticubicRectilinear", "NearestRegular",
                "NearestRectilinear"):
        assert hasattr(getattr(interpn_amd, cls), "eval_lattice"), cls


@pytest.mark.parametrize("elem", [8, 4])
def test_plan_verdict_for_every_method_and_dimension(lib, elem):
    for method, n in itertools.product((LINEAR, CUBIC, NEAREST), range(1, 9)):
        if method == NEAREST and n > 6:
            continue
        dims = [6] * n
        lens = [40] * n if n <= 3 else [3] * n  # N = 2: 40 rows only, see below
        if n == 2:
            lens = [2000, 40]
        st, path, lds, npts = _plan(lib, elem, method, dims, lens)
        assert st == OK
        covered = method in (LINEAR, CUBIC) and n in (2, 3)
        assert path == (FUSED if covered else EXPANDED), (method, n)
        assert lds == (WAVES * _line(6, elem) if covered else 0)
        assert npts == int(np.prod(lens, dtype=object))


def test_plan_automatic_rules(lib):
    # a row for every wave of the device
    rows_min = WAVES * DEFAULT_CUS
    assert _plan(lib, 8, LINEAR, [64, 64], [rows_min, 100])[1] == FUSED
    assert _plan(lib, 8, LINEAR, [64, 64], [rows_min - 1, 100])[1] == EXPANDED
    assert _plan(lib, 8, CUBIC, [64, 64, 64], [32, 32, 100])[1] == FUSED
    assert _plan(lib, 8, CUBIC, [64, 64, 64], [32, 31, 100])[1] == EXPANDED
    # the last grid axis against the last lattice axis: n <= 4 max(m, 64)
    assert _plan(lib, 8, LINEAR, [64, 64, 256], [64, 64, 1])[1] == FUSED
    assert _plan(lib, 8, LINEAR, [64, 64, 257], [64, 64, 1])[1] == EXPANDED
    assert _plan(lib, 8, LINEAR, [64, 64, 400], [64, 64, 100])[1] == FUSED
    assert _plan(lib, 8, LINEAR, [64, 64, 401], [64, 64, 100])[1] == EXPANDED
    # a grid that 32 bits do not index goes through the handle's own kernels
    assert _plan(lib, 4, LINEAR, [70000, 70000], [5000, 5000])[1] == EXPANDED


def test_plan_honours_the_lattice_option(lib, monkeypatch):
    few_rows = ([64, 64, 64], [4, 4, 100])
    assert _plan(lib, 8, LINEAR, *few_rows)[1] == EXPANDED
    monkeypatch.setenv("INTERPN_HIP_LATTICE", "1")
    assert _plan(lib, 8, LINEAR, *few_rows)[1] == FUSED
    assert _plan(lib, 8, NEAREST, *few_rows)[1] == EXPANDED
    monkeypatch.setenv("INTERPN_HIP_LATTICE", "0")
    assert _plan(lib, 8, LINEAR, [64, 64, 64], [464, 464, 464])[1:3] == (EXPANDED, 0)
    monkeypatch.delenv("INTERPN_HIP_LATTICE")
    monkeypatch.setenv("INTERPN_HIP_FORCE_GENERIC", "1")
    assert _plan(lib, 8, LINEAR, [64, 64, 64], [464, 464, 464])[1] == EXPANDED


@pytest.mark.parametrize("elem", [8, 4])
@pytest.mark.parametrize("kb", [None, 1, 7, 60])
def test_plan_lds_boundary(lib, monkeypatch, elem, kb):
    """Four lines of n_{N-1} elements against the budget of rectilinear axis images: axis_lds_kb KiB, by default an eighth
    of a CU's LDS."""
    if kb is None:
        budget = DEFAULT_LDS_PER_CU // 8
    else:
        monkeypatch.setenv("INTERPN_HIP_AXIS_LDS_KB", str(kb))
        budget = kb * 1024
    inside = budget // (WAVES * elem)
    lens = [64, 64, 20000]
    for method, lo in ((LINEAR, 2), (CUBIC, 4)):
        st, path, lds, _ = _plan(lib, elem, method, [lo, lo, inside], lens)
        assert (st, path, lds) == (OK, FUSED, WAVES * _line(inside, elem)) and lds <= budget
        st, path, lds, _ = _plan(lib, elem, method, [lo, lo, inside + 1], lens)
        assert (st, path, lds) == (OK, EXPANDED, 0)
        assert WAVES * _line(inside + 1, elem) > budget
        st, path, lds, _ = _plan(lib, elem, method, [lo + 1, inside], [5000, 20000])
        assert (st, path) == (OK, FUSED)
        assert _plan(lib, elem, method, [lo + 1, inside + 1], [5000, 20000])[1] == EXPANDED


def test_plan_point_count_and_argument_errors(lib):
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [3, 0, 9])[0::3] == (OK, 0)
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [3, 0, 9])[1] == EXPANDED
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [2**31, 2**31, 2])[0] == UNSUPPORTED  # more than 2^31 axis coordinates in all
    assert _plan(lib, 8, LINEAR, [5] * 8, [2**8] * 8)[0] == INVALID               # 2^64 points
    assert _plan(lib, 8, LINEAR, [5] * 8, [2**8] * 7 + [2**7])[0::3] == (OK, 2**63)
    assert _plan(lib, 8, LINEAR, [5, 6, 7], [2**21, 2**21, 2**21])[0::3] == (OK, 2**63)
    assert _plan(lib, 2, LINEAR, [5, 6], [3, 3])[0] == INVALID
    assert _plan(lib, 8, 7, [5, 6], [3, 3])[0] == INVALID
    assert _plan(lib, 8, LINEAR, [5, 1], [3, 3])[0] == INVALID
    assert _plan(lib, 8, CUBIC, [5, 3], [3, 3])[0] == INVALID
    assert _plan(lib, 8, CUBIC, [5, 4], [3, 3])[0] == OK
    assert _plan(lib, 4, LINEAR, [5, 2**24 + 1], [3, 3])[0] == UNSUPPORTED
    d = (c_size_t * 2)(5, 6)
    assert lib.interpn_hip_lattice_plan(8, LINEAR, 2, None, d, None, None, None) == INVALID
    assert lib.interpn_hip_lattice_plan(8, LINEAR, 2, d, None, None, None, None) == INVALID
    assert lib.interpn_hip_lattice_plan(8, LINEAR, 0, d, d, None, None, None) == INVALID
    assert lib.interpn_hip_lattice_plan(8, LINEAR, 9, d, d, None, None, None) == INVALID
    assert lib.interpn_hip_lattice_plan(8, LINEAR, 2, d, d, None, None, None) == OK  # every output is optional


def test_null_arguments(lib):
    lens = (c_size_t * 2)(3, 3)
    ptrs = (c_void_p * 2)()
    path = c_int(-7)
    assert lib.interpn_hip_eval_lattice_device(None, ptrs, lens, 2, None, None, 0, ctypes.byref(path)) == INVALID
    assert path.value == EXPANDED
    assert lib.interpn_hip_eval_lattice_device(None, ptrs, lens, 2, None, None, 2, None) == INVALID  # unknown flag
    assert lib.interpn_hip_eval_lattice_host(None, ptrs, lens, 2, None, None) == INVALID
    assert lib.interpn_hip_reserve_lattice(None, lens, 2, 1) == INVALID


def test_python_argument_errors():
    """Decided before a device is touched: a handle-less Interpolator is enough."""
    import interpn_amd

    it = interpn_amd.Interpolator(0, np.float64, 3)
    axes = [np.zeros(3), np.zeros(4), np.zeros(5)]
    with pytest.raises(TypeError, match=r"axes\[1\].*expected dtype float64"):
        it.eval_lattice_host([axes[0], axes[1].astype(np.float32), axes[2]])
    with pytest.raises(TypeError, match=r"axes\[2\].*1-D"):
        it.eval_lattice_host([axes[0], axes[1], np.zeros((5, 1))])
    with pytest.raises(TypeError, match="numpy array"):
        it.eval_lattice_host([axes[0], axes[1], [0.0] * 5])
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 4, 5\)"):
        it.eval_lattice_host(axes, np.zeros((3, 5, 4)))
    with pytest.raises(TypeError, match="argument 'out': expected dtype float64"):
        it.eval_lattice_host(axes, np.zeros((3, 4, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="not contiguous"):
        it.eval_lattice_host(axes, np.zeros((3, 4, 10))[:, :, ::2])
    with pytest.raises(ValueError):  # the null handle itself: INTERPN_HIP_ERR_INVALID_ARGUMENT
        it.eval_lattice_host(axes)
    with pytest.raises(TypeError, match=r"axes\[0\]: expected a contiguous 1-D"):
        it.eval_lattice_tensors(axes)

    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    vals = np.zeros((4, 5))
    ax2 = [np.zeros(3), np.zeros(6)]
    with pytest.raises(ValueError, match="Unsupported interpolation configuration"):
        interpn_amd.interpn_lattice(ax2, grids, vals, method="quintic")
    with pytest.raises(ValueError, match="expected 2 coordinate vectors"):
        interpn_amd.interpn_lattice(ax2[:1], grids, vals)
    with pytest.raises(AssertionError, match="float32 and float64"):
        interpn_amd.interpn_lattice(ax2, grids, vals.astype(np.int32))
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        interpn_amd.interpn_lattice(ax2, grids, [[0.0] * 5] * 4)
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 6\)"):
        interpn_amd.interpn_lattice(ax2, grids, vals, out=np.zeros((6, 3)))
    with pytest.raises(ValueError, match="expected 2 lengths"):
        interpn_amd.lattice_plan(np.float64, "linear", [4, 5], [3])
    assert interpn_amd.lattice_plan(np.float32, "cubic", [4, 5], [3000, 7]) == ("fused", 4 * 32, 21000)


def _first_bad_formula(lens, bad):
    """min over bad (d, j) of j * prod(lens[e], e > d) — what k_lattice_axes reports."""
    return min(j * int(np.prod(lens[d + 1:], dtype=object)) for d, j in bad)


def test_first_bad_formula_against_a_scan():
    """The reference's loop walks the expanded lattice in C order and stops at the first point with a bad coordinate."""
    rng = np.random.default_rng(5)
    for trial in range(200):
        n = int(rng.integers(1, 5))
        lens = [int(v) for v in rng.integers(1, 8, n)]
        nbad = int(rng.integers(1, 4))
        bad = []
        for _ in range(nbad):
            d = int(rng.integers(0, n))
            bad.append((d, int(rng.integers(0, lens[d]))))
        axes = [np.zeros(m) for m in lens]
        for d, j in bad:
            axes[d][j] = np.nan
        mesh = np.meshgrid(*axes, indexing="ij")
        failing = np.zeros(lens, dtype=bool)
        for m in mesh:
            failing |= np.isnan(m)
        assert int(np.flatnonzero(failing.ravel())[0]) == _first_bad_formula(lens, bad), (lens, bad)


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_row_kernel_has_no_scratch_and_no_agprs(tmp_path):
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_lattice.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_lattice.o")],
            stderr=err, cwd=os.path.dirname(src))
    rows = [r for r in parse(str(remarks)) if "k_lattice_rows<" in r["demangled"]]
    names = {r["demangled"].split("(")[0].replace("void ", "") for r in rows}
    want = {f"k_lattice_rows<{t}, {method}, {n}, {rect}, {fma}>" for t, method, n, rect, fma in
            itertools.product(("double", "float"), (0, 1), (2, 3), ("false", "true"), ("false", "true"))}
    assert names == want, names ^ want
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 128 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]  # four waves per SIMD at least
    others = [r for r in parse(str(remarks)) if any(k in r["demangled"] for k in ("k_lattice_axes<", "k_lattice_check<", "k_lattice_expand<"))]
    assert len(others) == 16 + 2 + 2 and all(r["scratch"] == 0 and r["agpr"] == 0 for r in others)
