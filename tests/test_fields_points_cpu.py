"""Point-major field sets (interpn_hip_fields_eval_points_*), the part that needs no GPU: exported symbols, the statuses
that are returned without a device, the Python argument errors that are raised before the library is entered, and the
build resources of the fused kernel and of the split path's join."""

import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INVALID = 32
SYMBOLS = ["interpn_hip_fields_eval_points_device", "interpn_hip_fields_eval_points_host", "interpn_hip_fields_reserve_points"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert f"int {s}(" in header, s
    assert "INTERPN_HIP_FIELDS_POINTS_PATH_FUSED = 0, INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT = 1" in header
    import interpn_amd

    assert "interpn_fields_points" in interpn_amd.__all__ and callable(interpn_amd.interpn_fields_points)
    for name in ("eval_points", "eval_points_host", "eval_points_tensors", "reserve_points"):
        assert callable(getattr(interpn_amd.Fields, name)), name
    assert interpn_amd._lib.FIELDS_POINTS_PATHS == {0: "fused", 1: "split"}


def test_null_set_and_flags(lib):
    """No set, no device: every entry point answers INVALID_ARGUMENT, whatever else it is given."""
    buf = np.zeros(16)
    p = buf.ctypes.data
    assert lib.interpn_hip_fields_eval_points_device(None, None, 0, 0, None, 0, None, 0, None) == INVALID
    assert lib.interpn_hip_fields_eval_points_device(None, p, 3, 2, p, 2, None, 0, None) == INVALID
    assert lib.interpn_hip_fields_eval_points_device(None, p, 3, 0, p, 2, None, 0, None) == INVALID  # in front of npoints == 0
    assert lib.interpn_hip_fields_eval_points_device(None, p, 3, 2, p, 2, None, 6, None) == INVALID  # unknown flags
    assert lib.interpn_hip_fields_eval_points_host(None, None, 0, 0, None, 0) == INVALID
    assert lib.interpn_hip_fields_eval_points_host(None, p, 3, 2, p, 2) == INVALID
    assert lib.interpn_hip_fields_reserve_points(None, 0, 0) == INVALID
    assert lib.interpn_hip_fields_reserve_points(None, 100, 1) == INVALID
    import ctypes

    path = ctypes.c_int(-5)
    assert lib.interpn_hip_fields_eval_points_device(None, p, 3, 2, p, 2, None, 0, ctypes.byref(path)) == INVALID
    assert path.value == 1  # INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT: always set


def test_interpn_fields_points_argument_errors():
    """Everything here is decided before a device is touched."""
    import interpn_amd

    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    xi = np.zeros((3, 2))
    vals = np.zeros((4, 5, 2))
    f = interpn_amd.interpn_fields_points
    with pytest.raises(ValueError, match="Unsupported interpolation configuration"):
        f(xi, grids, vals, method="quintic")
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        f(xi, grids, [[0.0] * 20] * 2)
    with pytest.raises(AssertionError, match="float32 and float64"):
        f(xi, grids, np.zeros((4, 5, 2), dtype=np.int32))
    with pytest.raises(TypeError, match="xi: expected a numpy array"):
        f([[0.0, 0.0]], grids, vals)
    with pytest.raises(ValueError, match=r"vals: expected shape \(\*dims, K\)"):
        f(xi, grids, np.zeros((4, 5)))
    with pytest.raises(ValueError, match=r"xi: expected shape \(\.\.\., 2\)"):
        f(np.zeros((3, 3)), grids, vals)  # wrong last axis
    with pytest.raises(ValueError, match=r"xi: expected shape \(\.\.\., 2\)"):
        f(np.zeros(()), grids, vals)
    with pytest.raises(ValueError, match="expected 2 x 20 values"):
        f(xi, grids, np.zeros((4, 6, 2)))
    with pytest.raises(TypeError, match="xi: expected dtype float64"):
        f(xi.astype(np.float32), grids, vals)  # the dtype is that of vals
    with pytest.raises(TypeError, match="xi: expected dtype float32"):
        f(xi, grids, vals.astype(np.float32))
    with pytest.raises(ValueError, match=r"out: expected shape \(3, 2\)"):
        f(xi, grids, vals, out=np.zeros((2, 3)))
    with pytest.raises(ValueError, match=r"out: expected shape \(5, 7, 2\)"):
        f(np.zeros((5, 7, 2)), grids, vals, out=np.zeros((35, 2)))


def test_fields_eval_points_argument_errors():
    """The checks of Fields.eval_points_host come in front of the library call: a set object without a handle shows them."""
    import interpn_amd

    fs = interpn_amd.Fields(0, np.float64, 3, 4)  # no handle behind it: nothing below may reach the library
    pts = np.zeros((6, 3))
    with pytest.raises(TypeError, match="expected a numpy array"):
        fs.eval_points_host([[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError, match="expected a numpy array"):
        fs.eval_points([[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError, match="expected dtype float64, got float32"):
        fs.eval_points(pts.astype(np.float32))
    with pytest.raises(ValueError, match=r"expected shape \(\.\.\., 3\), got \(6, 4\)"):
        fs.eval_points(np.zeros((6, 4)))
    with pytest.raises(ValueError, match=r"expected shape \(\.\.\., 3\)"):
        fs.eval_points(np.zeros(()))
    with pytest.raises(TypeError, match="out: expected a numpy array of float64"):
        fs.eval_points(pts, np.zeros((6, 4), dtype=np.float32))
    with pytest.raises(ValueError, match=r"out: expected shape \(6, 4\), got \(4, 6\)"):
        fs.eval_points(pts, np.zeros((4, 6)))
    with pytest.raises(ValueError, match=r"out: expected shape \(2, 3, 4\)"):
        fs.eval_points(pts.reshape(2, 3, 3), np.zeros((6, 4)))
    with pytest.raises(ValueError, match="every row must be contiguous"):
        fs.eval_points(pts, np.zeros((6, 8))[:, ::2])  # non-unit stride along the last axis
    with pytest.raises(ValueError, match="row stride must be a whole number of elements, at least 4"):
        fs.eval_points(pts, np.zeros(24).reshape(6, 4)[::-1])  # a negative row stride: rows would overlap going backwards
    with pytest.raises(ValueError, match="row stride must be a whole number of elements, at least 4"):
        fs.eval_points(pts, np.lib.stride_tricks.as_strided(np.zeros(24), shape=(6, 4), strides=(16, 8)))  # out_stride < K
    with pytest.raises(ValueError, match="C-contiguous"):
        fs.eval_points(pts.reshape(2, 3, 3), np.zeros((2, 3, 8))[:, :, :4])
    ro = np.zeros((6, 4))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        fs.eval_points(pts, ro)
    with pytest.raises(TypeError, match="takes no"):
        fs.eval_points(pts, stream=None)


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernels_have_no_scratch_and_no_agprs(tmp_path):
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_fields_points.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_fields_points.o")],
            stderr=err, cwd=os.path.dirname(src))
    rows = [r for r in parse(str(remarks)) if "k_linear_fields_points<" in r["demangled"]]
    names = {r["demangled"].split("(")[0].replace("void ", "") for r in rows}
    want = {f"k_linear_fields_points<{t}, {n}, {rect}, {fma}>" for t, n, rect, fma in
            itertools.product(("double", "float"), (2, 3), ("false", "true"), ("false", "true"))}
    assert names == want, names ^ want
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 128 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]  # four waves per SIMD at least
    join = [r for r in parse(str(remarks)) if "k_join_fields<" in r["demangled"]]
    assert {r["demangled"].split("(")[0].replace("void ", "") for r in join} == {"k_join_fields<double>", "k_join_fields<float>"}
    assert all(r["scratch"] == 0 and r["agpr"] == 0 for r in join), join
