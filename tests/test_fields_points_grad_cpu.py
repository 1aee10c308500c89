"""Point-major gradients of a field set (interpn_hip_fields_eval_points_grad_*), the part that needs no GPU: exported and
declared symbols, the statuses returned without a device, the Python argument errors raised before the library is entered,
and the build resources of the fused kernel.

Without a device no set can be made, so of the header's check list only its head (no set: INVALID_ARGUMENT, in front of
everything else) is reachable here; the whole list, in its order, on a live set and host pointers that are never
dereferenced, is tests/test_xi_field_set_jacobian_gpu.py::test_abi_checks_in_their_order."""

import ctypes
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INVALID = 32
SYMBOLS = ["interpn_hip_fields_eval_points_grad_device", "interpn_hip_fields_eval_points_grad_host",
           "interpn_hip_fields_reserve_points_grad"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert f"int {s}(" in header, s
    assert "Point-major gradients of a field set" in header
    import interpn_amd
    from interpn_amd import autograd

    assert "interpn_fields_points_grad" in interpn_amd.__all__ and callable(interpn_amd.interpn_fields_points_grad)
    assert len(interpn_amd.raw.__all__) == 16
    for name in ("eval_points_grad", "eval_points_grad_host", "eval_points_grad_tensors", "reserve_points_grad"):
        assert callable(getattr(interpn_amd.Fields, name)), name
    assert callable(autograd.interp_fields_points)


def test_null_set_comes_first(lib):
    """No set, no device: every entry point answers INVALID_ARGUMENT, whatever else it is given — strides that are too
    small, no points, unknown flags."""
    buf = np.zeros(16)
    p = buf.ctypes.data
    dev = lib.interpn_hip_fields_eval_points_grad_device
    host = lib.interpn_hip_fields_eval_points_grad_host
    assert dev(None, None, 0, 0, None, 0, None, 0, None, 0, None) == INVALID
    assert dev(None, p, 3, 2, p, 2, p, 6, None, 0, None) == INVALID
    assert dev(None, p, 3, 0, p, 2, p, 6, None, 0, None) == INVALID  # in front of npoints == 0
    assert dev(None, p, 3, 2, p, 2, p, 6, None, 6, None) == INVALID  # unknown flags
    assert host(None, None, 0, 0, None, 0, None, 0) == INVALID
    assert host(None, p, 3, 2, p, 2, p, 6) == INVALID
    assert lib.interpn_hip_fields_reserve_points_grad(None, 0, 0) == INVALID
    assert lib.interpn_hip_fields_reserve_points_grad(None, 100, 1) == INVALID
    path = ctypes.c_int(-5)
    assert dev(None, p, 3, 2, p, 2, p, 6, None, 0, ctypes.byref(path)) == INVALID
    assert path.value == 1  # INTERPN_HIP_FIELDS_POINTS_PATH_SPLIT: always set


def test_interpn_fields_points_grad_argument_errors():
    """Everything here is decided before a device is touched."""
    import interpn_amd

    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    xi = np.zeros((3, 2))
    vals = np.zeros((4, 5, 2))
    f = interpn_amd.interpn_fields_points_grad
    with pytest.raises(ValueError, match="Unsupported interpolation configuration"):
        f(xi, grids, vals, method="quintic")
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        f(xi, grids, [[0.0] * 20] * 2)
    with pytest.raises(TypeError, match="xi: expected a numpy array"):
        f([[0.0, 0.0]], grids, vals)
    with pytest.raises(ValueError, match=r"vals: expected shape \(\*dims, K\)"):
        f(xi, grids, np.zeros((4, 5)))
    with pytest.raises(ValueError, match=r"xi: expected shape \(\.\.\., 2\)"):
        f(np.zeros((3, 3)), grids, vals)  # wrong last dimension
    with pytest.raises(ValueError, match="expected 2 x 20 values"):
        f(xi, grids, np.zeros((4, 6, 2)))
    with pytest.raises(TypeError, match="xi: expected dtype float64"):
        f(xi.astype(np.float32), grids, vals)  # the dtype is that of vals
    with pytest.raises(TypeError, match="xi: expected dtype float32"):
        f(xi, grids, vals.astype(np.float32))


def test_fields_eval_points_grad_argument_errors():
    """The checks of Fields.eval_points_grad_host come in front of the library call: a set object without a handle shows
    them.  (The value form does not look for overlapping blocks, and neither does this one.)"""
    import interpn_amd

    fs = interpn_amd.Fields(0, np.float64, 3, 4)  # no handle behind it: nothing below may reach the library
    pts = np.zeros((6, 3))
    g = fs.eval_points_grad
    with pytest.raises(TypeError, match="expected a numpy array"):
        fs.eval_points_grad_host([[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError, match="expected a numpy array"):
        g([[0.0, 0.0, 0.0]])
    with pytest.raises(TypeError, match="expected dtype float64, got float32"):
        g(pts.astype(np.float32))
    with pytest.raises(ValueError, match=r"expected shape \(\.\.\., 3\), got \(6, 4\)"):
        g(np.zeros((6, 4)))
    with pytest.raises(ValueError, match=r"expected shape \(\.\.\., 3\)"):
        g(np.zeros(()))
    with pytest.raises(TypeError, match="out: expected a numpy array of float64"):
        g(pts, np.zeros((6, 4), dtype=np.float32))
    with pytest.raises(TypeError, match="jac: expected a numpy array of float64"):
        g(pts, None, np.zeros((6, 4, 3), dtype=np.float32))
    with pytest.raises(TypeError, match="jac: expected a numpy array of float64"):
        g(pts, None, [[0.0]])
    with pytest.raises(ValueError, match=r"out: expected shape \(6, 4\), got \(4, 6\)"):
        g(pts, np.zeros((4, 6)))
    with pytest.raises(ValueError, match=r"jac: expected shape \(6, 4, 3\), got \(6, 3, 4\)"):
        g(pts, None, np.zeros((6, 3, 4)))
    with pytest.raises(ValueError, match=r"jac: expected shape \(2, 3, 4, 3\)"):
        g(pts.reshape(2, 3, 3), None, np.zeros((6, 4, 3)))
    with pytest.raises(ValueError, match="out: every row must be contiguous"):
        g(pts, np.zeros((6, 8))[:, ::2])  # inner stride 2
    with pytest.raises(ValueError, match="jac: every row must be contiguous"):
        g(pts, None, np.zeros((6, 4, 6))[:, :, ::2])  # inner stride 2
    with pytest.raises(ValueError, match="jac: every row must be contiguous"):
        g(pts, None, np.zeros((6, 4, 4))[:, :, :3])  # fields of a row 4 elements apart: the row is no run of K N
    with pytest.raises(ValueError, match="out: the row stride must be a whole number of elements, at least 4"):
        g(pts, np.zeros(24).reshape(6, 4)[::-1])  # a negative row stride
    with pytest.raises(ValueError, match="jac: the row stride must be a whole number of elements, at least 12"):
        g(pts, None, np.lib.stride_tricks.as_strided(np.zeros(72), shape=(6, 4, 3), strides=(64, 24, 8)))  # jac_stride < K N
    with pytest.raises(ValueError, match="jac: expected a contiguous block"):
        g(pts.reshape(2, 3, 3), None, np.zeros((2, 3, 4, 4))[..., :3])
    ro = np.zeros((6, 4, 3))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        g(pts, None, ro)
    with pytest.raises(TypeError, match="takes no"):
        g(pts, stream=None)
    # wider blocks are views the front end takes as they are
    from interpn_amd import _args

    wide = np.zeros((6, 20))
    assert _args.point_results("jac", wide[:, 1:13].reshape(6, 4, 3), (6,), (4, 3), 6) == 20
    rows, n, stride, lead = _args.point_rows("pts", np.zeros((6, 4))[:, :3], 3)
    assert (n, stride, lead) == (6, 4, (6,)) and rows.shape == (6, 3)
    rows, n, stride, lead = _args.point_rows("pts", np.zeros((2, 3, 3)), 3)
    assert (n, stride, lead) == (6, 3, (2, 3))


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernel_has_no_scratch_and_no_agprs(tmp_path):
    """Every instantiation of the fused kernel — {f64, f32} x N = {2, 3} x {regular, rectilinear}, in both fma flavours —
    exists and keeps its state in VGPRs (the compiler's resource remarks; resource counts only)."""
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_fields_points_grad.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_fields_points_grad.o")],
            stderr=err, cwd=os.path.dirname(src))
    rows = [r for r in parse(str(remarks)) if "k_linear_fields_points_grad<" in r["demangled"]]
    names = {re.search(r"k_linear_fields_points_grad<[^>]*>", r["demangled"]).group(0) for r in rows}
    want = {f"k_linear_fields_points_grad<{t}, {n}, {rect}, {fma}>" for t, n, rect, fma in
            itertools.product(("double", "float"), (2, 3), ("false", "true"), ("false", "true"))}
    assert names == want, names ^ want
    assert len(rows) == len(want) == 16
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 128 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]  # four waves per SIMD at least
