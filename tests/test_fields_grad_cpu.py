"""Gradients of a field set (interpn_hip_fields_eval_grad_*), the part that needs no GPU: exported and declared symbols, the
statuses returned without a device, the Python argument errors raised before the library is entered, and the build resources
of the fused kernel."""

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
SYMBOLS = ["interpn_hip_fields_eval_grad_device", "interpn_hip_fields_eval_grad_host"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert f"int {s}(" in header, s
    assert "Gradients of a field set" in header
    import interpn_amd
    from interpn_amd import autograd

    assert "interpn_fields_grad" in interpn_amd.__all__ and callable(interpn_amd.interpn_fields_grad)
    for name in ("eval_grad", "eval_grad_host", "eval_grad_tensors", "eval_grad_device_ptrs"):
        assert callable(getattr(interpn_amd.Fields, name)), name
    assert callable(autograd.interp_fields)


def test_null_set_and_flags(lib):
    """No set, no device: both entry points answer INVALID_ARGUMENT, whatever else they are given."""
    import ctypes

    buf = np.zeros(16)
    p = buf.ctypes.data
    assert lib.interpn_hip_fields_eval_grad_device(None, None, 0, None, 0, None, 0, 0, None, 0, None) == INVALID
    assert lib.interpn_hip_fields_eval_grad_device(None, None, 0, p, 4, p, 4, 4, None, 0, None) == INVALID
    assert lib.interpn_hip_fields_eval_grad_device(None, None, 0, p, 4, p, 4, 4, None, 6, None) == INVALID  # unknown flags
    assert lib.interpn_hip_fields_eval_grad_host(None, None, None, 0, None, 0, None, 0, 0) == INVALID
    assert lib.interpn_hip_fields_eval_grad_host(None, None, None, 0, p, 4, p, 4, 4) == INVALID
    path = ctypes.c_int(-5)
    assert lib.interpn_hip_fields_eval_grad_device(None, None, 0, p, 4, p, 4, 4, None, 0, ctypes.byref(path)) == INVALID
    assert path.value == 1  # INTERPN_HIP_FIELDS_PATH_PER_FIELD: always set


def test_python_argument_errors():
    """The checks of Fields.eval_grad_host and of interpn_fields_grad come in front of the library call."""
    import interpn_amd

    fs = interpn_amd.Fields(0, np.float64, 2, 3)  # no handle behind it: nothing below may reach the library
    obs = [np.zeros(10), np.zeros(10)]
    with pytest.raises(ValueError, match=r"out: expected a \(3, 10\) array of float64"):
        fs.eval_grad_host(obs, np.zeros((10, 3)))
    with pytest.raises(ValueError, match=r"grad: expected a \(3, 2, 10\) array of float64"):
        fs.eval_grad_host(obs, None, np.zeros((3, 10, 2)))
    with pytest.raises(ValueError, match=r"grad: expected a \(3, 2, 10\) array of float64"):
        fs.eval_grad_host(obs, None, np.zeros((3, 2, 10), dtype=np.float32))
    with pytest.raises(ValueError, match="out: rows must be contiguous"):
        fs.eval_grad_host(obs, np.zeros((3, 20))[:, ::2])
    with pytest.raises(ValueError, match="grad: the last axis must be contiguous"):
        fs.eval_grad_host(obs, None, np.zeros((3, 2, 20))[:, :, ::2])
    with pytest.raises(ValueError, match="grad: one uniform stride of at least 10 elements"):
        fs.eval_grad_host(obs, None, np.zeros((3, 3, 10))[:, :2])
    with pytest.raises(ValueError, match="grad: one uniform stride of at least 10 elements"):
        fs.eval_grad_host(obs, None, np.zeros((6, 10)).reshape(3, 2, 10)[:, ::-1])  # rows going backwards
    ro = np.zeros((3, 2, 10))
    ro.flags.writeable = False
    with pytest.raises(ValueError, match="read-only"):
        fs.eval_grad_host(obs, None, ro)
    with pytest.raises(TypeError, match="takes no"):
        fs.eval_grad(obs, stream=None)
    grids = [np.linspace(0.0, 1.0, 4), np.linspace(0.0, 1.0, 5)]
    f = interpn_amd.interpn_fields_grad
    with pytest.raises(ValueError, match="field_axis"):
        f(obs, grids, np.zeros((3, 4, 5)), field_axis=1)
    with pytest.raises(ValueError, match="Unsupported interpolation configuration"):
        f(obs, grids, np.zeros((3, 4, 5)), method="quintic")
    with pytest.raises(TypeError, match="numpy array or a torch tensor"):
        f(obs, grids, [[0.0] * 20] * 3)
    with pytest.raises(ValueError, match="expected a field axis"):
        f(obs, grids, np.zeros(20))
    with pytest.raises(ValueError, match="expected 3 x 20 values"):
        f(obs, grids, np.zeros((3, 4, 6)))


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_kernel_has_no_scratch_and_no_agprs(tmp_path):
    """Every instantiation of the fused kernel — {f64, f32} x N = {2, 3} x {regular, rectilinear}, in both fma flavours —
    exists and keeps its state in VGPRs (the compiler's resource remarks; resource counts only)."""
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_linear_fields_grad.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_linear_fields_grad.o")],
            stderr=err, cwd=os.path.dirname(src))
    rows = [r for r in parse(str(remarks)) if "k_linear_fields_grad<" in r["demangled"]]
    names = {re.search(r"k_linear_fields_grad<[^>]*>", r["demangled"]).group(0) for r in rows}
    want = {f"k_linear_fields_grad<{t}, {n}, {rect}, {fma}>" for t, n, rect, fma in
            itertools.product(("double", "float"), (2, 3), ("false", "true"), ("false", "true"))}
    assert names == want, names ^ want
    assert len(rows) == len(want)
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    assert all(0 < r["vgpr"] <= 256 for r in rows), [(r["demangled"], r["vgpr"]) for r in rows]  # two waves per SIMD at least
