"""Point-major gradients (interpn_hip_eval_points_grad_*, interpn_points_grad, autograd.interp_points), the part that needs
no GPU: the exported symbols, the checks made before any device work (host pointers that are never dereferenced), and the
build resources of the fused kernels against those of the column-form kernels they are made of."""

import os
import shutil
import subprocess
import sys
from ctypes import c_int, c_void_p

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OK, INVALID, UNSUPPORTED = 0, 32, 33
SYMBOLS = ["interpn_hip_eval_points_grad_device", "interpn_hip_eval_points_grad_host", "interpn_hip_reserve_points_grad"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s + "(" in header, s
    import interpn_amd
    from interpn_amd import autograd

    assert "interpn_points_grad" in interpn_amd.__all__ and callable(interpn_amd.interpn_points_grad)
    for name in ("eval_points_grad_host", "eval_points_grad_tensors", "reserve_points_grad", "last_points_path"):
        assert hasattr(interpn_amd.Interpolator, name), name
    for cls in ("MultilinearRegular", "MultilinearRectilinear", "MulticubicRegular", "MulticubicRectilinear"):
        assert hasattr(getattr(interpn_amd, cls), "eval_points_grad"), cls
    for cls in ("NearestRegular", "NearestRectilinear"):
        assert not hasattr(getattr(interpn_amd, cls), "eval_points_grad"), cls
    assert callable(autograd.interp_points) and callable(autograd.interp)


def test_raw_keeps_the_references_sixteen_names():
    import interpn_amd

    assert len(interpn_amd.raw.__all__) == 16 and not [n for n in interpn_amd.raw.__all__ if "points" in n or "grad" in n]


def test_null_handle_is_invalid_before_anything_else(lib):
    """The first check: a NULL handle, whatever the other arguments are (no points, bad strides, NULL grad)."""
    x = np.zeros((4, 3))
    out = np.zeros(4)
    g = np.zeros((4, 3))
    px, po, pg = c_void_p(x.ctypes.data), c_void_p(out.ctypes.data), c_void_p(g.ctypes.data)
    path = c_int(-5)
    for n in (4, 0):
        for stride, gstride in ((3, 3), (0, 3), (3, 0), (1, 1)):
            for grad in (pg, None):
                assert lib.interpn_hip_eval_points_grad_device(None, px, stride, n, po, grad, gstride, None, 0, path) == INVALID
                assert lib.interpn_hip_eval_points_grad_host(None, px, stride, n, po, grad, gstride) == INVALID
    assert lib.interpn_hip_eval_points_grad_device(None, None, 0, 0, None, None, 0, None, 0, None) == INVALID
    assert lib.interpn_hip_reserve_points_grad(None, 100, 1) == INVALID
    assert not out.any() and not g.any()


def test_interpn_points_grad_rejects_what_interpn_points_rejects():
    import interpn_amd

    g = [np.linspace(0.0, 1.0, 4)]
    with pytest.raises(AssertionError):  # dtype rule of interpn(): float32 / float64 only
        interpn_amd.interpn_points_grad(np.zeros((3, 1)), g, np.arange(4))
    with pytest.raises(TypeError):
        interpn_amd.interpn_points_grad(np.zeros((3, 1)), g, [0.0, 1.0, 2.0, 3.0])
    with pytest.raises(AssertionError, match="Dimension mismatch"):  # last axis of xi is not N
        interpn_amd.interpn_points_grad(np.zeros((3, 2)), g, np.arange(4.0))
    with pytest.raises(ValueError):
        interpn_amd.interpn_points_grad(np.zeros((3, 1)), g, np.arange(4.0), method="quintic")
    with pytest.raises(ValueError):  # what interpn_grad rejects: no gradient form
        interpn_amd.interpn_points_grad(np.zeros((3, 1)), g, np.arange(4.0), method="nearest")


# ---- build resources
def _remarks(tmp_path, unit):
    from tools.kernel_resources import parse

    csrc = os.path.join(ROOT, "interpn_amd", "csrc")
    remarks = tmp_path / (unit + ".txt")
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-I", csrc,
             "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
             os.path.join(csrc, unit + ".hip"), "-o", str(tmp_path / (unit + ".o"))], stderr=err, cwd=csrc)
    return parse(str(remarks))


def _params(row, kernel):
    """The template arguments of an instantiation, as one string: "double, 3, false, true, 1, 1, 2, 0, 0"."""
    d = row["demangled"]
    start = d.index(kernel + "<") + len(kernel) + 1
    return d[start:d.index(">", start)]


def _step(vgprs):
    """Waves per SIMD of a kernel with this many VGPRs: 512 registers, allocated in granules of 8, at most 8 waves."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_result_buffers_are_viewed_never_copied():
    """`eval_points_grad` of the classes flattens a caller's `out` and `grad`: what can be flattened without a copy is the
    caller's own memory (a `(..., 4)` buffer cut to 3 columns among it), what cannot is rejected, not copied silently."""
    import torch

    from interpn_amd.classes import _Base

    for zeros in (np.zeros, torch.zeros):
        padded = zeros((5, 7, 4))
        view = _Base._flat_view(padded[..., :3], (-1, 3), "grad")
        assert tuple(view.shape) == (35, 3)
        view[34, 2] = 1.5
        assert float(padded[4, 6, 2]) == 1.5
        assert tuple(_Base._flat_view(zeros((5, 7)), (-1,), "out").shape) == (35,)
        with pytest.raises(ValueError, match="grad: .*without a copy"):
            _Base._flat_view(zeros((5, 7, 3))[:, :2, :], (-1, 3), "grad")
        with pytest.raises(ValueError, match="out: .*without a copy"):
            _Base._flat_view(zeros((5, 7))[:, :2], (-1,), "out")
    assert _Base._flat_view(None, (-1,), "out") is None


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_fused_kernels_have_no_scratch_no_agprs_and_the_column_kernels_occupancy(tmp_path):
    """k_points_grad.hip as the library builds it: every instantiation of the two fused kernels the launchers can reach, and
    k_join_grad, has no scratch and no AGPRs; and none sits on a lower occupancy step than the k_linear_grad / k_cubic_grad
    instantiation with the same template arguments."""
    rows = _remarks(tmp_path, "k_points_grad")
    linear = [r for r in rows if r["demangled"].startswith("void k_linear_points_grad<")]
    cubic = [r for r in rows if r["demangled"].startswith("void k_cubic_points_grad<")]
    # multilinear, per element type: N = 2 one layout, N = 3 three (f32: and the 2 x 4 x 4 bricks); regular + four
    # rectilinear axis searches; fma and nofma; one and two points per lane
    assert len(linear) == (1 + 3 + 1 + 4) * 5 * 2 * 2, len(linear)
    # multicubic: two element types, N = 2, 3, regular and rectilinear, fma and nofma, five tile layouts
    assert len(cubic) == 2 * 2 * 2 * 2 * 5, len(cubic)
    assert len([r for r in rows if "k_join_grad<" in r["demangled"]]) == 2
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    column = {}
    for unit, kernel in (("k_linear_grad", "k_linear_grad"), ("k_cubic_grad", "k_cubic_grad")):
        for r in _remarks(tmp_path, unit):
            if r["demangled"].startswith("void " + kernel + "<"):
                column[(kernel, _params(r, kernel))] = r["vgpr"]
    crossed = []
    for new_rows, kernel, base in ((linear, "k_linear_points_grad", "k_linear_grad"), (cubic, "k_cubic_points_grad", "k_cubic_grad")):
        for r in new_rows:
            want = column[(base, _params(r, kernel))]  # KeyError: an instantiation the column form does not have
            if _step(r["vgpr"]) < _step(want):
                crossed.append((r["demangled"], r["vgpr"], want))
    print("k_linear_points_grad VGPRs:", min(r["vgpr"] for r in linear), "..", max(r["vgpr"] for r in linear))
    print("k_cubic_points_grad VGPRs:", min(r["vgpr"] for r in cubic), "..", max(r["vgpr"] for r in cubic))
    assert not crossed, crossed
