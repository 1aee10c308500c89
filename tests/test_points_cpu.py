"""Point-major observation points (interpn_hip_eval_points_*, interpn_points), the part that needs no GPU: the exported
symbols, the checks made before any device work (host pointers that are never dereferenced), and the fused kernel's build
resources."""

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
OK, INVALID = 0, 32
SYMBOLS = ["interpn_hip_eval_points_device", "interpn_hip_eval_points_host", "interpn_hip_reserve_points"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in header, s
    for name in ("INTERPN_HIP_POINTS_PATH_FUSED", "INTERPN_HIP_POINTS_PATH_SPLIT", "INTERPN_HIP_POINTS_PATH_DIRECT"):
        assert name in header, name
    import interpn_amd

    assert "interpn_points" in interpn_amd.__all__ and callable(interpn_amd.interpn_points)
    for name in ("eval_points_host", "eval_points_tensors", "reserve_points", "last_points_path"):
        assert hasattr(interpn_amd.Interpolator, name), name
    for cls in ("MultilinearRegular", "MultilinearRectilinear", "MulticubicRegular", "MulticubicRectilinear", "NearestRegular",
                "NearestRectilinear"):
        assert hasattr(getattr(interpn_amd, cls), "eval_points"), cls


def test_raw_keeps_the_references_sixteen_names():
    import interpn_amd

    assert len(interpn_amd.raw.__all__) == 16 and not [n for n in interpn_amd.raw.__all__ if "points" in n]


def test_null_handle_is_invalid(lib):
    x = np.zeros((4, 3))
    out = np.zeros(4)
    path = c_int(-5)
    for n in (4, 0):
        assert lib.interpn_hip_eval_points_device(None, c_void_p(x.ctypes.data), 3, n, c_void_p(out.ctypes.data), None, 0, path) == INVALID
        assert lib.interpn_hip_eval_points_host(None, c_void_p(x.ctypes.data), 3, n, c_void_p(out.ctypes.data)) == INVALID
    assert lib.interpn_hip_eval_points_device(None, None, 0, 0, None, None, 0, None) == INVALID
    assert lib.interpn_hip_reserve_points(None, 100, 1) == INVALID
    assert not out.any()


def test_interpn_points_rejects_what_interpn_rejects():
    import interpn_amd

    g = [np.linspace(0.0, 1.0, 4)]
    with pytest.raises(AssertionError):  # dtype rule of interpn(): float32 / float64 only
        interpn_amd.interpn_points(np.zeros((3, 1)), g, np.arange(4))
    with pytest.raises(TypeError):
        interpn_amd.interpn_points(np.zeros((3, 1)), g, [0.0, 1.0, 2.0, 3.0])
    with pytest.raises(AssertionError, match="Dimension mismatch"):  # last axis of xi is not N
        interpn_amd.interpn_points(np.zeros((3, 2)), g, np.arange(4.0))
    with pytest.raises(ValueError):
        interpn_amd.interpn_points(np.zeros((3, 1)), g, np.arange(4.0), method="quintic")


# ---- build resources
@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_no_instantiation_has_scratch_or_agprs(tmp_path):
    """The translation unit itself, as the library builds it: every k_linear_points instantiation the launchers can reach,
    k_split_points and the two one-lane kernels."""
    from tools.kernel_resources import parse

    csrc = os.path.join(ROOT, "interpn_amd", "csrc")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-I", csrc,
             "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
             os.path.join(csrc, "k_linear_points.hip"), "-o", str(tmp_path / "k_linear_points.o")], stderr=err, cwd=csrc)
    rows = parse(str(remarks))
    fused = [r for r in rows if r["demangled"].startswith("void k_linear_points<")]
    # per element type: N = 2 one layout, N = 3 three (f32: and the 2 x 4 x 4 bricks); regular + four rectilinear axis
    # searches; fma and nofma; one and two points per lane
    assert len(fused) == (1 + 3 + 1 + 4) * 5 * 2 * 2, len(fused)
    assert len([r for r in rows if "k_split_points<" in r["demangled"]]) == 2
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    print("k_linear_points VGPRs:", sorted({r["vgpr"] for r in fused}))
