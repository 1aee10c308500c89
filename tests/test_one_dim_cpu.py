"""interpn::one_dim without a GPU: the status strings, the creators' validation (all of it runs before any device
work), the CPU restatement (tests/one_dim_restatement.py) against hand-derived answers, and the new kernels' resources."""

import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import one_dim_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_strerror_of_the_new_statuses():
    from interpn_amd import _lib

    assert _lib.strerror(11) == "Length mismatch"             # one_dim/mod.rs:53, :150
    assert _lib.strerror(12) == "Unrepresentable number"      # one_dim/mod.rs:111
    assert _lib.strerror(7) == "Unrepresentable coordinate value"  # unchanged


def test_validation_before_device_work():
    """Every check below fails before a device is touched (this machine may have none)."""
    from interpn_amd import Interpolator, _lib, one_dim

    lib = _lib.load()
    with pytest.raises(AssertionError, match="^Length mismatch$"):
        Interpolator.grid1d_rectilinear("Linear1D", np.array([0.0, 1.0, 2.0]), np.array([1.0, 2.0]))
    with pytest.raises(AssertionError, match="^Length mismatch$"):  # fewer than 2 entries
        Interpolator.grid1d_rectilinear("Left1D", np.array([0.0]), np.array([1.0]))
    with pytest.raises(AssertionError, match="^Length mismatch$"):
        one_dim.RectilinearGrid1D(np.array([0.0, 1.0]), np.array([1.0, 2.0, 3.0]))
    for n in (0, 1):  # the reference panics (in `new` for an empty slice, at the first point for one value)
        with pytest.raises(_lib.ReferencePanic):
            Interpolator.grid1d_regular("Nearest1D", 0.0, 1.0, np.zeros(n))
        with pytest.raises(_lib.ReferencePanic):
            one_dim.Right1D(one_dim.RegularGrid1D(0.0, 1.0, np.zeros(n)))
    # method codes of the multidimensional creators are not one_dim's and vice versa
    h = __import__("ctypes").c_void_p()
    vals = np.zeros(4)
    p = vals.ctypes.data_as(__import__("ctypes").c_void_p)
    assert lib.interpn_hip_create_grid1d_regular_f64(_lib.LINEAR, 0.0, 1.0, p, 4, 0, -1, __import__("ctypes").byref(h)) == 32
    assert lib.interpn_hip_create_grid1d_regular_f64(16 | 0x300, 0.0, 1.0, p, 4, 0, -1, __import__("ctypes").byref(h)) == 32
    assert lib.interpn_hip_create_grid1d_regular_f64(16, 0.0, 1.0, p, 4, 7, -1, __import__("ctypes").byref(h)) == 32


def test_restatement_known_answers():
    vals = np.array([1.0, 2.0, 4.0])
    ev = lambda m, x, **k: R.eval(m, "regular", np.float64, True, np.array(x, dtype=np.float64), start=0.0, step=1.0,
                                  vals=vals, **k)[0]
    x = [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0]
    assert ev("Linear1D", x).tolist() == [0.0, 1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0]
    assert ev("LinearHoldLast1D", x).tolist() == [1.0, 1.0, 1.5, 2.0, 3.0, 4.0, 4.0, 4.0]
    # Left: y0 of the clamped cell unless above stop; Right: y1 unless below start
    assert ev("Left1D", x).tolist() == [1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 4.0, 4.0]
    assert ev("Right1D", x).tolist() == [1.0, 2.0, 2.0, 4.0, 4.0, 4.0, 4.0, 4.0]
    # Nearest1D: an exact tie (0.5, 1.5) goes left
    assert ev("Nearest1D", x).tolist() == [1.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 4.0]


def test_restatement_rectilinear_traps():
    g = np.array([0.0, 1.0, 3.0])
    vals = np.array([1.0, 2.0, 4.0])
    x = np.array([np.nan, np.inf, -np.inf])
    out = {m: R.eval(m, "rectilinear", np.float64, True, x, grid=g, vals=vals)[0] for m in R.METHODS}
    assert out["Left1D"].tolist()[:2] == [1.0, 4.0]      # NaN: vals[0]; +inf: vals[n-1]
    assert out["Right1D"].tolist()[0] == 2.0             # NaN: vals[1]
    assert out["Nearest1D"].tolist()[0] == 2.0           # NaN goes right
    assert np.isnan(out["Linear1D"][0]) and np.isnan(out["LinearHoldLast1D"][0])
    assert out["LinearHoldLast1D"][1] == 4.0 and out["LinearHoldLast1D"][2] == 1.0
    # unsorted axis: std's probe sequence decides (size 5: g[2], g[3], g[3], then the final compare at base); by hand:
    # x = 1.5: 1 < x -> base 2; 2 < x no; 2 < x no; g[2] = 1 < x -> 3
    gu = np.array([0.0, 5.0, 1.0, 2.0, 9.0])
    assert R.partition_point_lt(gu, np.array([1.5])).tolist() == [3]
    assert R.partition_point_lt(gu, np.array([0.5])).tolist() == [1]
    assert R.partition_point_lt(gu, np.array([6.0])).tolist() == [4]
    # OutsideLow on an unsorted axis does not mean cell 0: x = 1.5 < g[0] = 2, yet the search ends at 3 -> cell 1
    gd = np.array([2.0, 0.0, 1.0])
    i, ext, *_ = R.grid_at("rectilinear", np.float64, np.array([1.5]), grid=gd, vals=vals)
    assert ext.tolist() == [R.LOW] and i.tolist() == [1]
    assert R.eval("Left1D", "rectilinear", np.float64, True, np.array([1.5]), grid=gd, vals=vals)[0].tolist() == [2.0]


def test_restatement_regular_traps():
    vals = np.array([1.0, 2.0, 4.0])
    for bad in (np.nan, np.inf, -np.inf, 1e300):
        out, fb = R.eval("Left1D", "regular", np.float64, True, np.array([0.5, bad, 0.5]), start=0.0, step=1.0, vals=vals)
        assert fb == 1 and out[0] == 1.0
    # a negative step: stop = -2 < start = 0; OutsideHigh (x > stop) is tested first, so every x > -2 is high, even
    # x = -1.5 between the two; x = 1 is high with cell floor((1 - 0) / -1) = -1 -> 0 (not n - 2), x = -3 is low with
    # cell floor(3) -> n - 2 (not 0)
    i, ext, *_ = R.grid_at("regular", np.float64, np.array([1.0, -3.0, -1.5]), start=0.0, step=-1.0, vals=vals)
    assert ext.tolist() == [R.HIGH, R.LOW, R.HIGH] and i.tolist() == [0, 1, 1]
    assert R.eval("Left1D", "regular", np.float64, True, np.array([1.0]), start=0.0, step=-1.0, vals=vals)[0].tolist() == [2.0]
    # NaN step: every point fails
    assert R.eval("Right1D", "regular", np.float64, True, np.array([0.0]), start=0.0, step=np.nan, vals=vals)[1] == 0
    # stop overflows to inf: nothing is OutsideHigh
    big = np.finfo(np.float64).max / 2
    assert np.isinf(R.regular_stop(big, big, 3, np.float64))
    # f32: T(n - 1) rounds once n - 1 exceeds 2^24
    assert R.regular_stop(np.float32(0), np.float32(1), 2**24 + 2, np.float32) == np.float32(2**24)


@pytest.mark.parametrize("method", ["Linear1D", "LinearHoldLast1D"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_sites_differ_in_the_last_bit(method, dtype):
    """one_dim/linear.rs:34 (Linear1D) and :76 (LinearHoldLast1D, inside): slope.mul_add(dx, y0) under `fma`,
    y0 + slope * dx without; a point where the two differ, each checked against exact rational arithmetic."""
    T = np.dtype(dtype).type
    rng = np.random.default_rng(1)
    vals = np.array([0.1, 0.7, 0.3], dtype=dtype)
    grid = dict(start=T(0), step=T(1), vals=vals)
    for x in rng.uniform(0.01, 1.99, size=2000).astype(dtype):
        a = R.eval(method, "regular", dtype, True, np.array([x]), **grid)[0][0]
        b = R.eval(method, "regular", dtype, False, np.array([x]), **grid)[0][0]
        if a != b:
            break
    else:
        pytest.fail("no point where the flavours differ")
    i = int(np.floor(float(x)))
    y0, y1 = vals[i], vals[i + 1]
    slope = T((y1 - y0) / T(1))
    dx = T(x - T(i))
    exact = Fraction(float(slope)) * Fraction(float(dx)) + Fraction(float(y0))
    assert a == R.round_to(exact, dtype)                                        # one rounding
    assert b == R.round_to(Fraction(float(y0)) + Fraction(float(T(slope * dx))), dtype)  # two


def test_round_to_ties_to_even():
    one = Fraction(1)
    ulp = Fraction(1, 2**23)
    assert R.round_to(one + ulp / 2, np.float32) == np.float32(1.0)          # tie -> even (1.0)
    assert R.round_to(one + 3 * ulp / 2, np.float32) == np.float32(1 + 2 * 2**-23)  # tie -> even (1 + 2 ulp)
    assert R.round_to(one + ulp / 2 + Fraction(1, 2**60), np.float32) == np.float32(1 + 2**-23)


def test_header_compiles_pedantic(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("needs g++")
    src = tmp_path / "t.c"
    src.write_text('#include "interpn_hip.h"\nint main(void) { return INTERPN_HIP_LINEAR_1D == 16 ? 0 : 1; }\n')
    subprocess.check_call([cxx, "-x", "c++", "-std=c++17", "-pedantic", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_one_dim_kernels_do_not_spill(tmp_path):
    sys.path.insert(0, ROOT)
    from tools.kernel_resources import parse

    src = os.path.join(ROOT, "interpn_amd", "csrc", "k_one_dim.hip")
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
             "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "k_one_dim.o")],
            stderr=err, cwd=os.path.dirname(src))
    rows = [r for r in parse(str(remarks)) if "one_dim" in r["demangled"]]
    assert len([r for r in rows if "k_one_dim<" in r["demangled"]]) >= 100, len(rows)
    bad = [(r["demangled"], r["agpr"], r["scratch"]) for r in rows if r["agpr"] != 0 or r["scratch"] != 0]
    assert not bad, bad
