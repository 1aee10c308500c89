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


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_vectorised_fused_step_is_the_exact_one(dtype):
    """one_dim_restatement.fma_vec against the rational `fma` on random operands, exact ties, operands next to a tie
    (where an f64 'compute wider and round again' shortcut double-rounds in f32), cancellation, zeros of both signs,
    subnormal results and the operands it hands to the scalar path."""
    T = np.dtype(dtype).type
    p = 24 if dtype == np.float32 else 53
    rng = np.random.default_rng(17)
    a, b, c = [], [], []
    for scale in (1.0, 1e-3, 1e4):
        a.append(rng.normal(size=1500) * scale)
        b.append(rng.normal(size=1500))
        c.append(rng.normal(size=1500) / scale)
    r = np.abs(rng.normal(size=400)).astype(dtype) + T(0.5)
    h = (np.nextafter(r, T(np.inf)) - r) / T(2)  # half an ulp of r: r + h is a tie
    e1, e2 = T(1) + T(2.0**-(p - 4)), T(1) - T(2.0**-(p - 4))
    e3 = T(1) + T(2.0**-(p - 1))  # h e3^2 adds bits far below the f64 sum's last place in f32
    for sgn in (1, -1):
        for hb in (T(1), e1, e2, e3):
            a.append(h * hb); b.append(np.full_like(r, sgn) * (e3 if hb is e3 else T(1))); c.append(sgn * r)   # product small
            a.append(r); b.append(np.full_like(r, sgn)); c.append(sgn * h * hb)                                 # addend small
            a.append(r); b.append(np.full_like(r, sgn)); c.append(-sgn * h * hb)
    x = rng.normal(size=300).astype(dtype)
    a.append(x); b.append(x); c.append(-(x * x).astype(dtype))          # cancellation to the product's error term
    a.append(x); b.append(np.ones_like(x)); c.append(-x)                # exact zero: +0
    z = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 0.0, -0.0])
    a.append(z); b.append(np.array([1.0, 1.0, -1.0, -1.0, 0.0, -0.0, 0.0, -0.0])); c.append(np.array([0.0, -0.0, -0.0, 0.0, -0.0, 0.0, 5.0, -0.0]))
    tiny = float(np.finfo(dtype).tiny)
    a.append(x * tiny); b.append(rng.normal(size=300)); c.append(rng.normal(size=300) * tiny)   # subnormal results
    big = float(np.finfo(dtype).max)
    a.append(np.array([big, big, np.inf, np.nan, big, 1e-200, 0.0])); b.append(np.array([2.0, 2.0, 0.0, 1.0, 1.0, 1e-200, np.inf]))
    c.append(np.array([-big, -np.inf, 1.0, 1.0, big, 1.0, 1.0]))
    with np.errstate(all="ignore"):
        a, b, c = (np.concatenate(v).astype(dtype) for v in (a, b, c))
    got = R.fma_vec(a, b, c, dtype)
    want = np.array([R.fma(u, v, w, dtype) for u, v, w in zip(a, b, c)], dtype=dtype)
    eq = ((got == want) & (np.signbit(got) == np.signbit(want))) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~eq)
    assert bad.size == 0, [(float(a[i]).hex(), float(b[i]).hex(), float(c[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]
    if dtype == np.float32:  # the operands really contain cases the shortcut gets wrong
        with np.errstate(all="ignore"):
            naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        assert np.sum(naive != want) > 0
    with np.errstate(all="ignore"):
        assert np.sum((a * b + c).astype(dtype) != want) > 100  # and two roundings in T differ often


def test_knot_points_have_teeth():
    """The regular-grid inputs of tests/test_one_dim_gpu.py::test_regular_cell_index_next_to_knots, in numpy in the
    element type: every non-dyadic (dtype, step) family inside the admitted range holds points where
    floor(a0 * RN(1 / step)) != floor(a0 / step) (a kernel without the margin test would pick the wrong cell there), the
    model of floor_quotient_fast's admission refuses every one of them, and each family has points admitted and points
    refused around the same knot.  Power-of-two steps: the product is exact, no such point."""
    from tests import test_one_dim_gpu as G

    for label, dtype, start, step, n in G.TEETH_FAMILIES:
        T = np.dtype(dtype).type
        rng = np.random.default_rng(sum(map(ord, label)))
        x, k = G.knot_points(dtype, T(start), T(step), n, rng, ncells=20_000)
        lo, hi = G.step_limits(dtype)
        assert lo <= float(T(step)) <= hi, label
        a0 = (x - T(start)).astype(dtype)
        ok, f_fast, f_div = G.fast_path_model(dtype, a0, T(step))
        differ = f_fast != f_div
        print(label, "points", x.size, "differ", int(differ.sum()), "admitted", int(ok.sum()), "differ and admitted", int((differ & ok).sum()))
        assert differ.sum() > 0, label
        assert (differ & ok).sum() == 0, label  # today's margin refuses them all
        adm = np.zeros(n, dtype=bool)
        ref = np.zeros(n, dtype=bool)
        adm[k[ok]] = True
        ref[k[~ok]] = True
        assert (adm & ref).sum() > 0, label
    for dtype in (np.float64, np.float32):
        T = np.dtype(dtype).type
        x, k = G.knot_points(dtype, T(-1.25), T(0.125), 100_003, np.random.default_rng(1), ncells=5000)
        ok, f_fast, f_div = G.fast_path_model(dtype, (x - T(-1.25)).astype(dtype), T(0.125))
        assert (f_fast != f_div).sum() == 0
    # the limits of StepCellRange<T> as the families use them: in, on and out
    for dtype in (np.float64, np.float32):
        lo, hi = G.step_limits(dtype)
        s = G._limit_steps(dtype)
        assert float(s["lo"]) == lo and float(s["hi"]) == hi
        assert lo < float(s["lo_in"]) and float(s["hi_in"]) < hi and float(s["lo_out"]) < lo and float(s["hi_out"]) > hi
        one = np.ones(1, dtype=dtype)
        assert G.fast_path_model(dtype, one * s["lo"] * 2.5, s["lo"])[0].all() and not G.fast_path_model(dtype, one, s["lo_out"])[0].any()
        assert not G.fast_path_model(dtype, one, s["hi_out"])[0].any()


# Error bound of the linear pair against one_dim_restatement.exact, from the operation count of one_dim/linear.rs:28-34
# (u = 2^-p the unit roundoff, every operation correctly rounded: computed = exact (1 + d), |d| <= u):
#   dxg = (x1 - x0)(1 + d1), dy = (y1 - y0)(1 + d2), slope = dy / dxg (1 + d3), dx = (x - x0)(1 + d4)
#   => slope dx = t (1 + th4) with t = (y1 - y0)(x - x0)/(x1 - x0) and |th4| <= 4u / (1 - 4u);
#   fused:    r = (slope dx + y0)(1 + d5):              |r - (y0 + t)| <= |th4|(1 + u)|t| + u |y0 + t| <= 5 u (1 + 2^-20) scale
#   unfused:  r = (y0 + slope dx (1 + d5))(1 + d6):     one more rounding on t:                            6 u (1 + 2^-20) scale
# with scale = |y0| + |t| (the (1 + 2^-20) covers the second-order terms for p >= 24).  Underflow is the one way an
# operation misses |d| <= u (overflow aside: points with an infinite intermediate are left out): the division and the product / fused step then err by at most half the smallest subnormal
# eta, the slope's share multiplied by |x - x0|; subtractions are exact there.  Hence + eta (1 + |x - x0|).
# K is derived, not tuned.  Worst ratio |restatement - exact| / (u scale) seen by test_restatement_within_exact_bound:
# fused 2.01 (f64) / 3.02 (f32), unfused 3.02 / 3.02.
EXACT_K = {True: 5, False: 6}


def exact_bound_check(dtype, fma, x, got, value, scale, x0_dist=None):
    """Largest |got - exact| / (u scale) over the points given, after asserting each within K u scale + the underflow
    allowance.  Points must be finite with finite results."""
    p = 53 if np.dtype(dtype) == np.float64 else 24
    u = Fraction(1, 2**p)
    eta = Fraction(float(np.finfo(dtype).smallest_subnormal))
    worst = 0.0
    for j in range(len(x)):
        err = abs(Fraction(float(got[j])) - value[j])
        allow = EXACT_K[fma] * u * (1 + Fraction(1, 2**20)) * scale[j] + eta * (1 + (x0_dist[j] if x0_dist is not None else 0))
        assert err <= allow, (j, float(x[j]).hex(), float(got[j]).hex(), float(value[j]), float(err / (u * scale[j])) if scale[j] else None)
        if scale[j]:
            worst = max(worst, float(err / (u * scale[j])))
    return worst


def check_against_exact(kind, dtype, x, args, evaluate):
    """Every method and flavour of `evaluate(method, fma, x) -> out` against R.exact on the finite points of x.  Regular
    grids: only points whose rounded quotient selects the exact cell (test_exact_cell_share_left_out counts the others).
    Returns the worst ratios {fma: ratio}."""
    x = x[np.isfinite(x)]
    cell_r = R.grid_at(kind, dtype, x, **args)[0]
    worst = {True: 0.0, False: 0.0}
    for method in R.METHODS:
        value, scale, cell, tie = R.exact(method, kind, dtype, x, **args)
        keep = np.array([v is not None for v in value]) & (cell == cell_r)
        if kind == "rectilinear":
            assert np.array_equal(cell, cell_r)
        for fma in ((True, False) if method.startswith("Linear") else (False,)):
            got = evaluate(method, fma, x)
            k = keep & np.isfinite(got)
            if method == "Nearest1D":
                # Also left out: points whose two distances differ exactly but round to the same T (x = max-finite far
                # from both knots, a mid-point formed by rounding): the reference compares the rounded distances
                # (one_dim/hold.rs:98-104) and sees a tie there.  Rounding is monotone, so wherever the rounded distances
                # differ their order is the exact one, and those points must agree bit for bit.
                if kind == "rectilinear":
                    xa, xb = args["grid"][cell], args["grid"][cell + 1]
                else:
                    xa = (args["start"] + args["step"] * cell.astype(dtype)).astype(dtype)
                    xb = (xa + args["step"]).astype(dtype)
                with np.errstate(all="ignore"):
                    k &= ~tie & (np.abs(x - xa) != np.abs(x - xb))
            if method.startswith("Linear"):
                # the (1 + d) model needs every intermediate finite: an x1 - x0 that overflows to inf gives slope 0 and a
                # finite result that no bound of this kind covers ([-0.9 max, 0.9 max])
                if kind == "rectilinear":
                    xa, xb = args["grid"][cell], args["grid"][cell + 1]
                else:
                    xa = (args["start"] + args["step"] * cell.astype(dtype)).astype(dtype)
                    xb = (xa + args["step"]).astype(dtype)
                ya, yb = args["vals"][cell], args["vals"][cell + 1]
                with np.errstate(all="ignore"):
                    k &= np.isfinite(xb - xa) & np.isfinite((yb - ya) / (xb - xa)) & np.isfinite(x - xa) & np.isfinite(((yb - ya) / (xb - xa)) * (x - xa))
            idx = np.flatnonzero(k)
            if method.startswith("Linear"):
                g = args.get("grid")
                x0 = None
                if kind == "rectilinear":
                    x0 = [abs(Fraction(float(x[j])) - Fraction(float(g[cell[j]]))) for j in idx]
                else:
                    x0 = [abs(Fraction(float(x[j])) - Fraction(float(args["start"]))) for j in idx]
                w = exact_bound_check(dtype, fma, x[idx], got[idx], [value[j] for j in idx], [scale[j] for j in idx], x0)
                worst[fma] = max(worst[fma], w)
            else:  # a selected value: bit for bit
                want = np.array([float(value[j]) for j in idx], dtype=dtype)
                assert np.array_equal(got[idx], want), (method, kind)
    return worst


def test_restatement_within_exact_bound():
    """tests/one_dim_restatement.py against something that is not itself: R.exact on samples of the regular families and
    the stressed axes of tests/test_one_dim_gpu.py, both flavours and dtypes."""
    from tests import test_one_dim_gpu as G

    worst = {}
    for label, (dtype, start, step, n) in G.regular_families().items():
        if n > 2**23:
            continue  # exact() lists every knot; f32 past 2^24 cells the knots coincide
        rng = np.random.default_rng(sum(map(ord, label)))
        args = dict(start=start, step=step, vals=rng.normal(size=n).astype(dtype))
        x, _ = G.knot_points(dtype, start, step, n, rng, ncells=40)
        x = np.concatenate([x, rng.uniform(float(start) - 3 * float(step), float(start) + float(step) * (n + 2), 300).astype(dtype)])
        ev = lambda m, f, xs: R.eval(m, "regular", dtype, f, xs, **args)[0]
        for f, w in check_against_exact("regular", dtype, x, args, ev).items():
            key = (np.dtype(dtype).name, f)
            worst[key] = max(worst.get(key, 0.0), w)
    for dtype in (np.float64, np.float32):
        for name, g in G.stressed_axes(dtype).items():
            rng = np.random.default_rng(len(g))
            args = dict(grid=g, vals=rng.normal(size=len(g)).astype(dtype))
            x = G.axis_points(g)
            x = x[rng.permutation(len(x))[:1500]]
            ev = lambda m, f, xs: R.eval(m, "rectilinear", dtype, f, xs, **args)[0]
            for f, w in check_against_exact("rectilinear", dtype, x, args, ev).items():
                key = (np.dtype(dtype).name, f)
                worst[key] = max(worst.get(key, 0.0), w)
    print("worst |restatement - exact| / (u scale):", worst)
    for (name, f), w in worst.items():
        assert 0 < w <= EXACT_K[f]


def test_exact_cell_share_left_out():
    """Regular grids: the share of a family's finite points (the full point set of
    test_regular_cell_index_next_to_knots, test_one_dim_gpu.family_points) whose rounded quotient
    floor((x - start) / step) selects another cell than the exact comparison against the knots T(start + step T(i)), and
    which the exact bound therefore leaves out: at most 1 % per family.  Such points exist only next to knots (where the
    knot as the reference rounds it and the quotient's own rounding disagree about a point a few ulps away); of the
    knot neighbourhoods alone they are up to 17.5 % (f64 start 1e6, where x - start cancels and the knots carry
    ulp(1e6); f32 2.5/(n-1) 15.3 %, f32 past 2^24 13.5 %, f64 2.5/(n-1) 10.2 %, f64 1/3 2.3 %, f32 0.0731 2.2 %), by the
    reference's arithmetic, whatever a kernel does.  The families therefore carry 20 bulk points per knot neighbour,
    not a wider assertion; the test prints both shares."""
    from tests import test_one_dim_gpu as G

    over = {}
    for label, (dtype, start, step, n) in G.regular_families().items():
        if n > 2**23:
            continue  # not bounded against exact() (f32 past 2^24 cells: the step is below an ulp of x, knots coincide)
        T = np.dtype(dtype).type
        x, _ = G.family_points(label)
        nknot = len(G.knot_points(dtype, start, step, n, np.random.default_rng(sum(map(ord, label))))[0])
        cell_r = R.grid_at("regular", dtype, x, start=start, step=step, vals=np.zeros(n, dtype=dtype))[0]
        knots = (T(start) + T(step) * np.arange(n).astype(dtype)).astype(dtype)
        cell = np.clip(np.searchsorted(knots, x, side="right") - 1, 0, n - 2)
        out = cell != cell_r
        share = float(out.mean())
        print(f"{label}: {int(out.sum())} of {len(x)} left out ({100 * share:.2f} %); of the first {nknot} (knot neighbours) "
              f"{100 * float(out[:nknot].mean()):.2f} %")
        if share > 0.01:
            over[label] = round(100 * share, 2)
    assert not over, over
