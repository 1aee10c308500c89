"""Multicubic gradients (interpn_hip_eval_cubic_grad_*, interpn_grad(method="cubic")), the part that needs no GPU: the
exported symbols, the checks made before any device work, the fused kernels' build resources, and the numpy restatement of
the definition (tests/cubic_grad_restatement.py) that the GPU tests compare against bit for bit — its value output against
the oracle, its gradient against answers known exactly, against an exact-rational evaluation of the same definition, and
(in exact arithmetic) continuous across interior knots."""

import os
import shutil
import subprocess
import sys
from ctypes import c_size_t, c_void_p
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OK, INVALID, UNSUPPORTED = 0, 32, 33
SYMBOLS = ["interpn_hip_eval_cubic_grad_device", "interpn_hip_eval_cubic_grad_host"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- ABI and Python surface
def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in header, s
    import inspect

    import interpn_amd

    for name in ("eval_cubic_grad_host", "eval_cubic_grad_tensors"):
        assert hasattr(interpn_amd.Interpolator, name), name
    for cls in ("MulticubicRegular", "MulticubicRectilinear"):
        assert hasattr(getattr(interpn_amd, cls), "eval_cubic_grad"), cls
    params = inspect.signature(interpn_amd.interpn_grad).parameters
    assert params["method"].default == "linear" and params["method"].kind == inspect.Parameter.KEYWORD_ONLY
    assert params["linearize_extrapolation"].default is True


def test_null_handle_and_null_arrays_are_invalid(lib):
    """The codes of the linear namesakes (tests/test_grad_cpu.py), before any device work."""
    n = 4
    x = np.zeros(n)
    ptrs = (c_void_p * 1)(x.ctypes.data)
    lens = (c_size_t * 1)(n)
    for dev, host in ((lib.interpn_hip_eval_grad_device, lib.interpn_hip_eval_grad_host),
                      (lib.interpn_hip_eval_cubic_grad_device, lib.interpn_hip_eval_cubic_grad_host)):
        assert dev(None, ptrs, 1, c_void_p(x.ctypes.data), ptrs, n, None) == INVALID
        assert host(None, ptrs, lens, 1, c_void_p(x.ctypes.data), n, ptrs) == INVALID
        assert dev(None, None, 1, None, None, n, None) == INVALID
        assert host(None, None, None, 1, None, n, None) == INVALID
    assert not x.any()


def test_interpn_grad_method_argument():
    import interpn_amd

    g = [np.linspace(0.0, 1.0, 5)]
    v = np.arange(5.0)
    for bad in ("nearest", "quintic", None):
        with pytest.raises(ValueError):
            interpn_amd.interpn_grad([np.zeros(3)], g, v, method=bad)
    with pytest.raises(TypeError):  # keyword-only
        interpn_amd.interpn_grad([np.zeros(3)], g, v, "cubic")
    with pytest.raises(AssertionError):  # dtype rule of interpn(): float32 / float64 only
        interpn_amd.interpn_grad([np.zeros(3)], g, np.arange(5), method="cubic")


# ---- the restatement's VALUE has the oracle's bits: pins the cell rule, tt, the saturation arms, the footprint indexing and
# the reduction order; N = 5 runs the reference's recursive arm (k1_plain, fma_linear)
AXES = {1: [40], 2: [9, 11], 3: [7, 5, 6], 4: [5, 4, 6, 4], 5: [4, 5, 4, 4, 5]}


@pytest.mark.parametrize("linearize", [True, False], ids=["lin", "quad"])
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_restatement_value_has_the_oracles_bits(oracle, kind, n, dtype, fma, linearize):
    from tests import cubic_grad_restatement as cg
    from tests.helpers import run_oracle, synthetic_case

    case = synthetic_case("cubic", kind, n, AXES[n], 400, seed=7300 + 10 * n + (kind == "regular"), dtype=dtype,
                          linearize=linearize, extrap=0.4, specials=True)
    want = run_oracle(oracle, case, fma=fma)
    got, grad, ok = cg.eval_grad_case(case, fma=fma)
    assert ok.all()
    assert got.dtype == np.dtype(dtype) and grad.shape == (n, 400) and grad.dtype == np.dtype(dtype)
    assert np.array_equal(_bits(got), _bits(want)), int(np.sum(_bits(got) != _bits(want)))


# ---- exact known answers.  The Hermite piece with central-difference slopes (and the edge cells' k1 = 2 dy - k0) reproduces
# a quadratic exactly; on dyadic grids, at dyadic points and with small integer coefficients every intermediate is
# representable, so the restatement must give the analytic derivative exactly.
STARTS = [-1.0, 0.5, 2.0, -0.25]
STEPS = [0.5, 0.25, 1.0, 0.5]
DIMS = [6, 5, 7, 4]
QUAD = [(2, -3, 1), (-1, 2, 4), (3, 1, -2), (1, -4, 0)]  # (a, b, c): q(x) = a x^2 + b x + c


def _q(d, x):
    a, b, c = QUAD[d]
    return a * x * x + b * x + c


def _dq(d, x):
    a, b, _ = QUAD[d]
    return 2 * a * x + b


def _axis_points(d, outside):
    """multiples of step / 8: every knot, points inside every cell (both edge cells included) and, if asked for, up to two
    cells outside on both sides"""
    lo = -16 if outside else 0
    hi = 8 * (DIMS[d] - 1) + (16 if outside else 0)
    return STARTS[d] + (STEPS[d] / 8.0) * np.arange(lo, hi + 1)


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("linearize", [True, False], ids=["lin", "quad"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_sum_of_quadratics_regular_grid_exact(n, linearize, dtype, fma):
    """f = q_0(x_0) + .. + q_(N-1)(x_(N-1)).  Without linearized extrapolation the extended edge polynomial is q_d itself, so
    grad[d] = q_d'(x_d) everywhere, outside the grid too; with it a point outside keeps the slope at the edge knot."""
    from tests import cubic_grad_restatement as cg

    rng = np.random.default_rng(60 + n)
    idx = np.meshgrid(*[STARTS[d] + STEPS[d] * np.arange(DIMS[d]) for d in range(n)], indexing="ij")
    vals = sum(_q(d, idx[d]) for d in range(n)).astype(dtype).ravel()
    pts = [_axis_points(d, outside=True) for d in range(n)]
    npts = 600
    obs = [rng.choice(pts[d], npts).astype(dtype) for d in range(n)]
    for d in range(n):  # every class and both edge cells of every axis are certainly there
        obs[d][:pts[d].size] = pts[d]
    args = (DIMS[:n], np.array(STARTS[:n], dtype=dtype), np.array(STEPS[:n], dtype=dtype))
    out, grad, ok = cg.eval_grad("regular", args, vals, obs, linearize=linearize, fma=fma, dtype=dtype)
    assert ok.all()
    want_out = np.zeros(npts)
    for d in range(n):
        x = obs[d].astype(np.float64)
        lo, hi = STARTS[d], STARTS[d] + STEPS[d] * (DIMS[d] - 1)
        xc = np.clip(x, lo, hi) if linearize else x
        assert np.array_equal(grad[d], _dq(d, xc).astype(dtype)), d
        want_out += _q(d, xc) + _dq(d, xc) * (x - xc)
    assert np.array_equal(out, want_out.astype(dtype))


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("n", [2, 3])
def test_product_of_quadratics_regular_grid_exact(n, fma):
    """f = q_0(x_0) q_1(x_1) (q_2(x_2)): grad[d] = q_d'(x_d) times the other factors — N different numbers, which a swapped tt
    or a D at the wrong level would mix up.  f64 (the products of dyadic fractions need more than 24 bits), extended edge
    polynomials, points inside and outside the grid."""
    from tests import cubic_grad_restatement as cg

    rng = np.random.default_rng(80 + n)
    idx = np.meshgrid(*[STARTS[d] + STEPS[d] * np.arange(DIMS[d]) for d in range(n)], indexing="ij")
    vals = np.prod([_q(d, idx[d]) for d in range(n)], axis=0).ravel()
    obs = [rng.choice(_axis_points(d, outside=True), 500) for d in range(n)]
    args = (DIMS[:n], np.array(STARTS[:n]), np.array(STEPS[:n]))
    out, grad, ok = cg.eval_grad("regular", args, vals, obs, linearize=False, fma=fma)
    q = [_q(d, obs[d]) for d in range(n)]
    assert np.array_equal(out, np.prod(q, axis=0))
    for d in range(n):
        want = _dq(d, obs[d]) * np.prod([q[e] for e in range(n) if e != d], axis=0)
        assert np.array_equal(grad[d], want), d


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_rectilinear_arms_quadratic_exact(dtype, fma):
    """The rectilinear arms on an axis given as coordinates whose spacing happens to be uniform and dyadic (ratios 1,
    weights 1/2: every operation exact; a ratio other than 1 needs 1 / (1 + r), a third at best): the same exact answers
    from the other node function, N = 1 and the sum form in N = 2."""
    from tests import cubic_grad_restatement as cg

    g = [(-0.5 + 0.25 * np.arange(7)).astype(dtype), (1.0 + 0.5 * np.arange(5)).astype(dtype)]
    x = [(-1.0 + np.arange(0, 41) / 16.0).astype(dtype), (0.0 + np.arange(0, 41) / 8.0).astype(dtype)]
    for linearize in (False, True):
        for n in (1, 2):
            X = np.meshgrid(*[a.astype(np.float64) for a in g[:n]], indexing="ij")
            vals = sum(_q(d, X[d]) for d in range(n)).astype(dtype).ravel()
            obs = [x[0], x[1][::-1].copy()][:n]
            out, grad, ok = cg.eval_grad("rectilinear", g[:n], vals, obs, linearize=linearize, fma=fma, dtype=dtype)
            want = np.zeros(41)
            for d in range(n):
                x64 = obs[d].astype(np.float64)
                xc = np.clip(x64, float(g[d][0]), float(g[d][-1])) if linearize else x64
                assert np.array_equal(grad[d], _dq(d, xc).astype(dtype)), (linearize, n, d)
                want += _q(d, xc) + _dq(d, xc) * (x64 - xc)
            assert np.array_equal(out, want.astype(dtype)), (linearize, n)


# ---- the definition in exact rational arithmetic: oracle/exact_rational.py's Hermite-basis form, differentiated
def _dcubic1d(x, g, y, i, linearize):
    """d/dx of exact_rational._cubic1d on cell [i, i + 1] (the cell is an argument, so that a knot can be approached from
    either side)."""
    from oracle.exact_rational import _slope

    n = len(g)
    h = g[i + 1] - g[i]
    dy = y[i + 1] - y[i]
    if i == 0:
        m1 = _slope(g, y, 1)
        m0 = 2 * dy / h - m1
    elif i == n - 2:
        m0 = _slope(g, y, i)
        m1 = 2 * dy / h - m0
    else:
        m0 = _slope(g, y, i)
        m1 = _slope(g, y, i + 1)
    if linearize and x < g[0]:
        return m0
    if linearize and x > g[n - 1]:
        return m1
    t = (x - g[i]) / h
    d00 = 6 * t**2 - 6 * t
    d10 = 3 * t**2 - 4 * t + 1
    d01 = -6 * t**2 + 6 * t
    d11 = 3 * t**2 - 2 * t
    return (d00 * y[i] + d10 * h * m0 + d01 * y[i + 1] + d11 * h * m1) / h


def _dweights_1d(g, x, i, linearize):
    need = sorted({k for k in (i - 1, i, i + 1, i + 2) if 0 <= k < len(g)})
    return {k: _dcubic1d(x, g, {j: (F(1) if j == k else F(0)) for j in need}, i, linearize) for k in need}


def _exact_setup(kind, grids, starts, steps, vals):
    n = len(grids)
    shape = [len(g) for g in grids]
    fv = [F(float(v)) for v in vals]
    if kind == "regular":
        reg = [(F(float(starts[d])), F(float(steps[d]))) for d in range(n)]
        fg = [[reg[d][0] + k * reg[d][1] for k in range(shape[d])] for d in range(n)]
    else:
        reg = [None] * n
        fg = [[F(float(v)) for v in g] for g in grids]
    return shape, fv, reg, fg


def _exact_grad_component(d, x, fg, fv, shape, reg, linearize, cell=None):
    """component d at the point x (Fractions): value weights along e != d, derivative weights along d"""
    from oracle import exact_rational as er

    ws = [er._weights_1d("cubic", fg[e], x[e], linearize, reg[e]) for e in range(len(fg))]
    if cell is None:
        cell = er._cell_regular(x[d], reg[d][0], reg[d][1], shape[d], 2) if reg[d] is not None else er._cell_rect(x[d], fg[d])
    ws[d] = _dweights_1d(fg[d], x[d], cell, linearize)
    return er._contract(ws, fv, shape, False)


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_gradient_against_exact_rational(kind, n, dtype, fma):
    """|grad[d] - exact| <= C N u A_D A_I^(N-1) M / h_d, with u the unit roundoff, M the largest |V| of the point's 4^N
    footprint, h_d the spacing of the cell that holds x_d (what the arm's t was divided by) and
        regular:      C = 23, A_I = 29,  A_D = 61       rectilinear (spacing ratios <= 2):  C = 31, A_I = 47, A_D = 100.

    Where the numbers come from (first order in u; points strictly inside the grid, so |tt| <= 1 in every arm):
    * magnitudes.  With the four inputs of a node bounded by B: |dy| <= 2B; regular |k0| <= B, edge cells |k1| = |2 dy - k0|
      <= 5B (interior: B); a = k0 - dy <= 3B, b = dy - k1 <= 7B, c1 = dy + a <= 5B, c2 = b - (a + a) <= 13B, c3 = a - b <= 10B,
      each bounded as the sum of the bounds of its operands, i.e. as computed.  So |I| and every Horner intermediate <= (1 + 5 +
      13 + 10) B = A_I B = 29 B, |D| <= (5 + 2 * 13 + 3 * 10) B = A_D B = 61 B, and |dD/dtt| <= (2 * 13 + 6 * 10) B = 86 B.
      Rectilinear with spacing ratios r in [1/2, 2]: a central difference is a0 b + c0 dd with a0 + c0 = 1 and |b|, |dd| <=
      2B max(1, 1/r) <= 4B, so |k0| <= 4B, edge |k1| <= 8B; a <= 6B, b <= 10B, c1 <= 8B, c2 <= 22B, c3 <= 16B: A_I = 47, A_D =
      100, |dD/dtt| <= 140 B.
    * roundings.  A node rounds at most 16 times on any path from an input to I or D on a regular grid (dy, cd, k1, a, b, c1,
      c2, c3, e3, up to 6 Horner operations; the halvings and doublings are exact), 24 on a rectilinear one (the ratio, the two
      weights, the quotient and the combination of each difference in addition), each by at most u times a quantity bounded
      above, and passes errors of its inputs on multiplied by at most A_I (A_D at level d).  tt = RN(RN(x - knot) / h) (- 1)
      with the knot and h exact (knots are small multiples of 1/8) carries at most 3u, which moves I by at most 3u A_D B and
      D by at most 3u * 86 B (140 B).
    * total.  The result's scale is S = A_D A_I^(N-1) M; summing the above over the N levels gives u S (16 N + 3 (N - 1)
      A_D / A_I + 3 * 86 / 61 + 1) <= 23 N u S on a regular grid and u S (24 N + 3 (N - 1) 100 / 47 + 3 * 140 / 100 + 1) <= 31
      N u S on a rectilinear one; the division by h_d adds the 1 and scales everything by 1 / h_d.
    The bound is loose (the constants are worst cases over all data of the same size and compound per level) but fixed
    before any run; every sampled point is checked."""
    from tests import cubic_grad_restatement as cg

    dtype = np.dtype(dtype)
    u = 2.0**-53 if dtype == np.float64 else 2.0**-24
    rng = np.random.default_rng(9100 + 100 * n + 10 * (kind == "regular") + (dtype == np.float32))
    npa, npts = 6, 40
    if kind == "regular":
        starts = (rng.integers(0, 9, n) / 8.0).astype(dtype)
        steps = (rng.integers(1, 7, n) / 8.0).astype(dtype)
        grids = [(float(starts[d]) + float(steps[d]) * np.arange(npa)).astype(dtype) for d in range(n)]
        args = ([npa] * n, starts, steps)
        C, AI, AD = 23, 29, 61
    else:
        grids = [(np.cumsum(rng.integers(2, 5, npa)) / 8.0).astype(dtype) for _ in range(n)]  # spacings 2/8 .. 4/8: ratios <= 2
        args = grids
        starts = steps = None
        C, AI, AD = 31, 47, 100
    vals = rng.uniform(-1.0, 1.0, npa**n).astype(dtype)
    obs = []
    for d in range(n):
        lo, hi = float(grids[d][0]), float(grids[d][-1])
        o = rng.uniform(lo, hi, npts).astype(dtype)
        o[:4] = [lo + (grids[d][1] - lo) / 3, hi - (hi - grids[d][-2]) / 3, lo + (grids[d][1] - lo) / 2, hi - (hi - grids[d][-2]) / 2]
        o = np.where((o <= lo) | (o >= hi), dtype.type(lo + (hi - lo) / 3), o)  # strictly inside
        obs.append(o)
    for linearize in (True, False):
        out, grad, ok = cg.eval_grad(kind, args, vals, obs, linearize=linearize, fma=fma, dtype=dtype)
        assert ok.all()
        shape, fv, reg, fg = _exact_setup(kind, grids, starts, steps, vals)
        g64 = [np.array([float(v) for v in fg[d]]) for d in range(n)]
        vabs = np.abs(vals.astype(np.float64)).reshape([npa] * n)
        worst = 0.0
        for k in range(npts):
            x = [F(float(obs[d][k])) for d in range(n)]
            cells = [int(np.clip(np.searchsorted(g64[d], float(obs[d][k]), side="right") - 1, 0, npa - 2)) for d in range(n)]
            M = float(vabs[tuple(slice(max(c - 1, 0), min(c + 3, npa)) for c in cells)].max())
            for d in range(n):
                exact = _exact_grad_component(d, x, fg, fv, shape, reg, linearize)
                h = float(fg[d][cells[d] + 1] - fg[d][cells[d]])
                err = abs(float(F(float(grad[d][k])) - exact))
                bound = C * n * u * AD * AI ** (n - 1) * M / h
                worst = max(worst, err / bound)
                assert err <= bound, (d, k, err, bound)
        print(f"cubic grad vs exact rational: {kind} N={n} {dtype.name} fma={fma} lin={linearize}: worst error / bound = {worst:.2e}")


@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_gradient_is_continuous_across_interior_knots_in_exact_arithmetic(kind, n):
    """The component along d, evaluated on the piece left of an interior knot of axis d and on the piece right of it, agrees
    at the knot — every interior knot of every axis, the other coordinates anywhere inside the grid.  (The multilinear
    gradient jumps there.)  Exact rational arithmetic."""
    rng = np.random.default_rng(300 + n + 10 * (kind == "regular"))
    npa = 6
    if kind == "regular":
        starts = rng.integers(0, 9, n) / 8.0
        steps = rng.integers(1, 7, n) / 8.0
        grids = [starts[d] + steps[d] * np.arange(npa) for d in range(n)]
    else:
        starts = steps = None
        grids = [np.cumsum(rng.integers(1, 7, npa)) / 8.0 for _ in range(n)]
    vals = rng.uniform(-1.0, 1.0, npa**n)
    shape, fv, reg, fg = _exact_setup(kind, grids, starts, steps, vals)
    for d in range(n):
        for knot in range(1, npa - 1):
            x = [F(float(rng.uniform(grids[e][0], grids[e][-1]))) for e in range(n)]
            x[d] = fg[d][knot]
            left = _exact_grad_component(d, x, fg, fv, shape, reg, True, cell=knot - 1)
            right = _exact_grad_component(d, x, fg, fv, shape, reg, True, cell=knot)
            assert left == right, (d, knot, float(left), float(right))


def test_exact_rational_derivative_is_the_derivative():
    """_dcubic1d against the difference quotient of exact_rational._cubic1d: for a cubic p, (p(x + e) - p(x - e)) / 2e =
    p'(x) + e^2 p'''/6 exactly, so the two agree to O(e^2) with e = 2^-30 (and exactly in the linearized arms)."""
    from oracle.exact_rational import _cubic1d

    g = [F(v) for v in (0, 1, 3, 4, 6, 7)]
    y = {k: F(v) for k, v in enumerate((2, -1, 4, 0, 3, 5))}
    e = F(1, 2**30)
    for i, xs in ((0, (F(1, 3), F(-2))), (2, (F(10, 3),)), (4, (F(13, 2), F(9)))):
        for x in xs:
            for lin in (False, True):
                fd = (_cubic1d(x + e, g, y, i, lin) - _cubic1d(x - e, g, y, i, lin)) / (2 * e)
                assert abs(fd - _dcubic1d(x, g, y, i, lin)) <= 100 * e * e, (i, float(x), lin)


# ---- build resources
@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_fused_kernels_have_no_scratch(tmp_path):
    """Every k_cubic_grad instantiation the launcher can reach: no scratch, no AGPRs (the compiler's resource remarks)."""
    from tools.kernel_resources import parse

    csrc = os.path.join(ROOT, "interpn_amd", "csrc")
    shapes = [(t, n, rect, fma, si, sj) for t in ("double", "float") for n in (2, 3) for rect in ("false", "true")
              for fma in ("true", "false") for (si, sj) in ((4, 4), (2, 4), (2, 2), (1, 4), (1, 1))]
    one = tmp_path / "cubic_grad_shapes.hip"
    one.write_text('#include "cubic_grad.h"\nusing namespace interpn;\n' + "".join(
        f"template __global__ void interpn::k_cubic_grad<{t}, {n}, {rect}, {fma}, {si}, {sj}>(const CubicGradArgs<{t}, {n}>);\n"
        for t, n, rect, fma, si, sj in shapes))
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-I", csrc,
             "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(one),
             "-o", str(tmp_path / "cubic_grad_shapes.o")], stderr=err, cwd=csrc)
    rows = [r for r in parse(str(remarks)) if "k_cubic_grad<" in r["demangled"]]
    assert len(rows) == len(shapes), (len(rows), len(shapes))
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    print("k_cubic_grad VGPRs:", {k: sorted({r["vgpr"] for r in rows if f"k_cubic_grad<{k}" in r["demangled"]})
                                  for k in ("double, 2", "double, 3", "float, 2", "float, 3")})
