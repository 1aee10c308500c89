"""Multilinear gradients (interpn_hip_eval_grad_*, interpn_grad), the part that needs no GPU: the exported symbols, the
checks made before any device work, and the numpy restatement of the definition (tests/grad_restatement.py) that the GPU
tests compare against bit for bit — its value output against the oracle, its gradient against answers known exactly and
against the exact-rational evaluation, and the fused kernel's build resources."""

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
SYMBOLS = ["interpn_hip_eval_grad_device", "interpn_hip_eval_grad_host"]


@pytest.fixture(scope="module")
def lib():
    from interpn_amd import _lib

    return _lib.load()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_symbols_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "interpn_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in header, s
    import interpn_amd

    assert "interpn_grad" in interpn_amd.__all__ and callable(interpn_amd.interpn_grad)
    for name in ("eval_grad_host", "eval_grad_tensors"):
        assert hasattr(interpn_amd.Interpolator, name), name
    for cls in ("MultilinearRegular", "MultilinearRectilinear", "MulticubicRegular", "MulticubicRectilinear", "NearestRegular",
                "NearestRectilinear"):
        assert hasattr(getattr(interpn_amd, cls), "eval_grad"), cls


def test_autograd_module_imports_torch_lazily():
    code = ("import sys; import interpn_amd; assert 'interpn_amd.autograd' not in sys.modules; "
            "import interpn_amd.autograd as a; assert 'torch' not in sys.modules; assert callable(a.interp)")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT, env={**os.environ, "PYTHONPATH": ROOT})


def test_null_handle_and_null_arrays_are_invalid(lib):
    n = 4
    x = np.zeros(n)
    ptrs = (c_void_p * 1)(x.ctypes.data)
    lens = (c_size_t * 1)(n)
    assert lib.interpn_hip_eval_grad_device(None, ptrs, 1, c_void_p(x.ctypes.data), ptrs, n, None) == INVALID
    assert lib.interpn_hip_eval_grad_host(None, ptrs, lens, 1, c_void_p(x.ctypes.data), n, ptrs) == INVALID
    assert lib.interpn_hip_eval_grad_device(None, None, 1, None, None, n, None) == INVALID
    assert lib.interpn_hip_eval_grad_host(None, None, None, 1, None, n, None) == INVALID


def test_interpn_grad_rejects_what_interpn_rejects():
    import interpn_amd

    g = [np.linspace(0.0, 1.0, 4)]
    with pytest.raises(AssertionError):  # dtype rule of interpn(): float32 / float64 only
        interpn_amd.interpn_grad([np.zeros(3)], g, np.arange(4))
    with pytest.raises(TypeError):
        interpn_amd.interpn_grad([np.zeros(3)], g, [0.0, 1.0, 2.0, 3.0])


# ---- the restatement's VALUE has the oracle's bits: pins the cell rule, t, the corner indexing and the reduction order
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_restatement_value_has_the_oracles_bits(oracle, kind, n, dtype, fma):
    from tests import grad_restatement as gr
    from tests.helpers import run_oracle, synthetic_case

    axis = {1: [40], 2: [9, 11], 3: [7, 5, 6], 4: [5, 4, 6, 3], 5: [4, 3, 5, 3, 4], 6: [3, 4, 3, 3, 2, 4]}[n]
    case = synthetic_case("linear", kind, n, axis, 400, seed=7100 + 10 * n + (kind == "regular"), dtype=dtype, specials=True)
    want = run_oracle(oracle, case, fma=fma)
    got, grad, ok = gr.eval_grad_case(case, fma=fma)
    assert ok.all()
    assert got.dtype == np.dtype(dtype) and grad.shape == (n, 400) and grad.dtype == np.dtype(dtype)
    assert np.array_equal(_bits(got), _bits(want)), int(np.sum(_bits(got) != _bits(want)))


# ---- exact known answers: power-of-two steps, dyadic points and small integers make every operation exact
def _dyadic_points(rng, lo, hi, npts, dtype):
    """multiples of 1/16 in [lo, hi]"""
    return (rng.integers(int(lo * 16), int(hi * 16) + 1, npts) / 16.0).astype(dtype)


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_affine_data_regular_grid_exact(n, dtype, fma):
    from tests import grad_restatement as gr

    rng = np.random.default_rng(50 + n)
    dims = [5, 4, 6, 3][:n]
    starts = np.array([-1.0, 0.5, 2.0, -0.25][:n], dtype=dtype)
    steps = np.array([0.5, 0.25, 2.0, 1.0][:n], dtype=dtype)
    a = [3, -2, 5, 7][:n]
    idx = np.meshgrid(*[np.arange(m) for m in dims], indexing="ij")
    vals = sum(a[d] * idx[d] for d in range(n)).astype(dtype).ravel()
    # inside the grid and up to two cells outside on both sides: outside, the edge cell's slope is the same constant
    obs = [_dyadic_points(rng, starts[d] - 2 * steps[d], starts[d] + steps[d] * (dims[d] + 1), 300, dtype) for d in range(n)]
    out, grad, ok = gr.eval_grad("regular", (dims, starts, steps), vals, obs, fma=fma, dtype=dtype)
    assert ok.all()
    for d in range(n):
        want = np.full(300, a[d] / float(steps[d]), dtype=dtype)
        assert np.array_equal(_bits(grad[d]), _bits(want)), d
    want_out = sum(a[d] * (obs[d].astype(np.float64) - float(starts[d])) / float(steps[d]) for d in range(n)).astype(dtype)
    assert np.array_equal(out, want_out)


@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_product_data_exact(kind, dtype, fma):
    """f = x y z is trilinear, so the interpolant reproduces it and grad = (y z, x z, x y) at the point — three different
    numbers, which a swapped t index would mix up.  Dyadic knots and points: exact in both element types."""
    from tests import grad_restatement as gr

    rng = np.random.default_rng(77)
    if kind == "regular":
        grids = [np.arange(5) * 0.5 - 1.0, np.arange(4) * 1.0 + 1.0, np.arange(6) * 0.25]
        args = ([5, 4, 6], np.array([-1.0, 1.0, 0.0], dtype=dtype), np.array([0.5, 1.0, 0.25], dtype=dtype))
    else:
        # cell widths are powers of two, so t is exact too
        grids = [np.array([-1.0, -0.5, 0.5, 1.0, 2.0]), np.array([1.0, 2.0, 2.5, 4.5]), np.array([0.0, 0.125, 0.375, 0.875, 1.875, 2.0])]
        args = [g.astype(dtype) for g in grids]
    X = np.meshgrid(*grids, indexing="ij")
    vals = (X[0] * X[1] * X[2]).astype(dtype).ravel()
    obs = [_dyadic_points(rng, g[0], g[-1], 500, dtype) for g in grids]
    out, grad, ok = gr.eval_grad(kind, args, vals, obs, fma=fma, dtype=dtype)
    x, y, z = (o.astype(np.float64) for o in obs)
    assert np.array_equal(out, (x * y * z).astype(dtype))
    for d, want in enumerate((y * z, x * z, x * y)):
        assert np.array_equal(grad[d], want.astype(dtype)), d


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_points_outside_the_grid_get_the_edge_cells_slope(kind, dtype):
    from tests import grad_restatement as gr

    g = [np.array([0.0, 0.5, 1.0, 1.5]) if kind == "regular" else np.array([0.0, 0.5, 2.0, 2.5]), np.array([1.0, 2.0, 3.0])]
    vals = np.array([[0, 1, 4], [2, 3, 8], [5, 9, 6], [7, 2, 1]], dtype=dtype).ravel()
    args = ([4, 3], np.array([0.0, 1.0], dtype=dtype), np.array([0.5, 1.0], dtype=dtype)) if kind == "regular" else [a.astype(dtype) for a in g]
    # below both axes; above both: t of the other dimension is 1.5 / -0.5 and so on, all dyadic
    obs = [np.array([-0.25, g[0][-1] + 0.25], dtype=dtype), np.array([0.5, 3.5], dtype=dtype)]
    out, grad, ok = gr.eval_grad(kind, args, vals, obs, fma=True, dtype=dtype)
    v = vals.reshape(4, 3).astype(np.float64)
    # point 0: cell (0, 0), t = (-0.5, -0.5); point 1: cell (2, 1), t = (1.5, 1.5)
    for p, (i, j, t0, t1) in enumerate([(0, 0, -0.5, -0.5), (2, 1, 1.5, 1.5)]):
        h0, h1 = float(g[0][i + 1] - g[0][i]), float(g[1][j + 1] - g[1][j])
        w0 = [v[i + 1, j] - v[i, j], v[i + 1, j + 1] - v[i, j + 1]]
        w1 = [v[i, j + 1] - v[i, j], v[i + 1, j + 1] - v[i + 1, j]]
        assert grad[0][p] == dtype((w0[0] + t1 * (w0[1] - w0[0])) / h0)
        assert grad[1][p] == dtype((w1[0] + t0 * (w1[1] - w1[0])) / h1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_dimension_exact(dtype):
    from tests import grad_restatement as gr

    vals = np.array([1.0, 4.0, -2.0, 0.0, 8.0], dtype=dtype)
    x = np.array([-3.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 7.0], dtype=dtype)
    # regular: start 0, step 0.5.  A knot belongs to the cell on its right (floor), the last knot to the last cell.
    out, grad, ok = gr.eval_grad("regular", ([5], np.array([0.0], dtype=dtype), np.array([0.5], dtype=dtype)), vals, [x], dtype=dtype)
    assert np.array_equal(grad[0], np.array([6, 6, 6, -12, -12, 4, 16, 16, 16], dtype=dtype))
    # rectilinear: partition_point(g < x) - 1 puts a knot into the cell on its LEFT
    g = np.array([0.0, 0.5, 1.0, 1.5, 2.0], dtype=dtype)
    out, grad, ok = gr.eval_grad("rectilinear", [g], vals, [x], dtype=dtype)
    assert np.array_equal(grad[0], np.array([6, 6, 6, 6, -12, -12, 4, 16, 16], dtype=dtype))
    assert np.array_equal(out[1:8], np.array([1.0, 2.5, 4.0, 1.0, -2.0, 0.0, 8.0], dtype=dtype))


# ---- against the exact-rational evaluation
@pytest.mark.parametrize("fma", [True, False], ids=["fma", "nofma"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["regular", "rectilinear"])
def test_gradient_against_exact_rational(kind, n, dtype, fma):
    """Inside a cell the interpolant is linear in x_d, so its exact partial derivative there is the exact difference
    quotient of two exact evaluations in that cell (oracle/exact_rational.py, Fractions).

    Bound: |grad[d] - exact| <= 8 N u M_d / h_d with u the unit roundoff and M_d the largest |V[c' | 1 << d] - V[c']| of
    the cell, from counting roundings with t in [0, 1]: one for W, at most three of relative size <= 2 M per lerp level
    (dy, the fused or unfused step, and the rounding of t) over N - 1 levels, one for the division.  That count takes t
    as the correctly rounded quotient, i.e. x - x0 and the knot itself exact.  The grids are chosen so that this holds:
    knots are non-negative multiples of 1/8 (regular: start and step such multiples), so start + step * i is exact, and
    for x0 <= x every such x0 is a multiple of ulp(x), which makes x - x0 (< x, a multiple of ulp(x)) exact.  The data
    are uniform random numbers, the points uniform random numbers strictly inside the grid (no knots, no polynomial).
    Every sampled point is checked."""
    from oracle import exact_rational
    from tests import grad_restatement as gr

    dtype = np.dtype(dtype)
    u = 2.0**-53 if dtype == np.float64 else 2.0**-24
    rng = np.random.default_rng(9000 + 100 * n + 10 * (kind == "regular") + (dtype == np.float32))
    npa, npts = 5, 60
    if kind == "regular":
        starts = (rng.integers(0, 9, n) / 8.0).astype(dtype)
        steps = (rng.integers(1, 7, n) / 8.0).astype(dtype)
        grids = [(float(starts[d]) + float(steps[d]) * np.arange(npa)).astype(dtype) for d in range(n)]
        args = ([npa] * n, starts, steps)
    else:
        grids = [(np.cumsum(rng.integers(1, 7, npa)) / 8.0).astype(dtype) for _ in range(n)]
        args = grids
        starts = steps = None
    vals = rng.uniform(-1.0, 1.0, npa**n).astype(dtype)
    obs = []
    for d in range(n):
        lo, hi = float(grids[d][0]), float(grids[d][-1])
        o = rng.uniform(lo, hi, npts).astype(dtype)
        o = np.where(np.isin(o, grids[d]) | (o <= lo) | (o >= hi), dtype.type(lo + (hi - lo) / 3), o)  # strictly inside, off the knots
        obs.append(o)
    out, grad, ok = gr.eval_grad(kind, args, vals, obs, fma=fma, dtype=dtype)
    assert ok.all()
    g64 = [g.astype(np.float64) for g in grids]
    vshape = vals.reshape([npa] * n).astype(np.float64)
    base = exact_rational.evaluate("linear", kind, g64, vals, obs, False, starts, steps)
    worst = 0.0
    for d in range(n):
        cell = np.clip(np.searchsorted(g64[d], obs[d].astype(np.float64), side="left") - 1, 0, npa - 2)
        x0, x1 = g64[d][cell], g64[d][cell + 1]
        # a second point of the same cell along d: a quarter or three quarters of the cell, whichever is farther (exact floats)
        xq = np.where(obs[d].astype(np.float64) - x0 > (x1 - x0) / 2, x0 + (x1 - x0) / 4, x0 + 3 * (x1 - x0) / 4)
        moved = [o.astype(np.float64) for o in obs]
        moved[d] = xq
        other = exact_rational.evaluate("linear", kind, g64, vals, moved, False, starts, steps)
        for k in range(npts):
            exact = (other[k] - base[k]) / (F(float(xq[k])) - F(float(obs[d][k])))
            # M_d of the point's cell
            cells = [int(np.clip(np.searchsorted(g64[e], float(obs[e][k]), side="left") - 1, 0, npa - 2)) for e in range(n)]
            sl = tuple(slice(c, c + 2) for c in cells)
            blk = vshape[sl]
            M = float(np.max(np.abs(np.diff(blk, axis=d))))
            h = float(x1[k] - x0[k])
            err = abs(float(F(float(grad[d][k])) - exact))
            bound = 8 * n * u * M / h
            worst = max(worst, err / bound)
            assert err <= bound, (d, k, err, bound)
    print(f"grad vs exact rational: {kind} N={n} {dtype.name} fma={fma}: worst error / bound = {worst:.3f}")


# ---- build resources
@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_fused_f64_3d_kernels_have_no_scratch(tmp_path):
    from tools.kernel_resources import parse

    csrc = os.path.join(ROOT, "interpn_amd", "csrc")
    shapes = [(rect, fma, si, sj, ppl, axr) for rect, axrs in (("false", (0,)), ("true", (0, 1, 2, 3)))
              for axr in axrs for fma in ("true", "false") for (si, sj) in ((1, 1), (1, 2), (2, 2)) for ppl in (1, 2)]
    one = tmp_path / "grad_shapes.hip"
    one.write_text('#include "linear_grad.h"\nusing namespace interpn;\n' + "".join(
        f"template __global__ void interpn::k_linear_grad<double, 3, {rect}, {fma}, {si}, {sj}, {ppl}, {axr}, 0>(const GradArgs<double, 3>);\n"
        for rect, fma, si, sj, ppl, axr in shapes))
    remarks = tmp_path / "remarks.txt"
    with open(remarks, "w") as err:
        subprocess.check_call(
            [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950", "-I", csrc,
             "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(one),
             "-o", str(tmp_path / "grad_shapes.o")], stderr=err, cwd=csrc)
    rows = [r for r in parse(str(remarks)) if "k_linear_grad<double, 3" in r["demangled"]]
    assert len(rows) == len(shapes), (len(rows), len(shapes))
    bad = [(r["demangled"], r["vgpr"], r["agpr"], r["scratch"]) for r in rows if r["scratch"] != 0 or r["agpr"] != 0]
    assert not bad, bad
    print("k_linear_grad<double, 3, ...> VGPRs:", sorted({r["vgpr"] for r in rows}))
