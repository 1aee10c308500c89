#!/usr/bin/env python3
"""Differential fuzz: random (method, kind, N, axis sizes, dtype, linearize, layout knobs, batch
size, special coordinates) through the C ABI against the CPU oracle, bit for bit.
    python tools/fuzz_parity.py [seconds=120] [seed=0]
    python tools/fuzz_parity.py one_dim [seconds=120] [seed=0]     interpn::one_dim against tests/one_dim_restatement.py
Prints one line per failure and a summary; exit code 1 if anything differed."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyoracle
from tests.helpers import run_hip_raw, run_oracle, synthetic_case

KNOBS = ("INTERPN_HIP_BRICKS", "INTERPN_HIP_PPL", "INTERPN_HIP_FORCE_GENERIC", "INTERPN_HIP_GENERIC_RUNTIME",
         "INTERPN_HIP_HOST_CHUNK", "INTERPN_HIP_ITERS_PER_BLOCK", "INTERPN_HIP_AXIS_REGS", "INTERPN_HIP_GENERIC_VEC", "INTERPN_HIP_PERSISTENT",
         "INTERPN_HIP_BINNED", "INTERPN_HIP_DEAL", "INTERPN_HIP_COLUMN", "INTERPN_HIP_COLUMN_THREADS", "INTERPN_HIP_COLUMN_PART",
         "INTERPN_HIP_COLUMN_GROUPS", "INTERPN_HIP_COLUMN_CPP", "INTERPN_HIP_COLUMN_COEF", "INTERPN_HIP_COLUMN_PAD", "INTERPN_HIP_COLUMN_TAIL", "INTERPN_HIP_COLUMN_KEYS", "INTERPN_HIP_SCATTER_STAGED", "INTERPN_HIP_BIN_SCRAMBLE", "INTERPN_HIP_AXIS_RECORDS", "INTERPN_HIP_BIN_SLICE_LOG2", "INTERPN_HIP_SWEEP", "INTERPN_HIP_SWEEP_PERIOD", "INTERPN_HIP_CUBIC_RECORDS", "INTERPN_HIP_SWEEP_PROBE", "INTERPN_HIP_GATED_ITERS", "INTERPN_HIP_SWEEP_LAYOUT",
         "INTERPN_HIP_POINTS_PATH", "INTERPN_HIP_POINTS_SLICE", "INTERPN_HIP_LATTICE")
LAYOUTS_LIN = [None, "off", "11", "12", "22", "c4"]
LAYOUTS_CUB = [None, "off", "44", "24", "22", "14", "11"]


def run_device(case, rng, dtype, fma=None):
    """The persistent-handle device entry point on torch tensors whose first element sits at a
    random element offset (exercises the aligned-vector and the scalar stream paths); a third of the
    cases pass the points interleaved through `eval_points_tensors` instead."""
    import torch

    import interpn_amd

    if case.kind == "regular":
        it = interpn_amd.Interpolator.regular(case.method, case.dims, case.starts, case.steps, case.vals,
                                              linearize_extrapolation=case.linearize, fma=fma)
    else:
        it = interpn_amd.Interpolator.rectilinear(case.method, case.grids, case.vals,
                                                  linearize_extrapolation=case.linearize, fma=fma)
    try:
        nobs = case.obs[0].size
        obs_t = []
        # (the sweep kernel takes 16-byte aligned streams only: mostly even element offsets when it is forced)
        sweep = os.environ.get("INTERPN_HIP_SWEEP") in ("1", "2")
        for o in case.obs:
            off = int(rng.choice([0, 2, 0, 2, 1])) if sweep else int(rng.integers(0, 4))
            t = torch.empty(nobs + off, dtype=torch.float64 if dtype == np.float64 else torch.float32, device="cuda")
            t[off:].copy_(torch.from_numpy(np.ascontiguousarray(o)))
            obs_t.append(t[off:])
        off = int(rng.choice([0, 2, 0, 2, 3])) if sweep else int(rng.integers(0, 4))
        out_full = torch.full((nobs + off,), -777.0, dtype=obs_t[0].dtype, device="cuda")
        out_t = out_full[off:]
        if rng.random() < 0.35:
            # the same points as ONE (n, N) tensor (rows of N or N + 1 elements) through the point-major entry point: mostly the
            # split path in small slices, so that every knob above also runs behind the slices; against the same oracle result
            nd = len(case.obs)
            it.set_option("points_path", int(rng.choice([2, 2, 0])))
            it.set_option("points_slice", int(rng.choice([256, 4096, 65536])))
            rows = torch.full((nobs, nd + int(rng.integers(0, 2))), 1e30, dtype=out_t.dtype, device="cuda")
            for d, t in enumerate(obs_t):
                rows[:, d] = t
            it.eval_points_tensors(rows[:, :nd], out_t)
        else:
            it.eval_tensors(obs_t, out_t)
        err, first_bad = None, None
        try:
            it.finish()
        except AssertionError as e:
            err, first_bad = str(e), getattr(e, "first_bad_index", None)
        return out_t.cpu().numpy(), err, first_bad
    finally:
        it.close()


def run(budget: float, seed: int, max_cases: int = 0):
    """Returns (cases, failures)."""
    from interpn_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(seed)
    t_end = time.time() + budget
    n_cases = n_fail = 0
    saved = {k: os.environ.get(k) for k in KNOBS}
    prev_fma = lib.interpn_hip_set_fma(1)
    try:
        while time.time() < t_end and (max_cases == 0 or n_cases < max_cases):
            method = rng.choice(["linear", "cubic", "nearest"], p=[0.45, 0.4, 0.15])
            kind = rng.choice(["regular", "rectilinear"])
            fp = 4 if method == "cubic" else 2
            nmax = 6 if method == "nearest" else 8
            N = int(rng.integers(1, nmax + 1))
            # keep the grid and the oracle's work bounded
            cap = 2_000_000
            axis = []
            # long axes for N <= 2 (LDS-staged up to 60 KiB of axis image, L1/L2 search beyond)
            axis_cap = 70 if N > 2 or rng.random() < 0.5 else (8000 if N == 1 else 3000)
            for d in range(N):
                hi = max(fp, int(round(cap ** (1.0 / N))))
                axis.append(int(rng.integers(fp, min(hi, axis_cap) + 1)))
            while np.prod(axis) > cap:
                axis[int(np.argmax(axis))] = max(fp, axis[int(np.argmax(axis))] // 2)
            work_per_pt = fp ** N
            nobs = int(min(200_000, max(1, 3_000_000 // work_per_pt)) * rng.uniform(0.05, 1.0)) + int(rng.integers(0, 5))
            dtype = np.float64 if rng.random() < 0.6 else np.float32
            linearize = bool(rng.integers(0, 2))
            extrap = float(rng.choice([0.0, 0.05, 0.3, 2.0]))
            env = {}
            if method == "linear":
                lay = LAYOUTS_LIN[int(rng.integers(0, len(LAYOUTS_LIN)))]
            elif method == "cubic":
                lay = LAYOUTS_CUB[int(rng.integers(0, len(LAYOUTS_CUB)))]
            else:
                lay = None
            if lay: env["INTERPN_HIP_BRICKS"] = lay
            if rng.random() < 0.15: env["INTERPN_HIP_PPL"] = "1"
            if rng.random() < 0.1: env["INTERPN_HIP_FORCE_GENERIC"] = "1"
            if rng.random() < 0.1: env["INTERPN_HIP_GENERIC_RUNTIME"] = "1"
            if rng.random() < 0.2: env["INTERPN_HIP_HOST_CHUNK"] = str(int(rng.integers(1, max(2, nobs))))
            if rng.random() < 0.2: env["INTERPN_HIP_ITERS_PER_BLOCK"] = str(int(rng.choice([1, 2, 3, 8, 64])))
            if rng.random() < 0.4: env["INTERPN_HIP_AXIS_REGS"] = str(int(rng.integers(0, 3)))
            # both forms of the recursive-arm kernel wherever the row-vector form is compiled
            # (k_generic.hip::generic_vec_ok; elsewhere the option falls back to the one-tree form)
            if rng.random() < 0.5: env["INTERPN_HIP_GENERIC_VEC"] = str(int(rng.integers(0, 2)))
            if rng.random() < 0.1: env["INTERPN_HIP_PERSISTENT"] = "1"
            # binned evaluation of the tiled multicubic kernels (device entry point, N = 2..4), dealt or not
            if method == "cubic" and rng.random() < 0.5: env["INTERPN_HIP_BINNED"] = "1"
            if rng.random() < 0.3: env["INTERPN_HIP_DEAL"] = "0"
            # round 3: the LDS-column evaluation of sorted 4-D multicubic points on regular grids (forced where it
            # applies: fully overlapped tiles), its workgroup size / part size, deliberately mis-binned points, short
            # slices; per-bucket search records on or off
            if method == "cubic" and N == 4 and rng.random() < 0.7:  # regular and (round 4) rectilinear grids
                env["INTERPN_HIP_BINNED"] = "1"
                env["INTERPN_HIP_BRICKS"] = "11"
                env["INTERPN_HIP_COLUMN"] = str(int(rng.choice([-1, 1, 1, 1, 0])))
                env["INTERPN_HIP_COLUMN_THREADS"] = str(int(rng.choice([256, 384, 768, 768])))
                env["INTERPN_HIP_COLUMN_GROUPS"] = str(int(rng.integers(1, 3)))
                if rng.random() < 0.6: env["INTERPN_HIP_COLUMN_CPP"] = str(int(rng.choice([1, 2, 3, 5])))  # several K-range phases on small grids
                if rng.random() < 0.5: env["INTERPN_HIP_COLUMN_PART"] = str(int(rng.choice([1, 64, 700, 2048, 12288])))
                if rng.random() < 0.4: env["INTERPN_HIP_BIN_SCRAMBLE"] = "1"
                if rng.random() < 0.4: env["INTERPN_HIP_SCATTER_STAGED"] = "0"
                if rng.random() < 0.3: env["INTERPN_HIP_BIN_SLICE_LOG2"] = "16"
                # round 4, second session: dim 0 from per-part Hermite coefficients (default) or from the values, LDS tiles
                # padded / bare, the bins' tail cut
                if rng.random() < 0.25: env["INTERPN_HIP_COLUMN_COEF"] = "0"
                if rng.random() < 0.5: env["INTERPN_HIP_COLUMN_PAD"] = str(int(rng.integers(0, 2)))
                if rng.random() < 0.4: env["INTERPN_HIP_COLUMN_TAIL"] = str(int(rng.choice([0, 0x22, 0x54, 0x1f])))
                if rng.random() < 0.4: env["INTERPN_HIP_COLUMN_KEYS"] = "0"
            # round 5: the sweep evaluation of 3-D f64 multilinear batches (device entry point), forced on batches of
            # any size, with the measured period, a fixed one, or no clock
            if method == "linear" and N == 3 and rng.random() < 0.7:  # f64 and (second session) f32
                env["INTERPN_HIP_SWEEP"] = "1"
                env["INTERPN_HIP_SWEEP_PERIOD"] = str(int(rng.choice([0, 0, 1, 300, 2500])))
                env.pop("INTERPN_HIP_FORCE_GENERIC", None)
                if rng.random() < 0.4: env["INTERPN_HIP_SWEEP_LAYOUT"] = str(rng.choice(["11", "12"]))  # (round 6: either table, whatever the grid's size)
            if kind == "rectilinear" and rng.random() < 0.3: env["INTERPN_HIP_AXIS_RECORDS"] = "0"
            # round 5, last session: rectilinear multicubic with / without the per-cell records of the axes (or a bound they
            # exceed), and 2-D / 3-D multicubic through the sweep kernel
            if method == "cubic" and kind == "rectilinear" and rng.random() < 0.4: env["INTERPN_HIP_CUBIC_RECORDS"] = str(int(rng.choice([0, 0, 1, 64])))
            if method == "cubic" and N in (2, 3) and rng.random() < 0.3:
                env["INTERPN_HIP_SWEEP"] = "1"
                env["INTERPN_HIP_SWEEP_PERIOD"] = str(int(rng.choice([0, 1, 1500])))
                env["INTERPN_HIP_BRICKS"] = "11"
                env.pop("INTERPN_HIP_FORCE_GENERIC", None)
                env.pop("INTERPN_HIP_BINNED", None)
            # round 6: the device-side sample in front of the sweep kernels and the gated pair of launches behind it, on batches
            # of any size from 16384 points (option sweep = 2), unordered or clustered in one cell (the sample's two verdicts)
            clustered = False
            if ((method == "linear" and N in (2, 3)) or (method == "nearest" and N in (2, 3) and kind == "regular") or (method == "cubic" and N == 2)) \
                    and nobs >= 16384 and rng.random() < 0.5:
                env["INTERPN_HIP_SWEEP"] = "2"
                env["INTERPN_HIP_SWEEP_PROBE"] = str(int(rng.choice([1, 2])))
                env["INTERPN_HIP_GATED_ITERS"] = str(int(rng.choice([0, 1, 3, 16, 64])))
                env.pop("INTERPN_HIP_FORCE_GENERIC", None)
                env.pop("INTERPN_HIP_BINNED", None)
                if method == "cubic": env["INTERPN_HIP_BRICKS"] = "11"
                clustered = bool(rng.random() < 0.5)
            # per-bucket records for 1-D multilinear-rectilinear, also on axes short enough for LDS
            if method == "linear" and kind == "rectilinear" and N == 1 and rng.random() < 0.5: env["INTERPN_HIP_BRICKS"] = "on"
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            case = synthetic_case(method, kind, N, axis, nobs, int(rng.integers(0, 2**31)), dtype, linearize=linearize,
                                  extrap=extrap, specials=bool(rng.integers(0, 2)))
            if method == "cubic" and rng.random() < 0.3:
                # grid values the rectilinear node's short divisions must hand back: a lattice (differences that are exactly +0),
                # blocks of tiny / huge magnitude, zeros of both signs
                v = case.vals.astype(np.float64)
                mode = int(rng.integers(0, 3))
                if mode == 0:
                    v = np.round(v * 4) / 4 + 0.0
                elif mode == 1:
                    k = int(rng.integers(0, v.size))
                    v[k:k + v.size // 7 + 1] *= (1e-300 if dtype == np.float64 else 1e-36) if rng.random() < 0.5 else (1e200 if dtype == np.float64 else 1e30)
                else:
                    k = int(rng.integers(0, v.size))
                    z = np.zeros(min(v.size - k, v.size // 5 + 1))
                    z[rng.random(z.size) < 0.5] = -0.0
                    v[k:k + z.size] = z
                with np.errstate(all="ignore"):
                    case.vals = v.astype(dtype)
            if clustered:  # every point inside one cell (+ a few strays): neighbours share table lines, the one-pass kernel takes the batch
                for d in range(N):
                    g = case.grids[d].astype(np.float64)
                    c = int(rng.integers(0, g.size - 1))
                    keep = case.obs[d][::997].copy()
                    case.obs[d][:] = rng.uniform(g[c], g[c + 1], nobs).astype(dtype)
                    case.obs[d][::997] = keep
            if kind == "rectilinear" and rng.random() < 0.3:
                # inject NaN / inf / huge coordinates: rectilinear never errors, results must still match
                for _ in range(3):
                    case.obs[int(rng.integers(0, N))][int(rng.integers(0, nobs))] = rng.choice([np.nan, np.inf, -np.inf, 1e30, -1e30])
            fma = bool(rng.random() < 0.7)  # the reference's `fma` cargo feature, both flavours
            lib.interpn_hip_set_fma(1 if fma else 0)
            inject = kind == "regular" and rng.random() < 0.25
            if inject:
                # regular grids abort at the first unrepresentable coordinate: same error, same
                # prefix written, rest of `out` untouched (host entry points)
                for _ in range(int(rng.integers(1, 4))):
                    case.obs[int(rng.integers(0, N))][int(rng.integers(0, nobs))] = rng.choice([np.nan, np.inf, -np.inf])
            want = np.full(nobs, -777.0, dtype=dtype)
            got = np.full(nobs, -777.0, dtype=dtype)
            err_o = err_g = None
            try:
                run_oracle(pyoracle, case, fma, out=want)
            except AssertionError as e:
                err_o = str(e)
            device_path = rng.random() < 0.3 or "INTERPN_HIP_COLUMN" in env or "INTERPN_HIP_SWEEP" in env
            # per-handle flavour (round 3): on the device path half of the cases pass the flavour to the handle while the
            # process default says the opposite
            fma_arg = None
            if device_path and rng.random() < 0.5:
                fma_arg = fma
                lib.interpn_hip_set_fma(0 if fma else 1)
            try:
                if device_path:
                    got, err_g, first_bad = run_device(case, rng, dtype, fma_arg)
                else:
                    run_hip_raw(case, out=got)
            except AssertionError as e:
                err_g = str(e)
            except Exception as e:  # noqa: BLE001
                err_g = "EXC " + repr(e)
            if device_path and err_g is not None and err_o == err_g:
                # device entry point: out[first_bad..] is unspecified; the index and the prefix are not
                k = int(np.flatnonzero(want == dtype(-777.0))[0]) if np.any(want == dtype(-777.0)) else nobs
                same = first_bad == k and np.array_equal(got[:k], want[:k], equal_nan=True)
            else:
                same = err_o == err_g and np.array_equal(got, want, equal_nan=True)
            if inject and err_o is None:
                same = False  # the injection must have been seen
            n_cases += 1
            if not same:
                n_fail += 1
                nbad = int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want)))))
                if os.environ.get("FUZZ_DUMP"):
                    ib = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4]
                    print("   DUMP vals abs min/max", float(np.nanmin(np.abs(case.vals))), float(np.nanmax(np.abs(case.vals))), "zeros", int((case.vals == 0).sum()),
                          "bad:", [(int(i), float(got[i]), float(want[i]), [float(o[i]) for o in case.obs]) for i in ib], flush=True)
                print(f"FAIL method={method} kind={kind} N={N} axis={axis} nobs={nobs} dtype={np.dtype(dtype).name} "
                      f"linearize={linearize} fma={fma} device_path={device_path} extrap={extrap} env={env} nbad={nbad} err_oracle={err_o!r} err_hip={err_g!r}", flush=True)
    finally:
        lib.interpn_hip_set_fma(prev_fma)
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return n_cases, n_fail


def _one_dim_grid(rng, kind, dtype, n):
    """A grid from the step / axis families of tests/test_one_dim_gpu.py: (args, lo, hi) with [lo, hi] its finite extent."""
    T = np.dtype(dtype).type
    fi = np.finfo(dtype)
    vals = rng.normal(size=n).astype(dtype)
    if kind == "regular":
        lo_s, hi_s = (2.0**-128, 2.0**128) if dtype == np.float64 else (2.0**-16, 2.0**16)  # StepCellRange<T>
        fam = int(rng.integers(0, 7))
        if fam == 0: step = 0.0731
        elif fam == 1: step = 1.0 / 3.0
        elif fam == 2: step = 2.5 / (n - 1)
        elif fam == 3: step = 2.0 ** float(rng.integers(-12, 8))
        elif fam == 4: step = float(rng.choice([lo_s, hi_s])) * float(rng.choice([1.0, 1.0 + 4 * fi.eps, 1.0 - 4 * fi.eps]))
        elif fam == 5: step = float(rng.uniform(1e-4, 10.0))
        else: step = float(rng.choice([0.0, -0.125, np.nan]))  # degenerate: the division path, every point may fail
        start = float(rng.choice([0.0, -1.25, 1e6, -3e3])) if fam != 4 else 0.0
        start, step = T(start), T(step)
        with np.errstate(all="ignore"):
            stop = T(start + step * T(n - 1))
        return dict(start=start, step=step, vals=vals), float(start), float(stop)
    fam = int(rng.integers(0, 6))
    if fam == 0:
        g = np.cumsum(rng.uniform(0.1, 1.0, size=n)) - 0.3 * n
    elif fam == 1:  # one cluster of knots 1 ulp apart inside a wide axis
        m = min(n - 2, 4000)
        c = np.empty(m, dtype=dtype)
        v = T(rng.uniform(1.0, 2.0))
        for j in range(m):
            c[j] = v
            v = np.nextafter(v, T(np.inf))
        rest = rng.uniform(3.0, 1e4, size=n - m - 1)
        g = np.concatenate([[-50.0], c.astype(np.float64), rest])
    elif fam == 2:
        g = rng.uniform(-1.0, 1.0, size=n) * float(rng.choice([1e-30, 1.0, 1e30]))
    elif fam == 3:  # huge span: overflows in f64, M / span subnormal in f32
        g = np.concatenate([[-0.9 * float(fi.max)], rng.uniform(-10.0, 10.0, size=n - 2), [0.9 * float(fi.max)]])
    elif fam == 4:
        g = np.concatenate([[-np.inf], rng.uniform(-10.0, 10.0, size=n - 2), [np.inf]]) if n > 2 else np.array([-1.0, np.inf])
    else:
        g = rng.normal(size=n)  # unsorted: the std probe sequence
    with np.errstate(all="ignore"):
        g = g.astype(dtype)
    if fam != 5:
        g = np.unique(g)
        vals = vals[:len(g)]
    if len(g) < 2:
        g, vals = np.array([0.0, 1.0], dtype=dtype), vals[:2] if len(vals) >= 2 else np.zeros(2, dtype=dtype)
    fin = g[np.isfinite(g)]
    return dict(grid=g, vals=vals), float(fin.min()), float(fin.max())


def run_one_dim(budget: float, seed: int, max_cases: int = 0):
    """interpn::one_dim against tests/one_dim_restatement.py, bit for bit.  Returns (cases, failures)."""
    import torch

    from interpn_amd import Interpolator
    from tests import one_dim_restatement as R

    rng = np.random.default_rng(seed)
    t_end = time.time() + budget
    n_cases = n_fail = 0
    while time.time() < t_end and (max_cases == 0 or n_cases < max_cases):
        method = str(rng.choice(R.METHODS))
        kind = str(rng.choice(["regular", "rectilinear"]))
        dtype = np.float64 if rng.random() < 0.5 else np.float32
        fma = bool(rng.integers(0, 2))
        n = int(rng.choice([2, 3, int(rng.integers(2, 200)), int(rng.integers(2, 70_001))]))
        args, lo, hi = _one_dim_grid(rng, kind, dtype, n)
        npts = int(rng.choice([1, 2, 3, int(rng.integers(1, 600)), int(rng.integers(1, 9000)), int(rng.integers(1, 60_000))]))
        span = hi - lo if np.isfinite(hi - lo) and hi > lo else 1.0
        with np.errstate(all="ignore"):
            x = np.concatenate([rng.uniform(lo - 0.3 * span, lo + 1.3 * span, npts)[: max(1, npts - npts // 4)],
                                (lo + span * rng.integers(0, 64, npts // 4) / 64.0)])[:npts].astype(dtype)
            near = rng.random(npts) < 0.2  # a fifth of the points moved a few ulps
            for j in range(int(rng.integers(1, 4))):
                x[near] = np.nextafter(x[near], dtype(rng.choice([-np.inf, np.inf])))
        inject = rng.random() < 0.3
        if inject:
            for _ in range(int(rng.integers(1, 4))):
                x[int(rng.integers(0, npts))] = rng.choice([np.nan, np.inf, -np.inf])
        if not inject:
            x[~np.isfinite(x)] = dtype(lo)
        want, bad = R.eval(method, kind, dtype, fma, x, **args)
        opts = {"ppl": int(rng.choice([0, 0, 1])), "axis_lds_kb": int(rng.choice([-1, -1, 0, 1, 60]))}
        device_path = bool(rng.random() < 0.5)
        err = first_bad = None
        ok = True
        try:
            if kind == "regular":
                it = Interpolator.grid1d_regular(method, args["start"], args["step"], args["vals"], device=0, dtype=dtype, fma=fma)
            else:
                it = Interpolator.grid1d_rectilinear(method, args["grid"], args["vals"], device=0, dtype=dtype, fma=fma)
            for k, v in opts.items():
                it.set_option(k, v)
            if device_path:
                tt = torch.float64 if dtype == np.float64 else torch.float32
                o1, o2 = int(rng.integers(0, 4)), int(rng.integers(2, 6))
                ob = torch.zeros(npts + o1, dtype=tt, device="cuda:0")
                ob[o1:] = torch.from_numpy(x)
                full = torch.full((npts + o2 + 2,), -777.0, dtype=tt, device="cuda:0")
                it.eval_tensors([ob[o1:]], full[o2:o2 + npts])
                try:
                    it.finish()
                except AssertionError as e:
                    err, first_bad = str(e), getattr(e, "first_bad_index", None)
                h = full.cpu().numpy()
                got = h[o2:o2 + npts]
                ok = bool(np.all(h[:o2] == -777.0) and np.all(h[o2 + npts:] == -777.0))  # guards
            else:
                got = np.full(npts, -777.0, dtype=dtype)
                try:
                    it.eval_host([x], got)
                except AssertionError as e:
                    err = str(e)
                if bad is not None:
                    ok = bool(np.all(got[bad:] == dtype(-777.0)))  # host: untouched from the first bad point on
                    first_bad = bad
            name = it.kernel_name()
            it.close()
            k = npts if bad is None else bad
            same = ((got[:k] == want[:k]) & (np.signbit(got[:k]) == np.signbit(want[:k]))) | (np.isnan(got[:k]) & np.isnan(want[:k]))
            ok = ok and bool(same.all()) and (err == "Unrepresentable number") == (bad is not None) and (bad is None or first_bad == bad)
            ok = ok and "k_one_dim<" in name and (opts["ppl"] != 1 or name.endswith(", 1>")) and (opts["axis_lds_kb"] != 0 or ", false, " in name[-12:])
        except Exception as e:  # noqa: BLE001
            ok, err = False, "EXC " + repr(e)
        n_cases += 1
        if not ok:
            n_fail += 1
            desc = {k: (v if np.ndim(v) == 0 else f"<{len(v)}>") for k, v in args.items()}
            print(f"FAIL one_dim method={method} kind={kind} dtype={np.dtype(dtype).name} fma={fma} n={n} npts={npts} grid={desc} "
                  f"opts={opts} device_path={device_path} inject={inject} bad={bad} first_bad={first_bad} err={err!r}", flush=True)
    return n_cases, n_fail


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "one_dim":
        budget = float(sys.argv[2]) if len(sys.argv) > 2 else 120.0
        seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
        n_cases, n_fail = run_one_dim(budget, seed)
        print(f"fuzz one_dim: {n_cases} cases, {n_fail} failures, seed {seed}, {budget:.0f} s")
        sys.exit(1 if n_fail else 0)
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    n_cases, n_fail = run(budget, seed)
    print(f"fuzz: {n_cases} cases, {n_fail} failures, seed {seed}, {budget:.0f} s")
    sys.exit(1 if n_fail else 0)
