#!/usr/bin/env python3
"""Multicubic value-and-gradient evaluation against the same handle's plain evaluations on the same device-resident,
unordered points.

    python tools/bench_cubic_grad.py --out profiles/cubic_grad_bench.json [--reps 21] [--only cub3-64-f64]

Method (DESIGN.md "Multicubic gradients", that of tools/bench_grad.py): coordinates drawn on the device (uniform over the grid
widened by 2 %, no order), HIP events around `--inner` back-to-back evaluations, 3 warm-up evaluations per contender, then
`--reps` rounds that ALTERNATE the contenders on one handle in one process, their order rotating from round to round, so that
clock and cache state drift hit all of them alike.  Median and inter-quartile range per contender, in ms per evaluation.

Contenders
  grad_fused    eval_cubic_grad_tensors on the automatic path: k_cubic_grad (N = 2, 3; absent for N = 4)
  grad_n        the same call with option force_generic = 1: k_cubic_grad_n, the runtime-N kernel
  eval_onepass  eval_tensors with options binned = 0, column = 0, sweep = 0: the one-pass tiled value kernel, like for like
  eval_auto     eval_tensors on the automatic path (large batches: sorted or swept)
Finite differences are N + 1 automatic evaluations: (N + 1) x eval_auto.
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, kind, grid shape, dtype, points
WORKLOADS = [
    ("cub3-64-f64", "regular", [64] * 3, np.float64, 10_000_000),
    ("cub3-64-f64-rect", "rectilinear", [64] * 3, np.float64, 10_000_000),
    ("cub3-64-f32", "regular", [64] * 3, np.float32, 10_000_000),
    ("cub3-64-f32-rect", "rectilinear", [64] * 3, np.float32, 10_000_000),
    ("cub2-512-f64", "regular", [512] * 2, np.float64, 30_000_000),
    ("cub4-32-f64", "regular", [32] * 4, np.float64, 1_000_000),
]
PATH_OPTIONS = ("binned", "column", "sweep")


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return float(med), float(q3 - q1)


def run(name, kind, shape, dtype, npts, reps, inner):
    import torch

    import interpn_amd

    rng = np.random.default_rng(1000 + len(name))
    n = len(shape)
    elem = np.dtype(dtype).itemsize
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    grids = []
    for d in range(n):
        g = np.linspace(-1.0, 1.0, shape[d])
        if kind == "rectilinear":
            j = (rng.random(g.size) - 0.5) * 0.5 * (g[1] - g[0])
            j[0] = j[-1] = 0.0
            g = g + j
        grids.append(g.astype(dtype))
    vals = rng.uniform(-1.0, 1.0, int(np.prod(shape))).astype(dtype)
    if kind == "regular":
        starts = np.array([g[0] for g in grids], dtype=dtype)
        steps = np.array([g[1] - g[0] for g in grids], dtype=dtype)
        it = interpn_amd.Interpolator.regular("cubic", shape, starts, steps, vals, linearize_extrapolation=True, dtype=dtype)
    else:
        it = interpn_amd.Interpolator.rectilinear("cubic", grids, vals, linearize_extrapolation=True, dtype=dtype)
    auto = {o: it.get_option(o) for o in PATH_OPTIONS}
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    obs = [(torch.rand(npts, dtype=tdt, device="cuda:0", generator=gen) * 2.04 - 1.02) for _ in range(n)]
    out = torch.empty(npts, dtype=tdt, device="cuda:0")
    grad = torch.empty((n, npts), dtype=tdt, device="cuda:0")

    def f_fused():
        it.eval_cubic_grad_tensors(obs, out, grad)

    def f_n():
        it.set_option("force_generic", 1)
        it.eval_cubic_grad_tensors(obs, out, grad)
        it.set_option("force_generic", 0)

    def f_onepass():
        for o in PATH_OPTIONS:
            it.set_option(o, 0)
        it.eval_tensors(obs, out)

    def f_auto():
        for o in PATH_OPTIONS:
            it.set_option(o, auto[o])
        it.eval_tensors(obs, out)

    contenders = (("grad_fused", f_fused), ("grad_n", f_n), ("eval_onepass", f_onepass), ("eval_auto", f_auto))
    if n not in (2, 3):
        contenders = contenders[1:]  # no fused form: the automatic gradient call IS the runtime-N kernel
    names, paths, ms = {}, {}, {c: [] for c, _ in contenders}
    for label, fn in contenders:
        for _ in range(3):
            fn()
        it.finish()
        names[label] = it.kernel_name()
        paths[label] = it.last_path
    # the value next to the gradient is the plain evaluation's, at the size that is timed
    f_onepass()
    it.finish()
    plain = out.clone()
    same = {}
    for label, fn in contenders[:-2]:
        fn()
        it.finish()
        same[label] = bool(((out == plain) | (out.isnan() & plain.isnan())).all())
    del plain
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    k = len(contenders)
    for rep in range(reps):
        for label, fn in contenders[rep % k:] + contenders[:rep % k]:  # rotate the order
            start.record()
            for _ in range(inner):
                fn()
            stop.record()
            stop.synchronize()
            ms[label].append(start.elapsed_time(stop) / inner)
    it.finish()
    table = it.table_layout()
    it.close()
    row = {"workload": name, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "points": npts, "reps": reps,
           "inner": inner, "kernels": names, "eval_paths": {c: paths[c] for c in ("eval_onepass", "eval_auto")},
           "table_bytes": table[0], "value_bits_equal_eval": same,
           "stream_bytes_per_point": {"eval": (n + 1) * elem, "grad": (2 * n + 1) * elem, "ratio": round((2 * n + 1) / (n + 1), 3)}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "gpoints_per_s": round(npts / (med * 1e-3) / 1e9, 3)}
    best = "grad_fused" if "grad_fused" in row else "grad_n"
    row["automatic_gradient"] = best
    for label in ("grad_fused", "grad_n"):
        if label in row:
            row[f"ratio_{label}_over_eval_onepass"] = round(row[label]["ms"] / row["eval_onepass"]["ms"], 3)
            row[f"ratio_{label}_over_eval_auto"] = round(row[label]["ms"] / row["eval_auto"]["ms"], 3)
            # finite differences: N + 1 automatic evaluations (and lose about half the digits)
            row[f"ratio_finite_differences_over_{label}"] = round((n + 1) * row["eval_auto"]["ms"] / row[label]["ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cubic_grad_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply every workload's point count (profiling runs)")
    ap.add_argument("--only", default="", help="comma-separated workload names")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_cubic_grad.py needs a GPU: nothing is measured without one")
    only = [s for s in a.only.split(",") if s]
    rows = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, kind, shape, dtype, npts in WORKLOADS:
        if only and name not in only:
            continue
        row = run(name, kind, shape, dtype, max(1, int(npts * a.scale)), a.reps, a.inner)
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        doc = {"tool": "tools/bench_cubic_grad.py", "device": torch.cuda.get_device_name(0),
               "method": "HIP events around `inner` evaluations, 3 warm-up evaluations per contender, contenders alternated in one "
                         "process on one handle with rotating order, median and IQR of ms per evaluation",
               "baseline": "eval_onepass", "rows": rows}
        with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
