#!/usr/bin/env python3
"""Point-major gradients (positions (n, N) in, gradient (n, N) out) against what a caller had to do before they existed.

    python tools/bench_points_grad.py --out profiles/points_grad_bench.json [--reps 21] [--only lin3-64-f64] [--small 1000000]

Method (the protocol of section 12): points drawn on the device (uniform over the grid widened by
2 %, no order), HIP events around `--inner` back-to-back evaluations, 3 warm-up evaluations per contender, then `--reps`
rounds that ALTERNATE the contenders on one handle in one process, their order rotating from round to round.  Median and
inter-quartile range per contender, in ms per evaluation.

Contenders
  A_auto        eval_points_grad_tensors, automatic path, load and store forms
  A_l<L>_s<S>   ... the fused multilinear kernel with points_load = L and points_store = S forced (1 per-lane vectors, 2 the
                wave's span through LDS (3-D f64 only), 3 elements)
  B_columns     eval_grad_tensors / eval_cubic_grad_tensors on pre-split columns into component-major output: the
                like-for-like kernel, equal bytes per point
  C_transpose   what a caller does today, timed together: pts.T.contiguous(), the gradient call, grad.T.contiguous()
  D_split       eval_points_grad_tensors with points_path = 2: de-interleave, the column kernel, interleave, slice by slice
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, method, kind, grid shape, dtype, points of the large size
WORKLOADS = [
    ("lin3-64-f64", "linear", "regular", [64] * 3, np.float64, 100_000_000),
    ("lin3-64-f64-rect", "linear", "rectilinear", [64] * 3, np.float64, 100_000_000),
    ("lin3-64-f32", "linear", "regular", [64] * 3, np.float32, 100_000_000),
    ("lin2-1000-f64", "linear", "regular", [1000] * 2, np.float64, 100_000_000),
    ("cub3-64-f64", "cubic", "regular", [64] * 3, np.float64, 10_000_000),
    ("cub2-512-f64", "cubic", "regular", [512] * 2, np.float64, 30_000_000),
]


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return float(med), float(q3 - q1)


def run(name, method, kind, shape, dtype, npts, reps, inner):
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
        it = interpn_amd.Interpolator.regular(method, shape, starts, steps, vals, linearize_extrapolation=True, dtype=dtype)
    else:
        it = interpn_amd.Interpolator.rectilinear(method, grids, vals, linearize_extrapolation=True, dtype=dtype)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    pts = torch.rand((npts, n), dtype=tdt, device="cuda:0", generator=gen) * 2.04 - 1.02
    cols = [pts[:, d].contiguous() for d in range(n)]
    out = torch.empty(npts, dtype=tdt, device="cuda:0")
    grad = torch.empty((npts, n), dtype=tdt, device="cuda:0")
    grad_cm = torch.empty((n, npts), dtype=tdt, device="cuda:0")
    column_call = it.eval_cubic_grad_tensors if method == "cubic" else it.eval_grad_tensors
    result = {}

    def points(path, load, store):
        def fn():
            it.set_option("points_path", path)
            it.set_option("points_load", load)
            it.set_option("points_store", store)
            it.eval_points_grad_tensors(pts, out, grad)
            result["grad"] = grad
        return fn

    def f_columns():
        column_call(cols, out, grad_cm)
        result["grad"] = None  # component-major: compared through its transpose below

    def f_transpose():
        t = pts.T.contiguous()
        column_call([t[d] for d in range(n)], out, grad_cm)
        result["grad"] = grad_cm.T.contiguous()

    contenders = [("A_auto", points(0, 0, 0))]
    if method == "linear":
        forms = (1, 2, 3) if (n == 3 and dtype == np.float64) else (1, 3)
        contenders += [(f"A_l{ld}_s{st}", points(1, ld, st)) for ld in forms for st in forms]
    contenders += [("B_columns", f_columns), ("C_transpose", f_transpose), ("D_split", points(2, 0, 0))]
    contenders = tuple(contenders)
    names, paths, ms = {}, {}, {c: [] for c, _ in contenders}
    for label, fn in contenders:
        for _ in range(3):
            fn()
        it.finish()
        names[label] = it.kernel_name()
        paths[label] = it.last_points_path() if label[0] in "AD" else None
    result.clear()
    # every contender computes C's bits, at the size that is timed
    f_transpose()
    it.finish()
    want_out, want_grad = out.clone(), result["grad"].clone()
    same = {}
    for label, fn in contenders:
        out.zero_()
        grad.zero_()
        grad_cm.zero_()
        fn()
        it.finish()
        g = result["grad"] if result["grad"] is not None else grad_cm.T
        same[label] = bool(((out == want_out) | (out.isnan() & want_out.isnan())).all()) and \
            bool(((g == want_grad) | (g.isnan() & want_grad.isnan())).all())
    del want_out, want_grad
    result.clear()
    torch.cuda.empty_cache()
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
    it.close()
    row = {"workload": name, "method": method, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "points": npts,
           "reps": reps, "inner": inner, "kernels": names, "points_paths": paths, "bits_equal_C": same,
           "stream_bytes_per_point": {"A_fused": (2 * n + 1) * elem, "B_columns": (2 * n + 1) * elem,
                                      "C_transpose": (6 * n + 1) * elem, "D_split": (6 * n + 1) * elem}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "gpoints_per_s": round(npts / (med * 1e-3) / 1e9, 2)}
    a, b, c, d = row["A_auto"], row["B_columns"], row["C_transpose"], row["D_split"]
    row["A_below_C_by_more_than_both_iqrs"] = bool(a["ms"] + a["iqr_ms"] + c["iqr_ms"] < c["ms"])
    row["ratio_A_over_C"] = round(a["ms"] / c["ms"], 3)
    row["ratio_A_over_D"] = round(a["ms"] / d["ms"], 3)
    row["ratio_A_over_B"] = round(a["ms"] / b["ms"], 3)
    row["A_above_B_by_more_than_both_iqrs"] = bool(a["ms"] > b["ms"] + a["iqr_ms"] + b["iqr_ms"])
    forced = {k2: v["ms"] for k2, v in row.items() if k2.startswith("A_l")}
    if forced:
        row["fastest_forced_form"] = min(forced, key=forced.get)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_grad_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--small", type=int, default=1_000_000, help="second batch size of the multilinear rows (0: none)")
    ap.add_argument("--only", default="", help="comma-separated workload names")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_points_grad.py needs a GPU: nothing is measured without one")
    only = [s for s in a.only.split(",") if s]
    rows = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for w in WORKLOADS:
        if only and w[0] not in only:
            continue
        sizes = [w[5]] + ([a.small] if w[1] == "linear" and a.small else [])
        for npts in sizes:
            row = run(*w[:5], npts, a.reps, a.inner)
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
            doc = {"tool": "tools/bench_points_grad.py", "device": torch.cuda.get_device_name(0),
                   "method": "HIP events around `inner` evaluations, 3 warm-up evaluations per contender, contenders alternated in "
                             "one process on one handle with rotating order, median and IQR of ms per evaluation",
                   "baseline": "C_transpose", "rows": rows}
            with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
