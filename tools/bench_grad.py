#!/usr/bin/env python3
"""Value-and-gradient evaluation against the same handle's plain evaluation on the same device-resident, unordered points.

    python tools/bench_grad.py --out profiles/grad_bench.json [--reps 21] [--points 100000000] [--only lin3-64-f64]

Method (DESIGN.md "Gradients"): coordinates drawn on the device (uniform over the grid widened by 2 %, no order), HIP events
around `--inner` back-to-back evaluations, 3 warm-up evaluations per contender, then `--reps` rounds that ALTERNATE the
contenders on one handle in one process, their order rotating from round to round, so that clock and cache state drift hit
all of them alike.  Median and inter-quartile range per contender, in ms per evaluation.

Contenders
  grad          eval_grad_tensors: value and N gradient components, one kernel
  eval_onepass  eval_tensors with option sweep = 0: the one-pass value kernel, the like-for-like comparison
  eval_auto     eval_tensors on the automatic path (large 3-D / 2-D batches: the sweep kernel)
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, kind, grid shape, dtype
WORKLOADS = [
    ("lin3-64-f64", "regular", [64] * 3, np.float64),
    ("lin3-64-f64-rect", "rectilinear", [64] * 3, np.float64),
    ("lin3-64-f32", "regular", [64] * 3, np.float32),
    ("lin3-64-f32-rect", "rectilinear", [64] * 3, np.float32),
    ("lin2-1000-f64", "regular", [1000] * 2, np.float64),
]


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
        it = interpn_amd.Interpolator.regular("linear", shape, starts, steps, vals, dtype=dtype)
    else:
        it = interpn_amd.Interpolator.rectilinear("linear", grids, vals, dtype=dtype)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    obs = [(torch.rand(npts, dtype=tdt, device="cuda:0", generator=gen) * 2.04 - 1.02) for _ in range(n)]
    out = torch.empty(npts, dtype=tdt, device="cuda:0")
    grad = torch.empty((n, npts), dtype=tdt, device="cuda:0")

    def f_grad():
        it.eval_grad_tensors(obs, out, grad)

    def f_onepass():
        it.set_option("sweep", 0)
        it.eval_tensors(obs, out)

    def f_auto():
        it.set_option("sweep", -1)
        it.eval_tensors(obs, out)

    contenders = (("grad", f_grad), ("eval_onepass", f_onepass), ("eval_auto", f_auto))
    names, ms = {}, {c: [] for c, _ in contenders}
    for label, fn in contenders:
        for _ in range(3):
            fn()
        it.finish()
        names[label] = it.kernel_name()
    # the value next to the gradient is the plain evaluation's, at the size that is timed
    f_onepass()
    it.finish()
    plain = out.clone()
    f_grad()
    it.finish()
    same = bool(((out == plain) | (out.isnan() & plain.isnan())).all())
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
           "inner": inner, "kernels": names, "table_bytes": table[0], "value_bits_equal_eval": same,
           "stream_bytes_per_point": {"eval": (n + 1) * elem, "grad": (2 * n + 1) * elem,
                                      "ratio": round((2 * n + 1) / (n + 1), 3)}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "gpoints_per_s": round(npts / (med * 1e-3) / 1e9, 2)}
    row["grad"]["stream_tb_per_s"] = round(npts * (2 * n + 1) * elem / (row["grad"]["ms"] * 1e-3) / 1e12, 3)
    row["eval_onepass"]["stream_tb_per_s"] = round(npts * (n + 1) * elem / (row["eval_onepass"]["ms"] * 1e-3) / 1e12, 3)
    row["ratio_grad_over_eval_onepass"] = round(row["grad"]["ms"] / row["eval_onepass"]["ms"], 3)
    row["ratio_grad_over_eval_auto"] = round(row["grad"]["ms"] / row["eval_auto"]["ms"], 3)
    # finite differences: N + 1 evaluations (and lose about half the digits)
    row["ratio_finite_differences_over_grad"] = round((n + 1) * row["eval_auto"]["ms"] / row["grad"]["ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_grad.py needs a GPU: nothing is measured without one")
    only = [s for s in a.only.split(",") if s]
    rows = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for w in WORKLOADS:
        if only and w[0] not in only:
            continue
        row = run(*w, a.points, a.reps, a.inner)
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        doc = {"tool": "tools/bench_grad.py", "device": torch.cuda.get_device_name(0),
               "method": "HIP events around `inner` evaluations, 3 warm-up evaluations per contender, contenders alternated in one "
                         "process on one handle with rotating order, median and IQR of ms per evaluation",
               "baseline": "eval_onepass", "rows": rows}
        with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
