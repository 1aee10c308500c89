#!/usr/bin/env python3
"""Point-major evaluation (an (n, N) tensor of points) against what a caller had to do before it existed.

    python tools/bench_points.py --out profiles/points_bench.json [--reps 21] [--points 100000000,1000000] [--only lin3-64-f64]

Method (the protocol of section 11): points drawn on the device (uniform over the grid widened by
2 %, no order), HIP events around `--inner` back-to-back evaluations, 3 warm-up evaluations per contender, then `--reps`
rounds that ALTERNATE the contenders on one handle in one process, their order rotating from round to round.  Median and
inter-quartile range per contender, in ms per evaluation.

Contenders
  A_auto        eval_points_tensors, automatic path and load form
  A_wide        ... the fused kernel with per-lane vector loads (option points_load = 1)
  A_lds         ... with the wave's span through LDS (points_load = 2; 3-D f64 only)
  A_elem        ... with element loads (points_load = 3: what a strided or misaligned block gets)
  B_columns     eval_tensors with sweep = 0 on pre-split columns: the like-for-like one-pass kernel, equal bytes per point
  C_transpose   what a user does today, timed together: pts.T.contiguous(), then automatic eval_tensors
  D_split       eval_points_tensors with points_path = 2: de-interleave slices on the device, automatic evaluation
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, method, kind, grid shape, dtype
WORKLOADS = [
    ("lin3-64-f64", "linear", "regular", [64] * 3, np.float64),
    ("lin3-64-f64-rect", "linear", "rectilinear", [64] * 3, np.float64),
    ("lin3-64-f32", "linear", "regular", [64] * 3, np.float32),
    ("lin2-1000-f64", "linear", "regular", [1000] * 2, np.float64),
    ("cub3-64-f64", "cubic", "regular", [64] * 3, np.float64),
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
        it = interpn_amd.Interpolator.regular(method, shape, starts, steps, vals, dtype=dtype)
    else:
        it = interpn_amd.Interpolator.rectilinear(method, grids, vals, dtype=dtype)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    pts = torch.rand((npts, n), dtype=tdt, device="cuda:0", generator=gen) * 2.04 - 1.02
    cols = [pts[:, d].contiguous() for d in range(n)]
    out = torch.empty(npts, dtype=tdt, device="cuda:0")
    fused = method == "linear" and n in (2, 3)

    def points(path, load):
        def fn():
            it.set_option("sweep", -1)
            it.set_option("points_path", path)
            it.set_option("points_load", load)
            it.eval_points_tensors(pts, out)
        return fn

    def f_columns():
        it.set_option("sweep", 0)
        it.eval_tensors(cols, out)

    def f_transpose():
        it.set_option("sweep", -1)
        t = pts.T.contiguous()
        it.eval_tensors([t[d] for d in range(n)], out)

    contenders = [("A_auto", points(0, 0))]
    if fused:
        contenders += [("A_wide", points(1, 1)), ("A_elem", points(1, 3))]
        if n == 3 and dtype == np.float64:
            contenders.append(("A_lds", points(1, 2)))
        contenders.append(("B_columns", f_columns))
    contenders += [("C_transpose", f_transpose), ("D_split", points(2, 0))]
    contenders = tuple(contenders)
    names, paths, ms = {}, {}, {c: [] for c, _ in contenders}
    for label, fn in contenders:
        for _ in range(3):
            fn()
        it.finish()
        names[label] = it.kernel_name()
        paths[label] = it.last_points_path() if label[0] in "AD" else None
    # every contender computes the same bits, at the size that is timed
    f_transpose()
    it.finish()
    plain = out.clone()
    same = {}
    for label, fn in contenders:
        out.zero_()
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
    it.close()
    row = {"workload": name, "method": method, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "points": npts,
           "reps": reps, "inner": inner, "kernels": names, "points_paths": paths, "bits_equal_transpose_then_eval": same,
           "stream_bytes_per_point": {"A_fused": (n + 1) * elem, "B_columns": (n + 1) * elem, "C_transpose": (3 * n + 1) * elem,
                                      "D_split": (3 * n + 1) * elem}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "gpoints_per_s": round(npts / (med * 1e-3) / 1e9, 2)}
    a, c, d = row["A_auto"], row["C_transpose"], row["D_split"]
    row["A_below_C_by_more_than_both_iqrs"] = bool(a["ms"] + a["iqr_ms"] + c["iqr_ms"] < c["ms"])
    row["ratio_A_over_C"] = round(a["ms"] / c["ms"], 3)
    row["ratio_A_over_D"] = round(a["ms"] / d["ms"], 3)
    if fused:
        b = row["B_columns"]
        row["ratio_A_over_B"] = round(a["ms"] / b["ms"], 3)
        row["A_above_B_by_more_than_both_iqrs"] = bool(a["ms"] > b["ms"] + a["iqr_ms"] + b["iqr_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--points", default="100000000,1000000", help="comma-separated batch sizes")
    ap.add_argument("--only", default="", help="comma-separated workload names")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_points.py needs a GPU: nothing is measured without one")
    only = [s for s in a.only.split(",") if s]
    rows = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for npts in [int(s) for s in a.points.split(",") if s]:
        for w in WORKLOADS:
            if only and w[0] not in only:
                continue
            row = run(*w, npts, a.reps, a.inner)
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
            doc = {"tool": "tools/bench_points.py", "device": torch.cuda.get_device_name(0),
                   "method": "HIP events around `inner` evaluations, 3 warm-up evaluations per contender, contenders alternated in "
                             "one process on one handle with rotating order, median and IQR of ms per evaluation",
                   "baseline": "C_transpose", "rows": rows}
            with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
