#!/usr/bin/env python3
"""Point-major field sets: (n, N) points in, (n, K) values out, against what a caller had before them.

    python tools/bench_fields_points.py --out profiles/fields_points_bench.json [--reps 21] [--only 64f64] [--fields 2,3,4,8]

Method (that of tools/bench_fields.py): device-resident unordered points (uniform over the grid widened by 2 % on each
side), HIP events around one evaluation, 3 warm-up evaluations per variant, then `--reps` rounds that ALTERNATE the
variants on one set in one process, their order rotating from round to round; median and inter-quartile range in ms.

Variants per row:
  fused     points_path = 1: one launch of k_linear_fields_points
  split     points_path = 2: k_split_points, the column form (fused = -1), k_join_fields, per slice
  auto      points_path = -1
  baseline  what a caller has without the point-major form: pts.T.contiguous(), Fields.eval_tensors with fused = -1,
            out.T.contiguous() — both temporaries preallocated, the copies made by torch
  columns   k_linear_fields (fused = 1) on the already de-interleaved columns into (K, n) rows: not an alternative for a
            caller who holds rows, but the kernel the fused variant shares its body with
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, kind, shape, dtype
WORKLOADS = [
    ("64f64", "regular", [64, 64, 64], np.float64),
    ("64f32", "regular", [64, 64, 64], np.float32),
    ("128f64", "regular", [128, 128, 128], np.float64),
    ("128f32", "regular", [128, 128, 128], np.float32),
    ("64f64-rect", "rectilinear", [64, 64, 64], np.float64),
    ("1000x1000f64", "regular", [1000, 1000], np.float64),
]
VARIANTS = ("fused", "split", "auto", "baseline", "columns")


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return float(med), float(q3 - q1)


def make_set(kind, shape, dtype, k):
    import interpn_amd

    rng = np.random.default_rng(len(shape) * 100 + k)
    grids = []
    for d in range(len(shape)):
        g = np.linspace(-1.0, 1.0, shape[d])
        if kind == "rectilinear":
            j = (rng.random(g.size) - 0.5) * 0.5 * (g[1] - g[0])
            j[0] = j[-1] = 0.0
            g = g + j
        grids.append(g.astype(dtype))
    vals = rng.uniform(-1.0, 1.0, (k, int(np.prod(shape)))).astype(dtype)
    if kind == "regular":
        starts = np.array([g[0] for g in grids], dtype=dtype)
        steps = np.array([g[1] - g[0] for g in grids], dtype=dtype)
        return interpn_amd.Fields.regular("linear", shape, starts, steps, vals, dtype=dtype)
    return interpn_amd.Fields.rectilinear("linear", grids, vals, dtype=dtype)


def run(name, kind, shape, dtype, npts, k, reps):
    import torch

    import interpn_amd

    n = len(shape)
    elem = np.dtype(dtype).itemsize
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fs = make_set(kind, shape, dtype, k)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1234 + k)
    pts = torch.rand((npts, n), dtype=tdt, device="cuda:0", generator=gen) * 2.08 - 1.04
    out = torch.empty((npts, k), dtype=tdt, device="cuda:0")
    cols = torch.empty((n, npts), dtype=tdt, device="cuda:0")   # the baseline's temporaries, and the columns variant's input
    rows = torch.empty((k, npts), dtype=tdt, device="cuda:0")
    col_list = [cols[d] for d in range(n)]

    def fused():
        fs.set_option("points_path", 1)
        fs.eval_points_tensors(pts, out)

    def split():
        fs.set_option("points_path", 2)
        fs.set_option("fused", -1)
        fs.eval_points_tensors(pts, out)

    def auto():
        fs.set_option("points_path", -1)
        fs.set_option("fused", -1)
        fs.eval_points_tensors(pts, out)

    def baseline():
        fs.set_option("fused", -1)
        cols.copy_(pts.T)
        fs.eval_tensors(col_list, rows)
        out.copy_(rows.T)

    def columns():
        fs.set_option("fused", 1)
        fs.eval_tensors(col_list, rows)

    calls = {"fused": fused, "split": split, "auto": auto, "baseline": baseline, "columns": columns}
    took, kernels, ms = {}, {}, {v: [] for v in VARIANTS}
    for v in VARIANTS:
        for _ in range(3):
            calls[v]()
        fs.finish()
        kernels[v] = fs.kernel_name()
        took[v] = {"points_path": fs.last_points_path if v in ("fused", "split", "auto") else None, "columns_path": fs.last_path}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    order = list(VARIANTS)
    for rep in range(reps):
        r = rep % len(order)
        for v in order[r:] + order[:r]:  # rotate: what ran just before (cache and clock state) evens out
            start.record()
            calls[v]()
            stop.record()
            stop.synchronize()
            ms[v].append(start.elapsed_time(stop))
    fs.finish()
    fs.close()
    per_line, lines, table_bytes = interpn_amd.fields_layout(dtype, shape, k)
    row = {"workload": name, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "points": npts, "fields": k,
           "fields_per_line": per_line, "lines_per_point": lines, "fused_table_bytes": table_bytes, "reps": reps,
           "took": took, "kernels": kernels,
           "bytes_per_point": {"fused": (n + k) * elem + lines * 128, "baseline_extra": 2 * (n + k) * elem}}
    for v in VARIANTS:
        med, iqr = quartiles(ms[v])
        row[v] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4)}
    row["fused_over_split"] = round(row["fused"]["ms"] / row["split"]["ms"], 3)
    row["auto_over_baseline"] = round(row["auto"]["ms"] / row["baseline"]["ms"], 3)
    row["fused_over_columns"] = round(row["fused"]["ms"] / row["columns"]["ms"], 3)
    row["auto_not_slower_than_baseline"] = bool(row["auto"]["ms"] <= row["baseline"]["ms"] + row["auto"]["iqr_ms"] + row["baseline"]["iqr_ms"])
    faster = "fused" if row["fused"]["ms"] <= row["split"]["ms"] else "split"
    row["faster_of_fused_and_split"] = faster
    row["auto_takes_the_faster"] = bool(took["auto"]["points_path"] == faster or
                                        abs(row["fused"]["ms"] - row["split"]["ms"]) <= row["fused"]["iqr_ms"] + row["split"]["iqr_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_points_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    ap.add_argument("--fields", default="2,3,4,8")
    ap.add_argument("--points", default="4000000,100000000")
    a = ap.parse_args()
    import torch

    only = [s for s in a.only.split(",") if s]
    rows = []
    doc = {"tool": "tools/bench_fields_points.py", "device": torch.cuda.get_device_name(0),
           "method": "HIP events, 3 warm-up evaluations per variant, variants alternated in one process on one set with rotating "
                     "order, median and IQR of --reps",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, kind, shape, dtype in WORKLOADS:
        if only and name not in only:
            continue
        for npts in [int(s) for s in a.points.split(",")]:
            for k in [int(s) for s in a.fields.split(",")]:
                row = run(name, kind, shape, dtype, npts, k, a.reps)
                rows.append(row)
                print(json.dumps({key: row[key] for key in ("workload", "points", "fields", "fused", "split", "auto", "baseline", "columns",
                                                            "fused_over_split", "auto_over_baseline", "fused_over_columns")}), flush=True)
                torch.cuda.empty_cache()
                with open(a.out, "w") as f:  # after every row: a run that is cut short leaves what it measured
                    json.dump(doc, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
