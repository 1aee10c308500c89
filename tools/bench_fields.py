#!/usr/bin/env python3
"""Field sets: the fused kernel against K runs of the single-field kernels, on one set in one process.

    python tools/bench_fields.py --out profiles/fields_bench.json [--reps 21] [--only 64f64]

Method: device-resident unordered points (uniform over the grid widened by 2 % on each side), HIP events around one
evaluation, 3 warm-up evaluations per path, then `--reps` rounds that ALTERNATE the paths — fused = 1, fused = 0 and
fused = -1 (what the set picks by itself) on the same set, their order rotating from round to round — so that clock
and cache state drift, and whatever ran just before, hit all of them alike.
The fused = 0 path runs the unchanged single-field kernels through K ordinary handles: it is the cost of K calls and the
baseline of every ratio.  Per row: median and inter-quartile range of each path in ms, the ratio per-field / fused, the
algorithmic bytes per point computed from the shapes (coordinates + results + whole table lines), TB/s and the share of
the 8 TB/s HBM peak, and the kernel names."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0

# name, kind, shape, dtype, points
WORKLOADS = [
    ("64f64", "regular", [64, 64, 64], np.float64, 100_000_000),
    ("64f64-small", "regular", [64, 64, 64], np.float64, 4_000_000),
    ("64f32", "regular", [64, 64, 64], np.float32, 100_000_000),
    ("64f32-small", "regular", [64, 64, 64], np.float32, 4_000_000),
    ("128f64", "regular", [128, 128, 128], np.float64, 100_000_000),
    ("64f64-rect", "rectilinear", [64, 64, 64], np.float64, 100_000_000),
    ("1000x1000f64", "regular", [1000, 1000], np.float64, 30_000_000),
]


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return float(med), float(q3 - q1)


def run(name, kind, shape, dtype, npts, k, reps):
    import torch

    import interpn_amd

    rng = np.random.default_rng(len(shape) * 100 + k)
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
    vals = rng.uniform(-1.0, 1.0, (k, int(np.prod(shape)))).astype(dtype)
    if kind == "regular":
        starts = np.array([g[0] for g in grids], dtype=dtype)
        steps = np.array([g[1] - g[0] for g in grids], dtype=dtype)
        fs = interpn_amd.Fields.regular("linear", shape, starts, steps, vals, dtype=dtype)
    else:
        fs = interpn_amd.Fields.rectilinear("linear", grids, vals, dtype=dtype)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1234 + k)
    obs = [(torch.rand(npts, dtype=tdt, device="cuda:0", generator=gen) * 2.08 - 1.04) for _ in range(n)]
    out = torch.empty((k, npts), dtype=tdt, device="cuda:0")
    paths = (("fused", 1), ("per_field", 0), ("auto", -1))
    names, took, ms = {}, {}, {p: [] for p, _ in paths}
    for label, opt in paths:
        fs.set_option("fused", opt)
        for _ in range(3):
            fs.eval_tensors(obs, out)
        fs.finish()
        names[label] = fs.kernel_name()
        took[label] = fs.last_path
    per_line, lines, table_bytes = interpn_amd.fields_layout(dtype, shape, k)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps):
        for label, opt in paths[rep % 3:] + paths[:rep % 3]:  # rotate: what ran just before (cache and clock state) evens out
            fs.set_option("fused", opt)
            start.record()
            fs.eval_tensors(obs, out)
            stop.record()
            stop.synchronize()
            ms[label].append(start.elapsed_time(stop))
    fs.finish()
    per_field_table = fs.get_option("sweep_table_bytes")
    fs.close()
    bytes_fused = n * elem + k * elem + lines * 128
    bytes_per_field = k * (n * elem + elem + 128)
    row = {"workload": name, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "points": npts, "fields": k,
           "fields_per_line": per_line, "lines_per_point": lines, "fused_table_bytes": table_bytes,
           "per_field_sweep_table_bytes": per_field_table, "reps": reps, "auto_takes": took["auto"], "kernels": names,
           "bytes_per_point": {"fused": bytes_fused, "per_field": bytes_per_field}}
    for label, _ in paths:
        med, iqr = quartiles(ms[label])
        b = bytes_per_field if took[label] == "per_field" else bytes_fused
        tbs = b * npts / (med * 1e-3) / 1e12
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "tb_per_s": round(tbs, 3), "share_of_peak": round(tbs / PEAK_TBS, 3)}
    row["ratio_per_field_over_fused"] = round(row["per_field"]["ms"] / row["fused"]["ms"], 3)
    faster = min(row["fused"]["ms"], row["per_field"]["ms"])
    spread = max(row["fused"]["iqr_ms"], row["per_field"]["iqr_ms"], row["auto"]["iqr_ms"])
    row["auto_within_spread_of_faster"] = bool(row["auto"]["ms"] <= faster + spread)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    ap.add_argument("--fields", default="2,4,8")
    a = ap.parse_args()
    import torch

    only = [s for s in a.only.split(",") if s]
    rows = []
    for name, kind, shape, dtype, npts in WORKLOADS:
        if only and name not in only:
            continue
        for k in [int(s) for s in a.fields.split(",")]:
            row = run(name, kind, shape, dtype, npts, k, a.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    doc = {"tool": "tools/bench_fields.py", "device": torch.cuda.get_device_name(0), "peak_tb_per_s": PEAK_TBS,
           "method": "HIP events, 3 warm-up evaluations per path, paths alternated in one process on one set, median and IQR",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
