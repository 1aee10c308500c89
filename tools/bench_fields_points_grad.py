#!/usr/bin/env python3
"""Point-major field-set gradients: (n, N) points in, (n, K) values and the (n, K, N) Jacobian out, against the chain of
layout passes around the column form.

    python tools/bench_fields_points_grad.py --out profiles/fields_points_grad_bench.json [--reps 21] [--only 64f64]

Method (that of tools/bench_fields_grad.py): device-resident unordered points (uniform over the grid widened by 2 % on each
side) as ONE (n, N) tensor, HIP events around one evaluation, 3 warm-up evaluations per contender, then `--reps` rounds that
ALTERNATE the contenders in one process, their order rotating from round to round, so that clock and cache state drift, and
whatever ran just before, hit all of them alike.  Contenders:
    chain   what a caller without this feature writes: `pts.T.contiguous()`, `Fields.eval_grad_tensors` on the columns,
            `out.T.contiguous()`, `jac.permute(2, 0, 1).contiguous()`; the baseline of every ratio
    split   `Fields.eval_points_grad_tensors` with option points_path = 2: k_split_points, the column form, two k_join_fields
    fused   the same with points_path = 1: one launch of k_linear_fields_points_grad
    auto    the same with points_path = -1: what the set picks by itself
Before anything is timed, every contender's values and Jacobian are compared with the `chain` contender's at the timed size,
bit for bit; a difference ends the run.  Per row: median and inter-quartile range in ms, the ratios against `chain` and of
split over fused, and the algorithmic stream bytes per point computed from the shapes."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, kind, shape, dtype, fields: the workloads of tools/bench_fields_grad.py
WORKLOADS = [
    ("64f64", "regular", [64, 64, 64], np.float64, (2, 3, 8)),
    ("64f64-rect", "rectilinear", [64, 64, 64], np.float64, (2, 3, 8)),
    ("64f32", "regular", [64, 64, 64], np.float32, (2, 3, 4, 5, 8)),
    ("1000x1000f64", "regular", [1000, 1000], np.float64, (2, 4)),
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
    pts = torch.rand((npts, n), dtype=tdt, device="cuda:0", generator=gen) * 2.08 - 1.04
    out = torch.empty((npts, k), dtype=tdt, device="cuda:0")
    jac = torch.empty((npts, k, n), dtype=tdt, device="cuda:0")
    fs.reserve_points_grad(npts)  # the split path's block: made once, outside the timed region
    result = {}

    def chain():
        cols = pts.T.contiguous()
        o, g = fs.eval_grad_tensors(list(cols))
        result["out"], result["jac"] = o.T.contiguous(), g.permute(2, 0, 1).contiguous()

    def by_path(opt):
        def call():
            fs.set_option("points_path", opt)
            fs.eval_points_grad_tensors(pts, out, jac)
            result["out"], result["jac"] = out, jac
        return call

    contenders = (("chain", chain), ("split", by_path(2)), ("fused", by_path(1)), ("auto", by_path(-1)))
    names, took, ms = {}, {}, {c: [] for c, _ in contenders}
    want_out = want_jac = None
    itype = torch.int64 if dtype == np.float64 else torch.int32
    for label, call in contenders:
        out.zero_()
        jac.zero_()
        for _ in range(3):
            call()
        fs.finish()
        names[label] = fs.kernel_name()
        if label == "chain":
            want_out, want_jac = result["out"].clone(), result["jac"].clone()
        else:
            took[label] = fs.last_points_path
            # bits, NaN-free data: integer views compare every bit
            if not (torch.equal(result["out"].view(itype), want_out.view(itype))
                    and torch.equal(result["jac"].view(itype), want_jac.view(itype))):
                raise SystemExit(f"{name} K={k}: {label} differs from the chain around the column form")
    del want_out, want_jac
    result.clear()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    m = len(contenders)
    for rep in range(reps):
        for label, call in contenders[rep % m:] + contenders[:rep % m]:  # rotate: what ran just before evens out
            start.record()
            call()
            stop.record()
            stop.synchronize()
            ms[label].append(start.elapsed_time(stop))
    fs.finish()
    per_line, lines, table_bytes = interpn_amd.fields_layout(dtype, shape, k)
    fs.close()
    stream = n + k + k * n  # elements per point of one evaluation
    row = {"workload": name, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "points": npts, "fields": k,
           "fields_per_line": per_line, "lines_per_point": lines, "fused_table_bytes": table_bytes, "reps": reps,
           "auto_takes": took["auto"], "paths": took, "kernels": names, "bits_equal_to_chain": True,
           "stream_bytes_per_point": {"chain": 3 * stream * elem, "split": 3 * stream * elem, "fused": stream * elem}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4)}
    for label in ("split", "fused", "auto"):
        row[f"ratio_{label}_over_chain"] = round(row[label]["ms"] / row["chain"]["ms"], 3)
    row["ratio_fused_over_split"] = round(row["fused"]["ms"] / row["split"]["ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_points_grad_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    a = ap.parse_args()
    import torch

    only = [s for s in a.only.split(",") if s]
    rows = []
    for name, kind, shape, dtype, fields in WORKLOADS:
        if only and name not in only:
            continue
        for k in fields:
            row = run(name, kind, shape, dtype, a.points, k, a.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    doc = {"tool": "tools/bench_fields_points_grad.py", "device": torch.cuda.get_device_name(0),
           "method": "HIP events, 3 warm-up evaluations per contender, contenders alternated in one process, median and IQR; "
                     "every contender bit-equal to transpose + column form + two transposes before timing",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
