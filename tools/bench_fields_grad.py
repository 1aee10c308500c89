#!/usr/bin/env python3
"""Field-set gradients: one fused call (K values and the K x N Jacobian) against K single-handle gradient calls.

    python tools/bench_fields_grad.py --out profiles/fields_grad_bench.json [--reps 21] [--only 64f64]

Method: device-resident unordered points (uniform over the grid widened by 2 % on each side), HIP events around one
evaluation, 3 warm-up evaluations per contender, then `--reps` rounds that ALTERNATE the contenders in one process, their
order rotating from round to round, so that clock and cache state drift, and whatever ran just before, hit all of them
alike.  Contenders:
    handles    K `Interpolator.eval_grad_tensors` calls on K ordinary handles, into slices of the same output blocks — what a
               caller without this feature writes, and what the parent commit can run; the baseline of every ratio
    fused      `Fields.eval_grad_tensors` with option fused = 1: one launch of k_linear_fields_grad
    per_field  the same with fused = 0: the set's own K handles
    auto       the same with fused = -1: what the set picks by itself
Before anything is timed, every contender's values and Jacobian are compared with the `handles` contender's at the timed
size, bit for bit; a difference ends the run.  Per row: median and inter-quartile range in ms, the ratios against `handles`,
and the algorithmic stream bytes per point computed from the shapes (coordinates in, values and components out)."""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, kind, shape, dtype, fields.  f32 K = 2, 5 and 2-D K = 2 are the rows whose table lines are less than 3/4 full
# (4 K < 3 ceil(K / P) P): the class the line-fill rule of the automatic choice sends to the per-field path.
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
        handles = [interpn_amd.Interpolator.regular("linear", shape, starts, steps, vals[f], dtype=dtype) for f in range(k)]
    else:
        fs = interpn_amd.Fields.rectilinear("linear", grids, vals, dtype=dtype)
        handles = [interpn_amd.Interpolator.rectilinear("linear", grids, vals[f], dtype=dtype) for f in range(k)]
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1234 + k)
    obs = [(torch.rand(npts, dtype=tdt, device="cuda:0", generator=gen) * 2.08 - 1.04) for _ in range(n)]
    out = torch.empty((k, npts), dtype=tdt, device="cuda:0")
    grad = torch.empty((k, n, npts), dtype=tdt, device="cuda:0")

    def by_handles():
        for f in range(k):
            handles[f].eval_grad_tensors(obs, out[f], grad[f])

    def by_set(opt):
        def call():
            fs.set_option("fused", opt)
            fs.eval_grad_tensors(obs, out, grad)
        return call

    contenders = (("handles", by_handles), ("fused", by_set(1)), ("per_field", by_set(0)), ("auto", by_set(-1)))
    names, took, ms = {}, {}, {c: [] for c, _ in contenders}
    want_out = want_grad = None
    for label, call in contenders:
        out.zero_()
        grad.zero_()
        for _ in range(3):
            call()
        for h in handles:
            h.finish()
        fs.finish()
        if label == "handles":
            want_out, want_grad = out.clone(), grad.clone()
            names[label] = handles[0].kernel_name()
        else:
            names[label] = fs.kernel_name()
            took[label] = fs.last_path
            # bits, NaN-free data: integer views compare every bit
            itype = torch.int64 if dtype == np.float64 else torch.int32
            if not (torch.equal(out.view(itype), want_out.view(itype)) and torch.equal(grad.view(itype), want_grad.view(itype))):
                raise SystemExit(f"{name} K={k}: {label} differs from the K single handles")
    del want_out, want_grad
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    m = len(contenders)
    for rep in range(reps):
        for label, call in contenders[rep % m:] + contenders[:rep % m]:  # rotate: what ran just before evens out
            start.record()
            call()
            stop.record()
            stop.synchronize()
            ms[label].append(start.elapsed_time(stop))
    for h in handles:
        h.finish()
        h.close()
    fs.finish()
    per_line, lines, table_bytes = interpn_amd.fields_layout(dtype, shape, k)
    fs.close()
    row = {"workload": name, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "points": npts, "fields": k,
           "fields_per_line": per_line, "lines_per_point": lines, "lines_less_than_three_quarters_full": bool(4 * k < 3 * lines * per_line),
           "fused_table_bytes": table_bytes, "reps": reps,
           "auto_takes": took["auto"], "kernels": names, "bits_equal_to_handles": True,
           "stream_bytes_per_point": {"handles": (n + (n + 1)) * k * elem, "fused": (n + (n + 1) * k) * elem}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4)}
    for label in ("fused", "per_field", "auto"):
        row[f"ratio_handles_over_{label}"] = round(row["handles"]["ms"] / row[label]["ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_grad_bench.json"))
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
    doc = {"tool": "tools/bench_fields_grad.py", "device": torch.cuda.get_device_name(0),
           "method": "HIP events, 3 warm-up evaluations per contender, contenders alternated in one process, median and IQR; "
                     "every contender bit-equal to K single-handle calls before timing",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
