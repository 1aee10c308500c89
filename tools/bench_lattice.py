#!/usr/bin/env python3
"""Lattice evaluation: the fused row kernel against the expanded path and against what a user did before —
`torch.meshgrid` + `eval_tensors` — on one handle in one process.

    python tools/bench_lattice.py --out profiles/lattice_bench.json [--reps 21] [--only lin3-64to464-f64]

Method: device-resident coordinate vectors, HIP events around one evaluation, 3 warm-up evaluations
per contender, then `--reps` rounds that ALTERNATE the contenders on the same handle, their order rotating from round to
round, so that clock and cache state drift, and whatever ran just before, hit all of them alike.  Median and
inter-quartile range per contender, in ms.

Contenders
  fused          option lattice = 1: k_lattice_axes + k_lattice_rows
  expanded       option lattice = 0: k_lattice_expand into scratch + the handle's ordinary evaluation, slice by slice
  auto           option lattice = -1: what the handle picks by itself
  meshgrid_eval  the baseline: torch.meshgrid(indexing="ij") + reshape + contiguous (N arrays of all points written) and
                 eval_tensors on them, both inside the timed region
  eval_only      eval_tensors on points expanded beforehand (the expansion left out of the timed region)
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, method, kind, grid shape, dtype, lattice lengths, last axis shuffled
WORKLOADS = [
    ("lin3-64to464-f64", "linear", "regular", [64] * 3, np.float64, [464] * 3, False),
    ("lin3-64to464-f32", "linear", "regular", [64] * 3, np.float32, [464] * 3, False),
    ("lin3-64to464-f64-rect", "linear", "rectilinear", [64] * 3, np.float64, [464] * 3, False),
    ("lin3-64to464-f32-rect", "linear", "rectilinear", [64] * 3, np.float32, [464] * 3, False),
    ("cub3-64to216-f64", "cubic", "regular", [64] * 3, np.float64, [216] * 3, False),
    ("cub3-64to216-f64-rect", "cubic", "rectilinear", [64] * 3, np.float64, [216] * 3, False),
    ("lin2-512to5000-f64", "linear", "regular", [512] * 2, np.float64, [5000] * 2, False),
    ("cub2-512to5000-f64", "cubic", "regular", [512] * 2, np.float64, [5000] * 2, False),
    ("lin3-128to32-f64-down", "linear", "regular", [128] * 3, np.float64, [32] * 3, False),
    ("lin3-64to464-f64-unsorted-last", "linear", "regular", [64] * 3, np.float64, [464] * 3, True),
    # the two layout rules of the automatic choice: few rows, and a last grid axis much longer than the lattice's
    ("lin3-64-few-rows", "linear", "regular", [64] * 3, np.float64, [8, 8, 200_000], False),
    ("lin3-long-grid-axis", "linear", "regular", [64, 64, 600], np.float64, [256, 256, 16], False),
]


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return float(med), float(q3 - q1)


def run(name, method, kind, shape, dtype, lens, shuffle_last, reps):
    import torch

    import interpn_amd

    rng = np.random.default_rng(len(shape) * 100 + len(name))
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
    axes = [np.linspace(-1.02, 1.02, m).astype(dtype) for m in lens]
    if shuffle_last:
        rng.shuffle(axes[-1])
    ax_t = [torch.from_numpy(a).to("cuda:0") for a in axes]
    npts = int(np.prod(lens))
    out = torch.empty(lens, dtype=tdt, device="cuda:0")
    flat = out.reshape(-1)
    points = [t.reshape(-1).contiguous() for t in torch.meshgrid(*ax_t, indexing="ij")]

    def lattice(opt):
        def f():
            it.set_option("lattice", opt)
            it.eval_lattice_tensors(ax_t, out)
        return f

    def meshgrid_eval():
        pts = [t.reshape(-1).contiguous() for t in torch.meshgrid(*ax_t, indexing="ij")]
        it.eval_tensors(pts, flat)

    def eval_only():
        it.eval_tensors(points, flat)

    contenders = (("fused", lattice(1)), ("expanded", lattice(0)), ("auto", lattice(-1)), ("meshgrid_eval", meshgrid_eval),
                  ("eval_only", eval_only))
    names, took, ms = {}, {}, {c: [] for c, _ in contenders}
    for label, fn in contenders:
        for _ in range(3):
            fn()
        it.finish()
        names[label] = it.kernel_name()
        took[label] = it.last_lattice_path if label in ("fused", "expanded", "auto") else it.last_path
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    k = len(contenders)
    for rep in range(reps):
        for label, fn in contenders[rep % k:] + contenders[:rep % k]:  # rotate the order
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ms[label].append(start.elapsed_time(stop))
    it.finish()
    it.close()
    row = {"workload": name, "method": method, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "lattice": lens,
           "points": npts, "last_axis_shuffled": shuffle_last, "reps": reps, "took": took, "kernels": names,
           "planned": interpn_amd.lattice_plan(dtype, method, shape, lens)[0],
           "bytes_per_point_model": {"fused": elem, "per_point_kernels": (n + 1) * elem}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "gpoints_per_s": round(npts / (med * 1e-3) / 1e9, 2)}
    row["fused"]["result_tb_per_s"] = round(npts * elem / (row["fused"]["ms"] * 1e-3) / 1e12, 3)
    row["ratio_meshgrid_eval_over_fused"] = round(row["meshgrid_eval"]["ms"] / row["fused"]["ms"], 2)
    row["ratio_eval_only_over_fused"] = round(row["eval_only"]["ms"] / row["fused"]["ms"], 2)
    row["ratio_expanded_over_fused"] = round(row["expanded"]["ms"] / row["fused"]["ms"], 2)
    faster = min(row["fused"]["ms"], row["expanded"]["ms"])
    spread = max(row["fused"]["iqr_ms"], row["expanded"]["iqr_ms"], row["auto"]["iqr_ms"])
    row["auto_within_spread_of_faster"] = bool(row["auto"]["ms"] <= faster + spread)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    a = ap.parse_args()
    import torch

    only = [s for s in a.only.split(",") if s]
    rows = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for w in WORKLOADS:
        if only and w[0] not in only:
            continue
        row = run(*w, a.reps)
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
        doc = {"tool": "tools/bench_lattice.py", "device": torch.cuda.get_device_name(0),
               "method": "HIP events, 3 warm-up evaluations per contender, contenders alternated in one process on one handle "
                         "with rotating order, median and IQR",
               "baseline": "meshgrid_eval", "rows": rows}
        with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
