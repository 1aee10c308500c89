#!/usr/bin/env python3
"""Gradients on a lattice: the fused row kernel against the library's expanded path and against what a user had before it —
`eval_grad_tensors` / `eval_cubic_grad_tensors` on pre-expanded device coordinates — on one handle in one process.

    python tools/bench_lattice_grad.py --out profiles/lattice_grad_bench.json [--reps 21] [--only lin3-64to464-f64]

Method (the protocol of tools/bench_grad.py and tools/bench_lattice.py): device-resident coordinate
vectors, HIP events around one evaluation, 3 warm-up evaluations per contender, then `--reps` rounds that ALTERNATE the
contenders on the same handle, their order rotating from round to round.  Median and inter-quartile range per contender,
in ms.  Before anything is timed the fused results are compared bit for bit with the baseline's at the timed size.

Contenders
  fused      option lattice = 1: k_lattice_axes + k_lattice_grad_rows
  expanded   option lattice = 0: k_lattice_expand into scratch + the handle's per-point gradient kernel, slice by slice
  auto       option lattice = -1: what the handle picks by itself
  baseline   the per-point gradient kernel on points expanded beforehand (the expansion left out of the timed region)
  expansion  torch.meshgrid(indexing="ij") + reshape + contiguous alone: what the baseline's user pays on top
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, method, kind, grid shape, dtype, lattice lengths, options
WORKLOADS = [
    ("lin3-64to464-f64", "linear", "regular", [64] * 3, np.float64, [464] * 3, {}),
    ("lin3-64to464-f32", "linear", "regular", [64] * 3, np.float32, [464] * 3, {}),
    ("lin3-64to464-f64-rect", "linear", "rectilinear", [64] * 3, np.float64, [464] * 3, {}),
    ("cub3-64to216-f64", "cubic", "regular", [64] * 3, np.float64, [216] * 3, {}),
    ("cub3-64to216-f64-rect", "cubic", "rectilinear", [64] * 3, np.float64, [216] * 3, {}),
    # three lines of 1000 f64 per wave are 93.75 KiB per workgroup: beyond the default budget and beyond the option's
    # largest value, 60 KiB, so in both rows "fused" (= wherever it fits) takes the expanded path; 640 is the longest last
    # grid axis a 2-D f64 multilinear call fuses at 60 KiB
    ("lin2-1000to4000-f64-lds60", "linear", "regular", [1000] * 2, np.float64, [4000] * 2, {"axis_lds_kb": 60}),
    ("lin2-1000to4000-f64-default", "linear", "regular", [1000] * 2, np.float64, [4000] * 2, {}),
    ("lin2-640to4000-f64-lds60", "linear", "regular", [640] * 2, np.float64, [4000] * 2, {"axis_lds_kb": 60}),
]


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return float(med), float(q3 - q1)


def run(name, method, kind, shape, dtype, lens, options, reps):
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
    for key, value in options.items():
        it.set_option(key, value)
    axes = [np.linspace(-1.02, 1.02, m).astype(dtype) for m in lens]
    ax_t = [torch.from_numpy(a).to("cuda:0") for a in axes]
    npts = int(np.prod(lens))
    out = torch.empty(lens, dtype=tdt, device="cuda:0")
    grad = torch.empty([n] + list(lens), dtype=tdt, device="cuda:0")
    points = [t.reshape(-1).contiguous() for t in torch.meshgrid(*ax_t, indexing="ij")]
    base_out = torch.empty(npts, dtype=tdt, device="cuda:0")
    base_grad = torch.empty((n, npts), dtype=tdt, device="cuda:0")
    per_point = it.eval_cubic_grad_tensors if method == "cubic" else it.eval_grad_tensors

    def lattice(opt):
        def f():
            it.set_option("lattice", opt)
            it.eval_lattice_grad_tensors(ax_t, out, grad)
        return f

    def baseline():
        per_point(points, base_out, base_grad)

    def expansion():
        return [t.reshape(-1).contiguous() for t in torch.meshgrid(*ax_t, indexing="ij")]

    # the same bits at the timed size, before anything is timed
    lattice(1)()
    baseline()
    it.finish()
    fused_path = it.last_lattice_path
    bits_equal = bool(torch.equal(out.reshape(-1).view(torch.int64 if elem == 8 else torch.int32),
                                  base_out.view(torch.int64 if elem == 8 else torch.int32))
                      and torch.equal(grad.reshape(n, -1).view(torch.int64 if elem == 8 else torch.int32),
                                      base_grad.view(torch.int64 if elem == 8 else torch.int32)))

    contenders = (("fused", lattice(1)), ("expanded", lattice(0)), ("auto", lattice(-1)), ("baseline", baseline),
                  ("expansion", expansion))
    names, took, ms = {}, {}, {c: [] for c, _ in contenders}
    for label, fn in contenders:
        for _ in range(3):
            fn()
        it.finish()
        torch.cuda.synchronize()
        names[label] = it.kernel_name()
        took[label] = it.last_lattice_path if label in ("fused", "expanded", "auto") else None
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
           "points": npts, "options": options, "reps": reps, "took": took, "kernels": names,
           "fused_bits_equal_baseline": bits_equal, "fused_setting_took": fused_path,
           "planned": interpn_amd.lattice_grad_plan(dtype, method, shape, lens)[0],
           "bytes_per_point_model": {"fused": (n + 1) * elem, "per_point_kernels": (2 * n + 1) * elem}}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "gpoints_per_s": round(npts / (med * 1e-3) / 1e9, 2)}
    row["fused"]["result_tb_per_s"] = round(npts * (n + 1) * elem / (row["fused"]["ms"] * 1e-3) / 1e12, 3)
    row["ratio_baseline_over_fused"] = round(row["baseline"]["ms"] / row["fused"]["ms"], 2)
    row["ratio_baseline_plus_expansion_over_fused"] = round((row["baseline"]["ms"] + row["expansion"]["ms"]) / row["fused"]["ms"], 2)
    row["ratio_expanded_over_fused"] = round(row["expanded"]["ms"] / row["fused"]["ms"], 2)
    # the automatic rule's obligation: never fused where fused is slower than the expanded path by more than both spreads
    row["fused_slower_than_expanded_beyond_spread"] = bool(
        row["fused"]["ms"] > row["expanded"]["ms"] + row["fused"]["iqr_ms"] + row["expanded"]["iqr_ms"])
    row["auto_rule_holds"] = not (took["auto"] == "fused" and took["fused"] == "fused" and row["fused_slower_than_expanded_beyond_spread"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lattice_grad_bench.json"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--only", default="", help="comma-separated workload names")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_lattice_grad.py measures on a GPU and found none")
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
        doc = {"tool": "tools/bench_lattice_grad.py", "device": torch.cuda.get_device_name(0),
               "method": "HIP events, 3 warm-up evaluations per contender, contenders alternated in one process on one handle "
                         "with rotating order, median and IQR; fused compared bit for bit with the baseline at the timed size",
               "baseline": "baseline (+ expansion, reported separately)", "rows": rows}
        with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
