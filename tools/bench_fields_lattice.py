#!/usr/bin/env python3
"""Field sets on a lattice: the fused kernel against the per-field path and against what a user did before — K
`Interpolator.eval_lattice_tensors` calls, plus `torch.stack(..., dim=-1)` for channel-last results — in one process.

    python tools/bench_fields_lattice.py --out profiles/fields_lattice_bench.json [--reps 21] [--only lin3-64to256-f64-K3-last]

Method: device-resident coordinate vectors, HIP events around one evaluation, 3 warm-up evaluations
per contender, then `--reps` rounds that ALTERNATE the contenders, their order rotating from round to round, so that clock
and cache state drift, and whatever ran just before, hit all of them alike.  Median and inter-quartile range per contender,
in ms.

Contenders
  fused      option lattice = 1: one k_lattice_axes + one k_lattice_fields_rows for all K fields
  per_field  option lattice = 0 on the set: K expanded lattice evaluations through the K handles (+ k_join_fields, fields-last)
  auto       option lattice = -1: what the set picks by itself
  baseline   what the parent offers: K Interpolator.eval_lattice_tensors calls on K single handles in automatic mode, and for
             fields-last results torch.stack(..., dim=-1) of the K results, all inside the timed region
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, method, kind, grid shape, dtype, K, lattice lengths, field_axis, axis_lds_kb (None: the default budget)
WORKLOADS = [
    ("cub2-1080p-to-2160p-f32-K3-last", "cubic", "regular", [1080, 1920], np.float32, 3, [2160, 3840], -1, 60),
    ("cub2-1080p-to-2160p-f32-K4-last", "cubic", "regular", [1080, 1920], np.float32, 4, [2160, 3840], -1, 60),
    ("lin2-512to4096-f64-K4-last", "linear", "regular", [512, 512], np.float64, 4, [4096, 4096], -1, None),
    ("lin2-512to4096-f64-K4-first", "linear", "regular", [512, 512], np.float64, 4, [4096, 4096], 0, None),
    ("lin3-64to256-f64-K3-last", "linear", "regular", [64] * 3, np.float64, 3, [256] * 3, -1, None),
    ("lin3-64to256-f64-K3-first", "linear", "regular", [64] * 3, np.float64, 3, [256] * 3, 0, None),
    ("cub3-64to160-f64-K2-last", "cubic", "regular", [64] * 3, np.float64, 2, [160] * 3, -1, None),
    ("lin3-64to256-f64-K3-last-rect", "linear", "rectilinear", [64] * 3, np.float64, 3, [256] * 3, -1, None),
    # G < K: 10 KiB hold two lines of 64 f64 and a [64][3] tile per wave (2560 bytes), not three lines
    ("lin3-64to256-f64-K4-last-G2", "linear", "regular", [64] * 3, np.float64, 4, [256] * 3, -1, 10),
]


def quartiles(ms):
    q1, med, q3 = np.percentile(np.asarray(ms), [25, 50, 75])
    return float(med), float(q3 - q1)


def run(name, method, kind, shape, dtype, k, lens, field_axis, kb, reps):
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
    fields = rng.uniform(-1.0, 1.0, (k, int(np.prod(shape)))).astype(dtype)
    if kind == "regular":
        starts = np.array([g[0] for g in grids], dtype=dtype)
        steps = np.array([g[1] - g[0] for g in grids], dtype=dtype)
        fs = interpn_amd.Fields.regular(method, shape, starts, steps, fields, dtype=dtype)
        singles = [interpn_amd.Interpolator.regular(method, shape, starts, steps, fields[f], dtype=dtype) for f in range(k)]
    else:
        fs = interpn_amd.Fields.rectilinear(method, grids, fields, dtype=dtype)
        singles = [interpn_amd.Interpolator.rectilinear(method, grids, fields[f], dtype=dtype) for f in range(k)]
    if kb is not None:
        fs.set_option("axis_lds_kb", kb)
        for it in singles:
            it.set_option("axis_lds_kb", kb)
    axes = [np.linspace(-1.02, 1.02, m).astype(dtype) for m in lens]
    ax_t = [torch.from_numpy(a).to("cuda:0") for a in axes]
    npts = int(np.prod(lens))
    out = torch.empty([k] + lens if field_axis == 0 else lens + [k], dtype=tdt, device="cuda:0")
    parts = [torch.empty(lens, dtype=tdt, device="cuda:0") for _ in range(k)]
    keep = {}

    def lattice(opt):
        def f():
            fs.set_option("lattice", opt)
            fs.eval_lattice_tensors(ax_t, out, field_axis=field_axis)
        return f

    def baseline():
        if field_axis == 0:
            for f, it in enumerate(singles):
                it.eval_lattice_tensors(ax_t, out[f])
        else:
            for f, it in enumerate(singles):
                it.eval_lattice_tensors(ax_t, parts[f])
            keep["stacked"] = torch.stack(parts, dim=-1)

    contenders = (("fused", lattice(1)), ("per_field", lattice(0)), ("auto", lattice(-1)), ("baseline", baseline))
    names, took, groups, results = {}, {}, {}, {}
    ms = {c: [] for c, _ in contenders}
    for label, fn in contenders:
        for _ in range(3):
            fn()
        fs.finish()
        for it in singles:
            it.finish()
        if label == "baseline":
            names[label], took[label] = singles[0].kernel_name(), singles[0].last_lattice_path
            results[label] = keep["stacked"].clone() if field_axis else out.clone()
        else:
            names[label], took[label], groups[label] = fs.kernel_name(), fs.last_lattice_path, fs.get_option("last_lattice_group")
            results[label] = out.clone()
    same = all(torch.equal(results["fused"].view(torch.uint8), results[c].view(torch.uint8)) for c in ("per_field", "auto", "baseline"))
    results.clear()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nc = len(contenders)
    for rep in range(reps):
        for label, fn in contenders[rep % nc:] + contenders[:rep % nc]:  # rotate the order
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ms[label].append(start.elapsed_time(stop))
    fs.finish()
    fs.close()
    for it in singles:
        it.finish()
        it.close()
    row = {"workload": name, "method": method, "kind": kind, "shape": shape, "dtype": np.dtype(dtype).name, "nfields": k,
           "lattice": lens, "layout": "field_major" if field_axis == 0 else "fields_last", "axis_lds_kb": kb, "points": npts,
           "reps": reps, "took": took, "kernels": names, "group": groups.get("fused"), "bit_identical": bool(same)}
    for label, _ in contenders:
        med, iqr = quartiles(ms[label])
        row[label] = {"ms": round(med, 4), "iqr_ms": round(iqr, 4), "gpoints_per_s": round(npts / (med * 1e-3) / 1e9, 2)}
    row["fused"]["result_tb_per_s"] = round(npts * k * elem / (row["fused"]["ms"] * 1e-3) / 1e12, 3)
    row["ratio_baseline_over_fused"] = round(row["baseline"]["ms"] / row["fused"]["ms"], 2)
    row["ratio_per_field_over_fused"] = round(row["per_field"]["ms"] / row["fused"]["ms"], 2)
    faster = min(row["fused"]["ms"], row["per_field"]["ms"])
    spread = max(row["fused"]["iqr_ms"], row["per_field"]["iqr_ms"], row["auto"]["iqr_ms"])
    row["auto_within_spread_of_faster"] = bool(row["auto"]["ms"] <= faster + spread)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_lattice_bench.json"))
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
        doc = {"tool": "tools/bench_fields_lattice.py", "device": torch.cuda.get_device_name(0),
               "method": "HIP events, 3 warm-up evaluations per contender, contenders alternated in one process with rotating "
                         "order, median and IQR",
               "baseline": "K Interpolator.eval_lattice_tensors calls (+ torch.stack(dim=-1) for fields-last results)", "rows": rows}
        with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
