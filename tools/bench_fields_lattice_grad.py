#!/usr/bin/env python3
"""Field-set gradients on a lattice: the fused kernel against the per-field path and against what a user did before — K
`Interpolator.eval_lattice_grad_tensors` calls, plus the `torch.stack` / `permute(...).contiguous()` that produce `(*m, K)`
and `(*m, K, N)` for channel-last results — in one process.

    python tools/bench_fields_lattice_grad.py --out profiles/fields_lattice_grad_bench.json [--reps 21] [--only NAME,NAME]

Method (that of tools/bench_fields_lattice.py): device-resident coordinate vectors, HIP events around
one evaluation, 3 warm-up evaluations per contender, then `--reps` rounds that ALTERNATE the contenders, their order
rotating from round to round, so that clock and cache state drift, and whatever ran just before, hit all of them alike.
Median and inter-quartile range per contender, in ms.  Every contender's values and Jacobian are compared bit for bit with
the fused kernel's at the timed size.

Contenders
  fused      option lattice = 1: one k_lattice_axes + one k_lattice_fields_grad_rows for all K fields
  auto       option lattice = -1: what the set picks by itself
  per_field  option lattice = 0 on the set: K expanded lattice-gradient evaluations through the K handles (+ two
             k_join_fields launches per slice, fields-last)
  baseline   what the parent offers: K Interpolator.eval_lattice_grad_tensors calls on K single handles in automatic mode; for
             fields-last results also torch.stack(values, dim=-1) and torch.stack(grads).permute(.., 0, 1).contiguous(), all
             inside the timed region
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, method, kind, grid shape, dtype, K, lattice lengths, field_axis, axis_lds_kb (None: the default budget; set on EVERY contender)
WORKLOADS = [
    ("lin3-64to256-f64-K3-last", "linear", "regular", [64] * 3, np.float64, 3, [256] * 3, -1, None),
    ("lin3-64to256-f64-K3-first", "linear", "regular", [64] * 3, np.float64, 3, [256] * 3, 0, None),
    ("lin3-64to256-f64-K3-last-rect", "linear", "rectilinear", [64] * 3, np.float64, 3, [256] * 3, -1, None),
    ("cub3-64to160-f64-K3-last", "cubic", "regular", [64] * 3, np.float64, 3, [160] * 3, -1, None),
    ("lin3-64to256-f32-K4-last", "linear", "regular", [64] * 3, np.float32, 4, [256] * 3, -1, None),
    ("cub2-540x960-to-1080p-f32-K3-last", "cubic", "regular", [540, 960], np.float32, 3, [1080, 1920], -1, 60),
    # G < K forced by the budget: 10 KiB hold the three lines of one field of 64 f64 columns per wave (1536 bytes), not of two
    ("cub3-64to160-f64-K3-first-G1", "cubic", "regular", [64] * 3, np.float64, 3, [160] * 3, 0, 10),
    ("lin3-64to256-f32-K8-last", "linear", "regular", [64] * 3, np.float32, 8, [256] * 3, -1, None),
    # the knob: 60 KiB hold the lines of all three fields (6144 bytes per wave) and a [64] x 13 tile (6656): G = K = 3
    ("lin3-64to256-f64-K3-last-kb60", "linear", "regular", [64] * 3, np.float64, 3, [256] * 3, -1, 60),
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
    jac = torch.empty([k, n] + lens if field_axis == 0 else lens + [k, n], dtype=tdt, device="cuda:0")
    parts = [torch.empty(lens, dtype=tdt, device="cuda:0") for _ in range(k)]
    gparts = [torch.empty([n] + lens, dtype=tdt, device="cuda:0") for _ in range(k)]
    keep = {}

    def lattice(opt):
        def f():
            fs.set_option("lattice", opt)
            fs.eval_lattice_grad_tensors(ax_t, out, jac, field_axis=field_axis)
        return f

    def baseline():
        if field_axis == 0:
            for f, it in enumerate(singles):
                it.eval_lattice_grad_tensors(ax_t, out[f], jac[f])
        else:
            for f, it in enumerate(singles):
                it.eval_lattice_grad_tensors(ax_t, parts[f], gparts[f])
            keep["out"] = torch.stack(parts, dim=-1)
            keep["jac"] = torch.stack(gparts).permute(*range(2, n + 2), 0, 1).contiguous()

    contenders = (("fused", lattice(1)), ("auto", lattice(-1)), ("per_field", lattice(0)), ("baseline", baseline))
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
            results[label] = (keep["out"].clone(), keep["jac"].clone()) if field_axis else (out.clone(), jac.clone())
        else:
            names[label], took[label], groups[label] = fs.kernel_name(), fs.last_lattice_path, fs.get_option("last_lattice_group")
            results[label] = (out.clone(), jac.clone())
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
               for c in ("auto", "per_field", "baseline") for a, b in zip(results["fused"], results[c]))
    results.clear()
    keep.clear()
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
    row["fused"]["result_tb_per_s"] = round(npts * k * (n + 1) * elem / (row["fused"]["ms"] * 1e-3) / 1e12, 3)
    row["ratio_baseline_over_fused"] = round(row["baseline"]["ms"] / row["fused"]["ms"], 2)
    row["ratio_per_field_over_fused"] = round(row["per_field"]["ms"] / row["fused"]["ms"], 2)
    # the automatic rule stands where fused is not slower than the baseline by more than the two contenders' combined IQR
    row["fused_not_slower_than_baseline"] = bool(row["fused"]["ms"] <= row["baseline"]["ms"] + row["fused"]["iqr_ms"] + row["baseline"]["iqr_ms"])
    faster = min(row["fused"]["ms"], row["per_field"]["ms"])
    spread = max(row["fused"]["iqr_ms"], row["per_field"]["iqr_ms"], row["auto"]["iqr_ms"])
    row["auto_within_spread_of_faster"] = bool(row["auto"]["ms"] <= faster + spread)
    # ... and the choice itself, judged by the chosen path's own timing: `auto` and the contender it picks are the same
    # launches, so a difference between those two timings is what the order of the rotation does, not what the rule does
    chosen = "fused" if took["auto"] == "fused" else "per_field"
    row["auto_chose"] = chosen
    row["auto_choice_within_spread_of_faster"] = bool(row[chosen]["ms"] <= faster + spread)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_lattice_grad_bench.json"))
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
        doc = {"tool": "tools/bench_fields_lattice_grad.py", "device": torch.cuda.get_device_name(0),
               "method": "HIP events, 3 warm-up evaluations per contender, contenders alternated in one process with rotating "
                         "order, median and IQR; every contender's values and Jacobian compared bit for bit at the timed size",
               "baseline": "K Interpolator.eval_lattice_grad_tensors calls (+ torch.stack(dim=-1) of the values and "
                           "torch.stack(grads).permute(.., 0, 1).contiguous() for fields-last results)", "rows": rows}
        with open(a.out, "w") as f:  # after every row: a run cut short keeps what it measured
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
