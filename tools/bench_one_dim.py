"""interpn::one_dim on the MI355X: every method x grid kind x {f64, f32} on the workloads of the issue that added it,
device-resident points, HIP events, warm-up, median of >= 20 launches, against a same-dtype torch device copy of the
same number of elements measured in the same process and alternated with the kernels (the floor).

  W1  1000 knots, 1e8 uniform points over the span +- 10 %      W2  10 knots, the same points
  W3  1e6 knots, 1e8 random points                               W4  1e6 knots, the same points sorted
  small: the per-call time at 1 and 100 points (device path, launch + finish)

    python tools/bench_one_dim.py [--reps 20] [--npts 100000000] [--json profiles/one_dim_bench.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METHODS = ("Linear1D", "LinearHoldLast1D", "Left1D", "Right1D", "Nearest1D")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--npts", type=int, default=100_000_000)
    ap.add_argument("--workloads", default="W1,W2,W3,W4,small")
    ap.add_argument("--json", default="")
    a = ap.parse_args()

    import torch

    from interpn_amd import Interpolator

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)

    def time_ms(fn, reps):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return ts

    results = []
    wl = a.workloads.split(",")
    for dtype in (np.float64, np.float32):
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        for name, nk, sort in (("W1", 1000, False), ("W2", 10, False), ("W3", 1_000_000, False), ("W4", 1_000_000, True)):
            if name not in wl:
                continue
            lo, hi = -1.0, 1.0
            span = hi - lo
            x = torch.rand(a.npts, dtype=tdt, device=dev) * (1.2 * span) + (lo - 0.1 * span)
            if sort:
                x = torch.sort(x).values
            out = torch.empty_like(x)
            dst = torch.empty_like(x)
            vals = rng.normal(size=nk).astype(dtype)
            grid = np.linspace(lo, hi, nk).astype(dtype)
            for kind in ("regular", "rectilinear"):
                for method in METHODS:
                    if kind == "regular":
                        it = Interpolator.grid1d_regular(method, dtype(lo), dtype(span / (nk - 1)), vals, device=0, dtype=dtype)
                    else:
                        it = Interpolator.grid1d_rectilinear(method, grid, vals, device=0, dtype=dtype)
                    ptrs, optr = [x.data_ptr()], out.data_ptr()
                    stream = torch.cuda.current_stream(dev).cuda_stream

                    def kern():
                        it.eval_device_ptrs(ptrs, optr, a.npts, stream)

                    # alternate: copy, kernel, copy, kernel ... (same process, same clocks); then the median of
                    # all `reps` launches of each
                    kms, cms = [], []
                    for _ in range(2):
                        cms += time_ms(lambda: dst.copy_(x), (a.reps + 1) // 2)
                        kms += time_ms(kern, (a.reps + 1) // 2)
                    it.finish()
                    k, c = float(np.median(kms)), float(np.median(cms))
                    row = dict(workload=name, knots=nk, sorted=sort, kind=kind, method=method,
                               dtype=np.dtype(dtype).name, npts=a.npts, ms=round(k, 4), copy_ms=round(c, 4),
                               gpts_per_s=round(a.npts / k / 1e6, 2), ratio_to_copy=round(k / c, 3),
                               kernel=it.kernel_name())
                    print(json.dumps(row), flush=True)
                    results.append(row)
                    it.close()
            del x, out, dst
            torch.cuda.empty_cache()
        if "small" in wl:
            for kind in ("regular", "rectilinear"):
                for method in METHODS:
                    vals = rng.normal(size=1000).astype(dtype)
                    grid = np.linspace(-1.0, 1.0, 1000).astype(dtype)
                    it = (Interpolator.grid1d_regular(method, dtype(-1.0), dtype(2.0 / 999), vals, device=0, dtype=dtype)
                          if kind == "regular" else Interpolator.grid1d_rectilinear(method, grid, vals, device=0, dtype=dtype))
                    for m in (1, 100):
                        xs = torch.rand(m, dtype=tdt, device=dev) * 2.2 - 1.1
                        o = torch.empty_like(xs)

                        def call():
                            it.eval_tensors([xs], o)
                            it.finish()

                        ms = float(np.median(time_ms(call, max(a.reps, 50))))
                        row = dict(workload="small", knots=1000, kind=kind, method=method, dtype=np.dtype(dtype).name,
                                   npts=m, us_per_call=round(ms * 1e3, 2))
                        print(json.dumps(row), flush=True)
                        results.append(row)
                    it.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
