#!/usr/bin/env python3
"""Host cost of small device-tensor calls (profiles/step_commands.md, "Small calls"): a 1e3-point 2-D multilinear call +
finish on a 4 x 4 grid (cfg1's `resident_handle_device_tensors_incl_status` loop) and a 20 000-point launch of the sweep
kernel + finish through a scratch block (3-D, 9 x 8 x 7, the shape of tests/test_step_commands_gpu.py).  Each call is
timed on its own: median and best of 3 000, one JSON line.  `INTERPN_AMD_LIB=<path>` loads another build of the library;
run the builds in alternating child processes."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import interpn_amd  # noqa: E402

CALLS = 3000
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)


def timed(it, obs, out):
    for _ in range(200):
        it.eval_tensors(obs, out)
        it.finish()
    torch.cuda.synchronize()
    us = np.empty(CALLS)
    for k in range(CALLS):
        t0 = time.perf_counter()
        it.eval_tensors(obs, out)
        it.finish()
        us[k] = (time.perf_counter() - t0) * 1e6
    return [round(float(np.median(us)), 2), round(float(us.min()), 2)]


res = {"lib": os.environ.get("INTERPN_AMD_LIB", "")}
it = interpn_amd.Interpolator.regular("linear", [4, 4], np.full(2, -1.0), np.full(2, 2.0 / 3), rng.uniform(-1, 1, 16))
obs = [torch.rand(1000, dtype=torch.float64, device=dev) * 2 - 1 for _ in range(2)]
res["call_1e3_us"] = timed(it, obs, torch.empty(1000, dtype=torch.float64, device=dev))
it.close()

os.environ["INTERPN_HIP_BRICKS"] = "11"  # (a grid this small keeps no sweep table by itself)
dims = [9, 8, 7]
it = interpn_amd.Interpolator.regular("linear", dims, np.full(3, -1.0), np.array([2.0 / (n - 1) for n in dims]),
                                      rng.uniform(-1, 1, int(np.prod(dims))))
del os.environ["INTERPN_HIP_BRICKS"]
it.set_option("sweep", 1)
obs = [torch.rand(20_000, dtype=torch.float64, device=dev) * 2 - 1 for _ in range(3)]
res["sweep_2e4_us"] = timed(it, obs, torch.empty(20_000, dtype=torch.float64, device=dev))
assert it.last_path == "sweep", (it.last_path, it.last_path_reason)
it.close()
print(json.dumps(res))
