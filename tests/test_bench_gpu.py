"""bench.py on the GPU: a plain run measures the headline only and `--dump-outputs` writes what its last timed step
computed (checked bit for bit against the oracle on the same inputs); `--full` still adds the measurements beside
the headline.  bench.py runs in a fresh child process, as the driver starts it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _run(*argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path, oracle):
    import torch

    P = 5_000_000  # more than bench.DUMP_POINTS: the seeded sample is what gets written
    rec = _run("--steps", "3", "--warmup", "1", "--points", str(P), "--dump-outputs", str(tmp_path))
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "Mpoints/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    # nothing beside the headline in a plain run
    assert "cpu_baseline" not in rec and "configs" not in rec and "host_path" not in rec
    assert "sustained" not in rec["roofline"] and "measured_copy_GBps" not in rec["roofline"]
    assert sorted(os.listdir(tmp_path)) == ["out.npy"]
    got = np.load(tmp_path / "out.npy")
    idx = bench.dump_index(P, 0, 1)
    assert got.dtype == np.float64 and got.shape == idx.shape and idx.size < P

    obs, _ = bench.make_obs(torch, torch.device("cuda", 0), P, 0)
    sub = [o.cpu().numpy()[idx] for o in obs]
    spec = bench.build_spec("linear", "regular", 64, 3, False, seed=1)
    want = np.zeros(idx.size)
    oracle.linear_regular(spec["dims"], spec["starts"], spec["steps"], spec["vals"], sub, want)
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_full_run_keeps_the_side_measurements():
    rec = _run("--steps", "3", "--warmup", "1", "--points", "4000000", "--full", "--no-configs", "--no-ablate",
               "--sustain-seconds", "0.05", "--cpu-sample", "200000")
    assert rec["steps"] == 3 and rec["value"] > 0
    assert rec["roofline"]["sustained"]["launches"] >= 8 and rec["roofline"]["measured_copy_GBps"] > 0
    assert rec["cpu_baseline"]["gpu_matches_bitwise"] is True
