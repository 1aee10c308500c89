"""The RCCL branch of the multi-GPU path, executed on the GPU box (round-2 verdict: it had never
run anywhere).  One rank is all a 1-GPU box offers, but the calls are the ones an 8-GPU node makes:
`init_process_group("nccl", device_id=...)`, RCCL broadcasts of `vals` and of the rectilinear axes
as CUDA tensors, an interpolator built on the broadcast buffer, `eval_shard`, the CUDA-tensor MIN
all-reduce in `finish()` (clean and with an injected NaN), `concat_on_host`, `destroy_process_group`
— and `bench.py --force-dist --backend nccl`, whose record must say what really happened.

Each case runs in a FRESH child process started by the test (a child, never an exec of this
process): a launcher's ranks are fresh processes too."""

import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update({"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": str(_free_port()), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    return env


def _last_json(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert lines, stdout[-2000:]
    return json.loads(lines[-1])


def _visible_gpus():
    """GPUs of the box (counting them does not initialise HIP in this process)."""
    import torch

    return max(1, torch.cuda.device_count())


def rccl_world_size(ngpus: int) -> int:
    """Ranks the RCCL tests spawn on a box with `ngpus` GPUs: one per GPU, at most 8 (1 on the
    pool's single-GPU boxes; the process guard of the GPU boxes allows 6 processes on ONE card, a
    rank per card is a different matter)."""
    return max(1, min(int(ngpus), 8))


@pytest.mark.gpu
def test_sharded_path_over_rccl_one_rank_per_gpu():
    """`min(device_count, 8)` fresh ranks, rank r on GPU r, over the nccl (= RCCL) backend: world size 1
    on a single-GPU box (the same calls), a real xGMI broadcast + MIN all-reduce on a multi-GPU node."""
    world = rccl_world_size(_visible_gpus())
    port = _free_port()
    procs = []
    for r in range(world):
        env = _env()
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(world), "MASTER_PORT": str(port)})
        procs.append(subprocess.Popen([sys.executable, "-m", "tests.rccl_child"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = _drain_together(procs, 600)
    assert all(p.returncode == 0 for p in procs), [(o[0][-1000:], o[1][-3000:]) for o in outs]
    rec = _last_json(outs[0][0])
    assert rec["backend"] == "nccl" and rec["world"] == world
    assert rec["broadcast"] == {"vals": 24**3, "axes": [24, 24, 24]}
    kinds = {c["kind"]: c for c in rec["cases"]}
    assert set(kinds) == {"regular", "rectilinear"}
    assert all(c["bitwise_equal"] and c["kernel"] for c in kinds.values())
    assert kinds["regular"]["first_bad_index"] == 200_003 - 1234


def _drain_together(procs, timeout):
    """communicate() with every child at once: rank 0 waits for rank 1 inside collectives, so
    reading rank 1's pipes only after rank 0 has exited would block both once rank 1 has written
    more than a pipe holds (RCCL / gloo warnings); the children are killed on timeout."""
    import threading

    outs = [None] * len(procs)

    def drain(i):
        try:
            outs[i] = procs[i].communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            procs[i].kill()
            outs[i] = procs[i].communicate()

    threads = [threading.Thread(target=drain, args=(i,)) for i in range(len(procs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    return outs


@pytest.mark.gpu
def test_sharded_path_two_ranks_on_one_gpu_over_gloo():
    """Two real ranks (two processes, two HIP contexts, real interpolator handles) sharing the test
    box's one GPU over gloo: contiguous shards, the first-bad index found in the LAST rank's shard
    and reported by every rank, results assembled on rank 0 and bit-identical to the oracle."""
    port = _free_port()
    procs = []
    for r in range(2):
        env = _env()
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": "2", "MASTER_PORT": str(port),
                    "INTERPN_TEST_BACKEND": "gloo", "INTERPN_TEST_SAME_DEVICE": "1"})
        procs.append(subprocess.Popen([sys.executable, "-m", "tests.rccl_child"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = _drain_together(procs, 600)
    assert all(p.returncode == 0 for p in procs), [(o[0][-1000:], o[1][-3000:]) for o in outs]
    rec = _last_json(outs[0][0])
    assert rec["backend"] == "gloo" and rec["world"] == 2
    kinds = {c["kind"]: c for c in rec["cases"]}
    assert all(c["bitwise_equal"] for c in kinds.values()) and kinds["regular"]["first_bad_index"] == 200_003 - 1234


@pytest.mark.gpu
def test_bench_force_dist_over_rccl_records_what_happened():
    env = _env()
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):  # bench.py is started plainly, as the driver does at N = 1
        env.pop(k)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--force-dist", "--backend", "nccl",
                        "--steps", "5", "--warmup", "2", "--points", "4000000", "--no-cpu-baseline", "--no-configs",
                        "--no-ablate", "--sustain-seconds", "0.05"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rec = _last_json(p.stdout)
    cfg = rec["config"]
    assert rec["n_gpus"] == 1 and cfg["backend"] == "nccl"
    assert cfg["process_group"] == {"initialised": True, "backend": "nccl", "world_size": 1}
    assert cfg["grid_broadcast"]["collective"] == "broadcast" and cfg["grid_broadcast"]["on"] == "device"
    assert cfg["grid_broadcast"]["bytes"] == 64**3 * 8
    assert "RCCL" in cfg["sharding"]
    assert rec["value"] > 0 and rec["roofline"]["frac"] > 0


@pytest.mark.gpu
def test_bench_single_process_claims_no_broadcast():
    env = _env()
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--points",
                        "4000000", "--no-cpu-baseline", "--no-configs", "--no-ablate", "--sustain-seconds", "0.05"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    cfg = _last_json(p.stdout)["config"]
    assert cfg["backend"] is None and cfg["process_group"]["initialised"] is False
    assert cfg["grid_broadcast"] is None
    assert "broadcast" not in cfg["sharding"]


@pytest.mark.gpu
def test_bench_one_rank_per_gpu_smoke():
    """`bench.py --gpus N --steps 2 --full` with N = min(device_count, 8) > 1: the driver's multi-GPU command in
    its spawned form (N fresh ranks over RCCL, grid broadcast, with --full the cfg5 block).  Skipped on a single-GPU box,
    where `test_bench_force_dist_over_rccl_records_what_happened` runs the same calls with one rank."""
    n = rccl_world_size(_visible_gpus())
    if n < 2:
        pytest.skip("one GPU visible: the one-rank form of this test runs instead")
    env = _env()
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1", "--full",
                        "--no-cpu-baseline", "--no-configs", "--no-ablate", "--sustain-seconds", "0.05"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    rec = _last_json(p.stdout)
    assert rec["n_gpus"] == n and rec["config"]["process_group"]["world_size"] == n
    assert rec["config"]["grid_broadcast"]["collective"] == "broadcast" and rec["scaling"] == "weak"
    assert rec["value"] > 0
