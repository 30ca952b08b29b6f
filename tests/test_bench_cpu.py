"""bench.py on CPU: the N > 1 control flow (gloo process group, barriers, max over ranks, the
padded flat gather, one JSON line from rank 0) with the --dry-run-cpu stand-in env, and the
CPU-baseline leg (oracle with auto-reset, Philox actions) on a short sample."""
import json
import os
import subprocess
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_bench_two_rank_dry_run_cpu():
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29651", os.path.join(REPO, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--preroll", "2", "--envs-per-gpu", "5",
           "--dry-run-cpu", "--full", "--legs", "HopperPyBulletEnv-v0:3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["config"]["global_envs"] == 10
    assert d["scaling"] == "weak" and "dry_run" in d and d["allgather_step_bytes"] == 10 * (28 + 2) * 4
    assert d["hopper_f32"]["global_envs"] == 6


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """Without --full: one timed window, no legs and no CPU baseline whatever --legs says; the
    headline keys stay; --dump-outputs writes the env's output buffers as float32 .npy."""
    import numpy as np
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--preroll", "2", "--envs-per-gpu", "5", "--dry-run-cpu", "--legs", "HopperPyBulletEnv-v0:3",
           "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["timed_windows"] == 1 and len(d["window_ms_per_step"]) == 1
    assert d["ms_per_step"] > 0 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert "hopper_f32" not in d and "cpu_baseline" not in d and "allgather_step_ms" not in d
    obs = np.load(tmp_path / "out" / "obs.npy")
    assert obs.shape == (5, 28) and obs.dtype == np.float32
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["done.npy", "obs.npy", "reward.npy"]


def test_cpu_baseline_leg_with_autoreset():
    sys.path.insert(0, REPO)
    import bench
    d = bench.cpu_baseline(seconds=1.0)
    assert d["value"] > 0 and d["kind"] == "port" and d["cores"] >= 1
    assert "auto-reset" in d["sample"]
