"""bench.py --gpus N on one node without an external launcher.

The driver's scaling run is `bench.py --gpus N`; bench.py starts the N rank processes itself when no
WORLD_SIZE is set (bench.self_launch) before anything touches the GPU, and every rank reports the group it
joined: `n_gpus` (WORLD_SIZE), `ranks_seen` (an all-reduce of ones over the group) and `dist_backend`.  On a
one-GPU box two ranks cannot run RCCL against each other, so the GPU test uses the rehearsal switches
(D2D_BENCH_BACKEND=gloo, D2D_BENCH_SHARE_GPU=1: both ranks on cuda:0); the nccl branch is the default of the
same code.  The PPO leg's update runs the bucketed gradient all-reduce (algorithms/data_parallel.py, the
per-agent updates of ippo.py:418-426), so its "allreduce" phase must be present and non-zero."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

LAUNCH_VARS = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "GROUP_RANK", "MASTER_ADDR", "MASTER_PORT")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_VARS}
    env.update({"PYTHONUNBUFFERED": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    env.update(kw)
    return env


def test_bench_refuses_world_size_mismatch():
    """WORLD_SIZE from a launcher that disagrees with --gpus: exit 2 before any GPU call (runs on CPU)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-cpu-baseline"],
                       env=_env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "refusing" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(420)
def test_bench_self_launch_two_ranks(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--legs", "env,ppo", "--steps", "10",
           "--warmup", "3", "--envs", "8192", "--ppo-envs", "256", "--ppo-epochs", "2", "--env-mode", "record",
           "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=_env(D2D_BENCH_BACKEND="gloo", D2D_BENCH_SHARE_GPU="1", TMPDIR=str(tmp_path)),
                       capture_output=True, text=True, timeout=400, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert len(lines) == 1, r.stdout[-3000:]  # rank 0 alone prints the line
    res = json.loads(lines[0])
    ph = res["ppo"]["phase_ms_per_update"]
    print(json.dumps({"n_gpus": res["n_gpus"], "ranks_seen": res["ranks_seen"], "backend": res["dist_backend"],
                      "value": res["value"], "ppo_phase_ms": ph}))
    assert res["n_gpus"] == res["ranks_seen"] == 2
    assert res["dist_backend"] == "gloo"
    assert res["config"]["global_envs"] == 2 * 8192
    assert ph.get("allreduce", 0.0) > 0.0, ph
    assert res["value"] > 0 and res["ppo_updates_per_s"] > 0


def test_bench_legs_need_full():
    """--legs selects among the legs of a --full run: without --full it is an argument error, not ignored (CPU)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--legs", "ppo"], env=_env(),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--full" in r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run reports the headline alone (no leg, repeat or CPU baseline), times exactly --steps steps, and
    --dump-outputs writes float32 arrays that two runs with equal arguments reproduce bit for bit (3 + 7 slots
    cross the episode end at --episode-length 8, so the reset inside the loop is covered)."""
    import numpy as np
    dirs = [tmp_path / "a", tmp_path / "b"]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7",
                               "--warmup", "3", "--envs", "1024", "--episode-length", "8", "--dump-outputs", str(d)],
                              env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
             for d in dirs]
    outs = [p.communicate(timeout=280) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, f"rc {p.returncode}\n{so[-3000:]}\n{se[-3000:]}"
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, outs[0][0][-3000:]
    res = json.loads(lines[0])
    assert res["steps"] == 7 and res["warmup"] == 3 and res["full"] is False
    assert res["ms_per_step"] > 0 and res["value"] > 0 and res["higher_is_better"] is True
    assert abs(res["value"] - 1024 / (res["ms_per_step"] / 1e3)) <= 1e-6 * res["value"]
    extra = {"with_inloop_action_sampling", "fp32_obs", "rollout", "ppo", "train", "configs", "d2denv", "gru",
             "gru_c5", "cpu_baseline"}
    assert not extra & set(res), sorted(extra & set(res))
    a = {f: np.load(dirs[0] / f) for f in sorted(os.listdir(dirs[0]))}
    assert sorted(a) == ["obs.npy", "reward.npy"]
    assert a["obs.npy"].dtype == np.float32 and a["obs.npy"].shape == (1024, 64, 30)
    assert a["reward.npy"].dtype == np.float32 and a["reward.npy"].shape == (1024,)
    assert a["obs.npy"].any() and np.isfinite(a["obs.npy"]).all()
    for f, x in a.items():
        assert np.array_equal(x, np.load(dirs[1] / f)), f
