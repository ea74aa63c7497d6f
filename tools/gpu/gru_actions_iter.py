"""Categorical GRU learners with 17 action ids (xp_gamma.py's shape: 5 agents x 16 channels, 24 inputs, hidden 64,
history_len 10, episodes of 200 slots): the GRU kernels' second action tile (csrc/gru_kernels.hip, AT = 2) against
the torch agent-stacked path -- what this shape ran while the kernels stopped at 16 actions -- in the same process,
alternating.

  python tools/gpu/gru_actions_iter.py --out profiles/gru_actions/bench.json --commit $(git rev-parse --short HEAD)

Per (algorithm, env count) two learners are built on envs of their own with the same seeds: one as a user gets it,
one with D2D_FUSED_POLICY=0 D2D_FUSED_UPDATE=0 set while its path switches are read (they are cached per learner).
Timed with device events, after a warm-up iteration of each, 5 repetitions, the two learners alternating: a training
rollout of one 200-slot episode per env, the forced log-prob pass of D2D-PPO's later epochs (the padded training
windows of every sample), one update epoch, and one whole iteration (rollout + 2 epochs, the evaluation stubbed).
Medians with min-max; `iteration_ok` says that the kernels' median iteration is not slower than the torch path's
median by more than the torch path's own min-max spread.  Env counts: 10 (the driver's num_episodes) and 256."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "d2d-ppo_amd")]

T_EP, HIDDEN, N_CHANNELS = 200, 64, 16
SHAPES = ((5, 10, 10), (5, 256, 10))                                      # (agents, envs, history_len)
TORCH_ENV = {"D2D_FUSED_POLICY": "0", "D2D_FUSED_UPDATE": "0"}


def make_env(n, E):
    """xp_gamma.py:33-54's env (its five devices; more agents repeat them)"""
    from envs.channel_selection_env import ChannelSelectionEnv
    return ChannelSelectionEnv(n_agents=n, n_channels=N_CHANNELS, deadlines=np.array([7] * n), period=np.array([7] * n),
                               lbdas=np.array([1 / 3.5] * n), episode_length=T_EP, traffic_model="aperiodic",
                               arrival_probs=np.array([1] * n), periodic_devices=np.array([k for k in range(n) if k % 5 in (2, 4)]),
                               offsets=np.resize(np.array([0, 2, 4, 0, 2]), n),
                               channel_switch=np.array([0.8] * (N_CHANNELS + 1)), verbose=False, n_envs=E,
                               device="cuda:0", seed=1)


def make_learner(algo, n, E, L, on_kernels):
    from algorithms.d2d_ppo import D2DPPO
    from algorithms.ippo import iPPO
    saved = {k: os.environ.get(k) for k in TORCH_ENV}
    if not on_kernels:
        os.environ.update(TORCH_ENV)
    try:
        torch.manual_seed(3)
        cls = iPPO if algo == "ippo" else D2DPPO
        lr = cls(make_env(n, E), hidden_size=HIDDEN, device="cuda", useRNN=True, history_len=L, early_stopping=False)
        assert lr.policy.A == N_CHANNELS + 1
        # the switches read the environment once per learner: read them now
        got = (lr._gru_ok(), lr._fused_update_ok(), lr._record_ok())
        assert got[:2] == (on_kernels, on_kernels), (algo, n, E, L, on_kernels, got)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    lr.test = lambda num_episodes: (0.5, 1.0, 0, 0.0)
    return lr


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], all=v)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def legs(algo, lr, E):
    """One repetition of one learner: ms of (rollout, forced pass, update epoch, iteration)"""
    roll = (lambda: lr._rollout(E, defer_values=True)) if algo == "ippo" else (lambda: lr._rollout(E))
    ms = {}
    ms["rollout"], ro = timed(roll)
    if algo == "d2d":
        if lr._fused_update_ok():
            ms["forced"], _ = timed(lambda: lr._logp_forced(ro))
        else:
            x, acts, _ = lr._update_inputs(ro)
            with torch.no_grad():
                ms["forced"], _ = timed(lambda: lr._evaluate(x, acts))
            del x, acts
    upd = lr._update_state(ro)
    ms["epoch"], _ = timed(lambda: lr._update_epoch(ro, upd))
    del ro, upd
    kw = dict(n_epoch=2, num_episodes=E, test_freq=10 ** 9)
    ms["iteration"], _ = timed(lambda: lr.train(1, **kw))
    return ms


def case(algo, n, E, L, reps):
    learners = {"hip": make_learner(algo, n, E, L, True), "torch": make_learner(algo, n, E, L, False)}
    for lr in learners.values():                                         # warm-up: every leg once
        legs(algo, lr, E)
    torch.cuda.synchronize()
    times = {}
    for _ in range(reps):
        for name, lr in learners.items():
            for leg, ms in legs(algo, lr, E).items():
                times.setdefault(f"{leg}_ms_{name}", []).append(ms)
    r = dict(algo=algo, n_agents=n, n_envs=E, history_len=L, hidden=HIDDEN, slots=T_EP,
             **{k: stats(v) for k, v in times.items()})
    hip, ref = r["iteration_ms_hip"], r["iteration_ms_torch"]
    r["iteration_speedup"] = ref["median"] / hip["median"]
    r["iteration_ok"] = hip["median"] <= ref["median"] + (ref["max"] - ref["min"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_actions", "bench.json"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--algos", default="ippo,d2d")
    ap.add_argument("--shapes", default=",".join("x".join(str(v) for v in s) for s in SHAPES),
                    help="agents x envs x history_len, comma-separated")
    a = ap.parse_args()
    res = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in a.shapes.split(","):
        n, E, L = (int(v) for v in shape.split("x"))
        for algo in a.algos.split(","):
            res.append(case(algo, n, E, L, a.reps))
            print(json.dumps({k: (round(v["median"], 2) if isinstance(v, dict) else v) for k, v in res[-1].items()}),
                  flush=True)
            torch.cuda.empty_cache()
            with open(a.out, "w") as fh:                                 # after every case: a long run keeps what it has
                json.dump(dict(commit=a.commit, device=torch.cuda.get_device_name(0), reps=a.reps,
                               note="ms, device events; hip = the GRU kernels with two action tiles, torch = D2D_FUSED_POLICY=0 "
                                    "D2D_FUSED_UPDATE=0 (the agent-stacked torch path); alternating in one process",
                               cases=res), fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
