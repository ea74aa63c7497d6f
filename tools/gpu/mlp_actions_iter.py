"""MLP learners with 17 action ids (xp_gamma.py's shape: 5 agents x 16 channels, 24 inputs, episodes of 200 slots) at
hidden 64 and the default 128: the two-tile MLP kernels (csrc/mlp_actions_kernels.hip) against the torch agent-stacked
path -- what this shape ran while the MLP kernels stopped at 16 actions -- in the same process, alternating.

  python tools/gpu/mlp_actions_iter.py --out profiles/mlp_actions/bench.json --commit $(git rev-parse --short HEAD)

A run can be split by shape: `--shapes 5x10x64`, then `--shapes 5x256x64 --append`, ... -- with --append the cases
already in --out are kept (it refuses a file of another commit, device or repetition count).

Per (algorithm, shape) two learners are built on envs of their own with the same seeds: one as a user gets it, one
with D2D_FUSED_POLICY=0 D2D_FUSED_UPDATE=0 set while its path switches are read (they are cached per learner).  The
second is the yardstick: what this shape ran before.  Timed with device events, after a warm-up of every leg of each,
5 repetitions, the two learners alternating: a training rollout of one 200-slot episode per env, the forced log-prob
pass of D2D-PPO's later epochs, one update epoch, and one whole iteration (rollout + 2 epochs, the evaluation
stubbed).  Medians with min-max; `iteration_ok` is the condition for keeping a size on the kernels: EVERY iteration on
the kernels is faster than the torch path's fastest.  Every timed step runs under a watchdog (--limit seconds): a step
that passes it ends the process with a traceback, and the file keeps the cases finished before.

Env counts: 10 (the driver's num_episodes) and 256."""
import argparse
import faulthandler
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "d2d-ppo_amd")]

T_EP, N_CHANNELS = 200, 16
SHAPES = ((5, 10, 64), (5, 10, 128), (5, 256, 64), (5, 256, 128))          # (agents, envs, hidden)
TORCH_ENV = {"D2D_FUSED_POLICY": "0", "D2D_FUSED_UPDATE": "0"}
LIMIT = [120]


def make_env(n, E):
    """xp_gamma.py:33-54's env (its five devices; more agents repeat them)"""
    from envs.channel_selection_env import ChannelSelectionEnv
    return ChannelSelectionEnv(n_agents=n, n_channels=N_CHANNELS, deadlines=np.array([7] * n), period=np.array([7] * n),
                               lbdas=np.array([1 / 3.5] * n), episode_length=T_EP, traffic_model="aperiodic",
                               arrival_probs=np.array([1] * n), periodic_devices=np.array([k for k in range(n) if k % 5 in (2, 4)]),
                               offsets=np.resize(np.array([0, 2, 4, 0, 2]), n),
                               channel_switch=np.array([0.8] * (N_CHANNELS + 1)), verbose=False, n_envs=E,
                               device="cuda:0", seed=1)


def make_learner(algo, n, E, H, on_kernels):
    from algorithms.d2d_ppo import D2DPPO
    from algorithms.ippo import iPPO
    from d2dhip import _lib
    saved = {k: os.environ.get(k) for k in TORCH_ENV}
    if not on_kernels:
        os.environ.update(TORCH_ENV)
    try:
        torch.manual_seed(3)
        cls = iPPO if algo == "ippo" else D2DPPO
        lr = cls(make_env(n, E), hidden_size=H, device="cuda", early_stopping=False)          # useRNN=False
        p = lr.policy
        assert p.A == N_CHANNELS + 1 and _lib.mlp_actions(p.F, p.H, p.A, 1), (p.F, p.H, p.A)
        # the switches read the environment once per learner: read them now
        got = (lr._fused_ok(), lr._fused_update_ok(), lr._record_ok())
        assert got == (on_kernels, on_kernels, False), (algo, n, E, H, on_kernels, got)
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
    """ms of fn by device events, under the watchdog"""
    faulthandler.dump_traceback_later(LIMIT[0], exit=True)
    try:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out
    finally:
        faulthandler.cancel_dump_traceback_later()


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


def case(algo, n, E, H, reps):
    learners = {"hip": make_learner(algo, n, E, H, True), "torch": make_learner(algo, n, E, H, False)}
    for lr in learners.values():                                         # warm-up: every leg once
        legs(algo, lr, E)
    torch.cuda.synchronize()
    times = {}
    for _ in range(reps):
        for name, lr in learners.items():
            for leg, ms in legs(algo, lr, E).items():
                times.setdefault(f"{leg}_ms_{name}", []).append(ms)
    r = dict(algo=algo, n_agents=n, n_envs=E, hidden=H, obs_dim=learners["hip"].policy.F, n_out=N_CHANNELS + 1,
             slots=T_EP, **{k: stats(v) for k, v in times.items()})
    hip, ref = r["iteration_ms_hip"], r["iteration_ms_torch"]
    r["iteration_speedup"] = ref["median"] / hip["median"]
    r["iteration_ok"] = hip["max"] < ref["min"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_actions", "bench.json"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--algos", default="ippo,d2d")
    ap.add_argument("--limit", type=int, default=LIMIT[0], help="seconds a timed step may take")
    ap.add_argument("--append", action="store_true", help="keep the cases --out already holds and add to them")
    ap.add_argument("--shapes", default=",".join("x".join(str(v) for v in s) for s in SHAPES),
                    help="agents x envs x hidden, comma-separated")
    a = ap.parse_args()
    LIMIT[0] = a.limit
    res = []
    if a.append and os.path.exists(a.out):
        with open(a.out) as fh:
            old = json.load(fh)
        same = (old["commit"], old["device"], old["reps"]) == (a.commit, torch.cuda.get_device_name(0), a.reps)
        assert same, f"--append: {a.out} holds another run ({old['commit']}, {old['device']}, reps {old['reps']})"
        res = old["cases"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for shape in a.shapes.split(","):
        n, E, H = (int(v) for v in shape.split("x"))
        for algo in a.algos.split(","):
            res.append(case(algo, n, E, H, a.reps))
            print(json.dumps({k: (round(v["median"], 2) if isinstance(v, dict) else v) for k, v in res[-1].items()}),
                  flush=True)
            torch.cuda.empty_cache()
            with open(a.out, "w") as fh:                                 # after every case: a long run keeps what it has
                json.dump(dict(commit=a.commit, device=torch.cuda.get_device_name(0), reps=a.reps,
                               note="ms, device events; hip = the two-tile MLP kernels, torch = D2D_FUSED_POLICY=0 "
                                    "D2D_FUSED_UPDATE=0 (the agent-stacked torch path); alternating in one process",
                               cases=res), fh, indent=1)
                fh.write("\n")


if __name__ == "__main__":
    main()
