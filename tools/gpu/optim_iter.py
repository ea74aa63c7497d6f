"""The optimizer phase of a training iteration on d2d_adam_step (fused_optimizer=True: d2dhip.optim.StackedAdam,
csrc/optim_kernels.hip) against torch's Adam + the per-agent clip, the learners' default, in the same process,
alternating.

  python tools/gpu/optim_iter.py --out profiles/optim/bench.json --commit $(git rev-parse --short HEAD)

Per shape two learners are built on envs of their own with the same seeds, one with fused_optimizer=True.  Timed with
device events after one warm-up iteration of each, 5 repetitions, the two learners alternating: the optimizer phase
alone (the learners' "adam" phase marks: clip + step of every optimizer of every epoch; for iRDQN the optimizer.step
of one update) and one whole iteration (rollout + n_epoch epochs; for iRDQN one whole update).  Medians, with the torch
path's min-max.  Shapes: configs[1] (16 agents x 4 channels, 4,096 envs, D2D-PPO MLP), c5 at 8 and 256 agents, the
headline iPPO update (64 agents, 2,048 envs, H = 64), xp_load's GRU D2D-PPO at 256 envs, iRDQN at 8 and 64 agents."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "d2d-ppo_amd")
sys.path[:0] = [ROOT, PKG]

T_EP = 200


class PhaseTimer:
    """The learners call _phase(name) after each phase: device events on the current stream."""

    def __init__(self):
        self.marks = []
        self.prev = self._event()

    @staticmethod
    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def mark(self, name):
        e = self._event()
        self.marks.append((name, self.prev, e))
        self.prev = e

    def total_ms(self, name):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for n, a, b in self.marks if n == name)


def comb_env(N, E, seed):
    from envs.combinatorial_env import CombinatorialEnv
    return CombinatorialEnv(n_agents=N, n_channels=8, deadlines=np.full(N, 7), lbdas=np.full(N, 1 / 14), period=None,
                            arrival_probs=None, offsets=None, episode_length=T_EP, traffic_model="aperiodic",
                            periodic_devices=[], channel_switch=np.ones((N, 8)) * 0.8, n_envs=E, device="cuda:0", seed=seed)


def headline_env(E, seed):
    from envs.combinatorial_env import CombinatorialEnv
    cs8 = np.array(json.load(open(os.path.join(PKG, "combinatorial_load", "channel_switch_8.json")))["__nd__"])
    N = 64
    return CombinatorialEnv(n_agents=N, n_channels=8, deadlines=np.array([7, 14] * (N // 2)), lbdas=np.full(N, 0.5),
                            period=np.full(N, 2), arrival_probs=np.resize(np.array([.2, .4, .8, 1, 1, 1]), N),
                            offsets=np.zeros(N), episode_length=T_EP, traffic_model="heterogeneous",
                            homogeneous_size=True, periodic_devices=[k for k in range(N) if k % 6 < 3],
                            channel_switch=np.resize(cs8, (N, 8)), n_envs=E, device="cuda:0", seed=seed)


def chsel_env(E, seed):
    from envs.channel_selection_env import ChannelSelectionEnv
    N = 16
    return ChannelSelectionEnv(n_agents=N, n_channels=4, deadlines=np.full(N, 7), lbdas=np.full(N, 1 / 3.5),
                               period=np.full(N, 2), arrival_probs=np.full(N, 0.5), offsets=np.zeros(N),
                               episode_length=T_EP, traffic_model="aperiodic", periodic_devices=[],
                               channel_switch=np.full(5, 0.8), n_envs=E, device="cuda:0", seed=seed)


def d2d(env, comb, **kw):
    from algorithms.d2d_ppo import D2DPPO
    return lambda fused: D2DPPO(env(), hidden_size=64, gamma=0.4, policy_lr=3e-4, value_lr=1e-3, beta_entropy=0.01,
                                device="cuda", combinatorial=comb, early_stopping=False, fused_optimizer=fused, **kw)


def ippo(env):
    from algorithms.ippo import iPPO
    return lambda fused: iPPO(env(), hidden_size=64, gamma=0.4, device="cuda", combinatorial=True, early_stopping=False,
                              fused_optimizer=fused)


def irdqn(N):
    from algorithms.irdqn import iRDQN
    return lambda fused: iRDQN(comb_env(N, 64, 24), history_len=5, replay_start_size=64, replay_buffer_size=10 ** 5,
                               minibatch_size=32, fused_optimizer=fused)


# name -> (kind, learner factory, epochs per iteration)
CASES = {
    "configs1_d2d_mlp_16x4096": ("ppo", lambda: d2d(lambda: chsel_env(4096, 21), False), 5),
    "c5_d2d_mlp_8x4096": ("ppo", lambda: d2d(lambda: comb_env(8, 4096, 22), True), 5),
    "c5_d2d_mlp_256x4096": ("ppo", lambda: d2d(lambda: comb_env(256, 4096, 22), True), 5),
    "headline_ippo_mlp_64x2048": ("ppo", lambda: ippo(lambda: headline_env(2048, 11)), 1),
    "xp_load_d2d_gru_64x256": ("ppo", lambda: d2d(lambda: headline_env(256, 11), True, useRNN=True, history_len=64), 2),
    "irdqn_8_h100": ("irdqn", lambda: irdqn(8), 1),
    "irdqn_64_h100": ("irdqn", lambda: irdqn(64), 1),
}


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], all=v)


def ppo_rep(lr, n_epoch):
    """(optimizer phase ms, iteration ms) of one iteration"""
    E = lr.env.batch().E
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lr.phase_timer = PhaseTimer()
    a.record()
    if "defer_values" in lr._rollout.__code__.co_varnames:               # iPPO, as its train() calls it
        ro = lr._rollout(E, defer_values=True)
    else:
        ro = lr._rollout(E)
    upd = lr._update_state(ro)
    for _ in range(n_epoch):
        lr._update_epoch(ro, upd)
    b.record()
    b.synchronize()
    adam = lr.phase_timer.total_ms("adam")
    lr.phase_timer = None
    return adam, a.elapsed_time(b)


def irdqn_prepare(ln):
    """Fill the replay ring with two waves of episodes, so that updates can be timed on their own."""
    b = ln._bind_env()
    b.spec.arrival_kinds()
    ln._alloc_ring(b, 4)
    for w in range(2):
        ln._train_wave(b, w * b.E)
    return b.E


def irdqn_rep(ln, E):
    """(optimizer.step ms, update ms): one whole update, then the step alone on the gradients it left"""
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    ln._update(E)
    b.record()
    ln.optimizer.step()
    c.record()
    c.synchronize()
    return b.elapsed_time(c), a.elapsed_time(b)


def case(name, reps):
    kind, factory, n_epoch = CASES[name]
    learners = {}
    for path, fused in (("torch", False), ("fused", True)):
        torch.manual_seed(3)
        np.random.seed(3)
        learners[path] = factory()(fused)
    E = {p: irdqn_prepare(ln) for p, ln in learners.items()} if kind == "irdqn" else None
    run = (lambda p: irdqn_rep(learners[p], E[p])) if kind == "irdqn" else (lambda p: ppo_rep(learners[p], n_epoch))
    for p in learners:                                                   # one warm-up of each
        run(p)
    torch.cuda.synchronize()
    times = {}
    for _ in range(reps):
        for p in learners:
            opt_ms, it_ms = run(p)
            times.setdefault(f"optimizer_ms_{p}", []).append(opt_ms)
            times.setdefault(f"iteration_ms_{p}", []).append(it_ms)
    r = dict(case=name, epochs=n_epoch, **{k: stats(v) for k, v in times.items()})
    r["optimizer_speedup"] = r["optimizer_ms_torch"]["median"] / r["optimizer_ms_fused"]["median"]
    r["iteration_speedup"] = r["iteration_ms_torch"]["median"] / r["iteration_ms_fused"]["median"]
    r["optimizer_share_torch"] = r["optimizer_ms_torch"]["median"] / r["iteration_ms_torch"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim", "bench.json"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    res = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.cases.split(","):
        res.append(case(name, a.reps))
        print(json.dumps({k: (round(v["median"], 3) if isinstance(v, dict) else v) for k, v in res[-1].items()}),
              flush=True)
        torch.cuda.empty_cache()
        with open(a.out, "w") as fh:                                     # after every case: a long run keeps what it has
            json.dump(dict(commit=a.commit, device=torch.cuda.get_device_name(0), reps=a.reps,
                           note="ms, device events; torch = torch.optim.Adam + grad_norm_clip_ / clip_grad_norm_ (the "
                                "default), fused = fused_optimizer=True (d2d_adam_step); alternating in one process; "
                                "optimizer = the learners' adam phase over all epochs of the iteration (iRDQN: one "
                                "optimizer.step), iteration = rollout + epochs (iRDQN: one update)",
                           cases=res), fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
