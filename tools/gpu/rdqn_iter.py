"""iRDQN slot / update timing: the HIP kernels (d2dhip/rdqn.py) against the stacked-torch path (gru_window + baddbmm
head, autograd for the update) in the same process, alternating, on the drivers' iRDQN block (xp_load.py:112-126,
xp_n_agents.py:116-130): 8 channels (30 inputs), hidden 100, history_len = n_agents, minibatch 64.

  python tools/gpu/rdqn_iter.py --out profiles/rdqn/bench.json --commit $(git rev-parse --short HEAD)

Per (n_agents, E): one acting slot over E envs (full window) and one update (target max-Q + gradients; Adam is the
same torch step on both paths and is left out), on the fp32 ring and on the compact obs record.  Warm, stream events
around every repetition, median of >= 50.

The acting-episode leg (the record ring and the carried acting state against a parent build):

  python tools/gpu/rdqn_iter.py --episodes --parent-root <a built checkout of the parent commit> \
      --out profiles/rdqn/record_carry.json --commit <this> --parent-commit <parent>

One episode of T = 200 acting slots, env step included, at n_agents = history_len in {8, 64, 256} x E in {1, 256},
for {fp32, record} x {recompute, carry}.  Every repetition is a fresh child process of THIS script per build
(--root: whose packages it imports): the parent's fp32 + recompute leg, this build's fp32 + recompute leg in a like
process, this build's other three legs, alternating, 5 repetitions; a child warms every shape and leg with a whole
episode, then times one episode per leg with device events.  The JSON holds every time, the medians and min-max, whether this
build's fp32 + recompute median lies within the parent's own min-max spread of the parent's median, and the carry
crossover (the smallest history_len from which carry is no slower than the parent at every E)."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--root" in sys.argv:                                                  # the build a child measures
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path[:0] = [ROOT, os.path.join(ROOT, "d2d-ppo_amd")]

from algorithms._core import gru_window  # noqa: E402
from d2dhip import rdqn  # noqa: E402


def torch_q(p, win):
    h = gru_window(win, p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"])
    y = torch.relu(torch.baddbmm(p["b1"].unsqueeze(1), h, p["w1"].transpose(1, 2)))
    y = torch.relu(torch.baddbmm(p["b2"].unsqueeze(1), y, p["w2"].transpose(1, 2)))
    return torch.baddbmm(p["b3"].unsqueeze(1), y, p["w3"].transpose(1, 2))


def windows(ring, samples, L, shift=0):
    """[N][B][L][F] windows of plain-row samples (env, last, L) -- the gather the kernels do in place."""
    e, last = samples[:, 0].long(), samples[:, 1].long() + shift
    rows = last.view(-1, 1) - (L - 1) + torch.arange(L, device=ring.device).view(1, -1)
    return ring[rows % ring.shape[0], e.view(-1, 1)].permute(2, 0, 1, 3)


def timed(fns, reps):
    """Median ms of each fn, run alternately (events around every call)."""
    times = {k: [] for k in fns}
    for _ in range(5):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def case(n, E, reps, B=64, F=30, H=100, A=8):
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(n + E)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / H ** 0.5).to(dev)  # noqa: E731
    p = {"w_ih": u(n, 3 * H, F), "w_hh": u(n, 3 * H, H), "b_ih": u(n, 3 * H), "b_hh": u(n, 3 * H), "w1": u(n, H, H),
         "b1": u(n, H), "w2": u(n, H, H), "b2": u(n, H), "w3": u(n, A, H), "b3": u(n, A)}
    L = n                                                                 # the drivers set history_len = n_agents
    rows = 2 * L + 2
    ring = torch.randint(0, 3, (rows, E, n, F), generator=g).float().to(dev)
    slot = torch.tensor([(e, rows - 2, L) for e in range(E)], dtype=torch.int32, device=dev)
    upd = torch.tensor([(int(torch.randint(0, E, (1,), generator=g)), L + b % L, L) for b in range(B)],
                       dtype=torch.int32, device=dev)
    act = torch.ones((B, n), dtype=torch.uint8, device=dev)
    rew = torch.randn((B, n), generator=g).to(dev)
    done = torch.zeros((B,), dtype=torch.uint8, device=dev)
    pt = {k: v.clone().requires_grad_() for k, v in p.items()}
    out = {}
    from d2dhip import record
    rec = record.encode(ring, torch.zeros((n, 1), dtype=torch.int32, device=dev))   # the same rows, 32 B each

    def rec_slot():
        rdqn.q_values(p, rec, slot, mode="eps", eps=0.1, want_q=False, want_qmax=False, out=out)

    def rec_update():
        qm = rdqn.q_values(p, rec, upd, row_shift=0, want_q=False, want_action=False)[1]
        rdqn.grads(p, rec, upd, L, act, rew, done, qm, 0.4, "huber")

    def hip_slot():
        rdqn.q_values(p, ring, slot, mode="eps", eps=0.1, want_q=False, want_qmax=False, out=out)

    def torch_slot():
        with torch.no_grad():
            q = torch_q(p, windows(ring, slot, L))
            greedy = q.argmax(-1).t()
            explore = torch.rand(E, n, device=dev) < 0.1
            a = torch.where(explore, torch.randint(0, 2, (E, n), device=dev), greedy)
            return (1 << a).to(torch.uint8)

    def hip_update():
        qm = rdqn.q_values(p, ring, upd, row_shift=0, want_q=False, want_action=False)[1]
        rdqn.grads(p, ring, upd, L, act, rew, done, qm, 0.4, "huber")

    def torch_update():
        with torch.no_grad():
            qm = torch_q(p, windows(ring, upd, L)).max(-1).values
        q = torch_q(pt, windows(ring, upd, L))[..., 0]
        td = rew.t() + 0.4 * qm
        loss = torch.nn.functional.smooth_l1_loss(q, td, reduction="none").mean(1).sum()
        for v in pt.values():
            v.grad = None
        loss.backward()

    r = dict(n_agents=n, E=E, L=L, minibatch=B)
    r.update({f"slot_ms_{k}": v for k, v in
              timed({"hip": hip_slot, "hip_record": rec_slot, "torch": torch_slot}, reps).items()})
    r.update({f"update_ms_{k}": v for k, v in
              timed({"hip": hip_update, "hip_record": rec_update, "torch": torch_update}, reps).items()})
    return r


# --------------------------------------------------------------------------------------- the acting episode
EP_T, EP_LEGS = 200, ("f32_recompute", "f32_carry", "record_recompute", "record_carry")


def episode_case(n, E, legs, F=30, H=100, A=8):
    """ms of one acting episode (reset + T x (d2d_rdqn_q launch, env step)) per leg, on the drivers' env block."""
    import numpy as np
    from envs.combinatorial_env import CombinatorialEnv
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(n + E)
    u = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) / H ** 0.5).to(dev)  # noqa: E731
    p = {"w_ih": u(n, 3 * H, F), "w_hh": u(n, 3 * H, H), "b_ih": u(n, 3 * H), "b_hh": u(n, 3 * H), "w1": u(n, H, H),
         "b1": u(n, H), "w2": u(n, H, H), "b2": u(n, H), "w3": u(n, A, H), "b3": u(n, A)}
    env = CombinatorialEnv(n_agents=n, n_channels=8, deadlines=np.resize(np.array([7, 14]), n), lbdas=np.full(n, 0.5),
                           period=np.full(n, 2), arrival_probs=np.resize(np.array([.2, .4, .8, 1, 1, 1]), n),
                           offsets=np.zeros(n), episode_length=EP_T, traffic_model="heterogeneous",
                           homogeneous_size=True, periodic_devices=[k for k in range(n) if k % 6 < 3],
                           channel_switch=np.full((n, 8), 0.3), n_envs=E, device="cuda:0", seed=1)
    b = env.batch()
    assert b.spec.F == F and b.spec.N == n
    T, L = EP_T, n                                                        # the drivers set history_len = n_agents
    rings = {"f32": torch.zeros((T + 1, E, n, F), dtype=torch.float32, device=dev)}
    if any(leg.startswith("record") for leg in legs):
        rings["record"] = b.record_buffer((T + 1,))
    acts = torch.zeros((E, n), dtype=b.action_buffer().dtype, device=dev)
    rew = torch.zeros((E,), dtype=torch.int32, device=dev)
    s = torch.zeros((E, 3), dtype=torch.int32, device=dev)
    s[:, 0] = torch.arange(E, dtype=torch.int32, device=dev)
    out = {"action": acts}

    def episode(leg):
        fmt, how = leg.split("_")
        ring = rings[fmt]
        carry = rdqn.CarryState() if how == "carry" else None
        b.reset(want_obs=True, out_obs=ring[0])
        for t in range(T):
            S = min(t + 1, L)
            s[:, 1] = t
            s[:, 2] = S
            kw = dict(carry=carry, row=t, window=S) if carry is not None else {}
            rdqn.q_values(p, ring, s, mode="eps", eps=0.1, rng_step=t, want_q=False, want_qmax=False, out=out, **kw)
            b.step(acts, want_obs=True, out_obs=ring[t + 1], out_reward=rew)
        return carry

    res = {}
    with torch.no_grad():
        for leg in legs:                                                  # warm every leg with a whole episode
            c = episode(leg)
            if c is not None:
                assert c.carried == min(L, T) - 1, (c.carried, L)
        torch.cuda.synchronize()
        for leg in legs:
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            episode(leg)
            z.record()
            z.synchronize()
            res[leg] = a.elapsed_time(z)
    return res


def episode_child(a):
    """One repetition of one build: a JSON line per shape."""
    legs = tuple(a.legs.split(","))
    for n in (int(x) for x in a.agents.split(",")):
        for E in (int(x) for x in a.envs.split(",")):
            print("EP " + json.dumps(dict(n_agents=n, E=E, ms=episode_case(n, E, legs))), flush=True)


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], all=v)


def episode_driver(a):
    """Alternate children of the parent build and of this one (this process never opens the GPU itself)."""
    # the fp32 + recompute leg of this build runs in a process of its own, like the parent's: the same warm-up and
    # the same allocations before the timed episode, so the two differ by the build alone
    builds = (("parent", os.path.abspath(a.parent_root), EP_LEGS[:1]), ("branch", ROOT, EP_LEGS[:1]),
              ("branch", ROOT, EP_LEGS[1:]))
    times = {}
    for rep_ in range(a.ep_reps):
        for name, root, legs in builds:
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--episode-child", "--agents", a.agents,
                   "--envs", a.envs, "--legs", ",".join(legs)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"{name} child failed ({r.returncode}) in repetition {rep_}: stopping")
            for ln in r.stdout.splitlines():
                if ln.startswith("EP "):
                    d = json.loads(ln[3:])
                    for leg, ms in d["ms"].items():
                        times.setdefault((d["n_agents"], d["E"]), {}).setdefault(f"{name}_{leg}", []).append(ms)
            print(f"repetition {rep_} {name} {','.join(legs)} done", flush=True)
    cases, slower = [], set()
    for (n, E), legs in sorted(times.items()):
        c = dict(n_agents=n, E=E, history_len=n, T=EP_T, episode_ms={k: stats(v) for k, v in legs.items()})
        par, own = c["episode_ms"]["parent_f32_recompute"], c["episode_ms"]["branch_f32_recompute"]
        c["fp32_recompute_within_parent_spread"] = abs(own["median"] - par["median"]) <= par["max"] - par["min"]
        c["carry_vs_parent"] = c["episode_ms"]["branch_f32_carry"]["median"] / par["median"]
        c["record_carry_vs_parent"] = c["episode_ms"]["branch_record_carry"]["median"] / par["median"]
        if c["carry_vs_parent"] > 1.0:
            slower.add(n)
        cases.append(c)
        print(json.dumps({k: v for k, v in c.items() if k != "episode_ms"} |
                         {k: round(v["median"], 2) for k, v in c["episode_ms"].items()}), flush=True)
    Ls = sorted({n for n, _ in times})
    above = [L for L in Ls if all(m not in slower for m in Ls if m >= L)]
    res = dict(commit=a.commit, parent_commit=a.parent_commit, reps=a.ep_reps, T=EP_T,
               note="ms of one acting episode: reset + T x (d2d_rdqn_q launch + env step), host launches included; "
                    "a fresh process per build and repetition, parent and branch alternating",
               carry_crossover_history_len=above[0] if above else None, cases=cases)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdqn", "bench.json"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--agents", default="8,64")
    ap.add_argument("--envs", default="1,256")
    ap.add_argument("--root", default=None, help="the checkout whose packages to import (default: this one)")
    ap.add_argument("--episodes", action="store_true", help="the acting-episode leg against --parent-root")
    ap.add_argument("--episode-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--legs", default=EP_LEGS[0], help=argparse.SUPPRESS)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-commit", default="unknown")
    ap.add_argument("--ep-reps", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.episode_child:
        return episode_child(a)
    if a.episodes:
        if a.agents == "8,64":
            a.agents = "8,64,256"
        return episode_driver(a)
    res = []
    for n in (int(x) for x in a.agents.split(",")):
        for E in (int(x) for x in a.envs.split(",")):
            res.append(case(n, E, a.reps))
            print(json.dumps(res[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(commit=a.commit, device=torch.cuda.get_device_name(0), reps=a.reps, cases=res), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
