"""iRDQN slot / update timing: the HIP kernels (d2dhip/rdqn.py) against the stacked-torch path (gru_window + baddbmm
head, autograd for the update) in the same process, alternating, on the drivers' iRDQN block (xp_load.py:112-126,
xp_n_agents.py:116-130): 8 channels (30 inputs), hidden 100, history_len = n_agents, minibatch 64.

  python tools/gpu/rdqn_iter.py --out profiles/rdqn/bench.json --commit $(git rev-parse --short HEAD)

Per (n_agents, E): one acting slot over E envs (full window) and one update (target max-Q + gradients; Adam is the
same torch step on both paths and is left out).  Warm, stream events around every repetition, median of >= 50."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    r.update({f"slot_ms_{k}": v for k, v in timed({"hip": hip_slot, "torch": torch_slot}, reps).items()})
    r.update({f"update_ms_{k}": v for k, v in timed({"hip": hip_update, "torch": torch_update}, reps).items()})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rdqn", "bench.json"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--agents", default="8,64")
    ap.add_argument("--envs", default="1,256")
    a = ap.parse_args()
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
