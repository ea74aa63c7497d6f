"""Plain-torch oracle of iRDQN's network and TD update (/root/reference/algorithms/irdqn.py:58-86, 133-148), shared by
tests/test_irdqn_cpu.py (which pins it to the reference's recorded losses and gradients, tests/golden/irdqn_*.npz) and
tests/test_irdqn_gpu.py (which holds the kernels to it)."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN

SD_NAMES = {"w_ih": "lstm.weight_ih_l0", "w_hh": "lstm.weight_hh_l0", "b_ih": "lstm.bias_ih_l0", "b_hh": "lstm.bias_hh_l0",
            "w1": "layers.0.weight", "b1": "layers.0.bias", "w2": "layers.2.weight", "b2": "layers.2.bias",
            "w3": "layers.4.weight", "b3": "layers.4.bias"}


def net_q(p, win):
    """Q [N][B][A] of windows win [N][B][S][F] (torch.nn.GRU's formula, gate order r, z, n; h0 = 0)."""
    n, B, S, _ = win.shape
    H = p["w_hh"].shape[2]
    h = torch.zeros(n, B, H, dtype=win.dtype)
    for s in range(S):
        gi = torch.baddbmm(p["b_ih"].unsqueeze(1), win[:, :, s], p["w_ih"].transpose(1, 2))
        gh = torch.baddbmm(p["b_hh"].unsqueeze(1), h, p["w_hh"].transpose(1, 2))
        r = torch.sigmoid(gi[..., :H] + gh[..., :H])
        z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
        c = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
        h = (1 - z) * c + z * h
    y = torch.relu(torch.baddbmm(p["b1"].unsqueeze(1), h, p["w1"].transpose(1, 2)))
    y = torch.relu(torch.baddbmm(p["b2"].unsqueeze(1), y, p["w2"].transpose(1, 2)))
    return torch.baddbmm(p["b3"].unsqueeze(1), y, p["w3"].transpose(1, 2))


def td_loss(p, pt, states, nexts, act, reward, done, gamma, loss):
    """Per-agent TD loss [N] and delta [N][B]: states / nexts [N][B][L][F], act [N][B] int64, reward [N][B], done [B]."""
    with torch.no_grad():
        qt = net_q(pt, nexts).max(-1).values
    qa = net_q(p, states).gather(2, act.unsqueeze(-1)).squeeze(-1)
    td = reward + (1 - done).unsqueeze(0) * gamma * qt
    delta = qa - td
    if loss == "huber":
        return torch.nn.functional.smooth_l1_loss(qa, td, reduction="none").mean(1), delta.detach()
    return (delta ** 2).mean(1), delta.detach()


def load_case(loss):
    zc = np.load(os.path.join(GOLDEN, "irdqn_common.npz"))
    z = np.load(os.path.join(GOLDEN, f"irdqn_{loss}.npz"))
    return zc, z, json.loads(str(zc["params_json"]))


def stacked(z, prefix, n_agents, dtype=torch.float64):
    """Agent-stacked parameters from the per-agent state_dicts stored under prefix.format(i)."""
    return {k: torch.stack([torch.from_numpy(z[f"{prefix.format(i)}/{sd}"].copy()) for i in range(n_agents)]).to(dtype)
            for k, sd in SD_NAMES.items()}


def chunk_batch(zc, starts, L, capacity, dtype=torch.float64):
    """The minibatch ReplayBuffer.sample_chunk (irdqn.py:24-42) builds from the recorded episodes through a deque of
    `capacity`: chunk i = retained transitions starts[i] .. starts[i] + L - 1; the loss takes the last one's action,
    reward and done (irdqn.py:292-297)."""
    obs = torch.from_numpy(zc["buffer/obs"]).to(dtype)                      # [episodes][T + 1][N][F]
    n_ep, T = obs.shape[0], obs.shape[1] - 1
    first = max(0, n_ep * T - capacity)
    ms = [[first + int(s) + j for j in range(L)] for s in starts]
    st = torch.stack([torch.stack([obs[m // T, m % T] for m in row]) for row in ms])          # [B][L][N][F]
    nx = torch.stack([torch.stack([obs[m // T, m % T + 1] for m in row]) for row in ms])
    last = [row[-1] for row in ms]
    act = torch.from_numpy(zc["buffer/actions"][last]).t().contiguous()      # [N][B]
    rew = torch.from_numpy(zc["buffer/rewards"][last]).to(dtype).t().contiguous()
    done = torch.from_numpy(zc["buffer/done"][last].astype(np.float64)).to(dtype)
    return st.permute(2, 0, 1, 3).contiguous(), nx.permute(2, 0, 1, 3).contiguous(), act, rew, done


def trajectory(zc, z, cfg, loss, dtype=torch.float64):
    """The K recorded updates re-run on the oracle (Adam as DQN.__init__ builds it, irdqn.py:130): per update the
    losses [N], deltas [N][B] and gradients, and the final parameters."""
    lk = cfg["learner"]
    N = cfg["env"]["n_agents"]
    p = {k: v.requires_grad_() for k, v in stacked(zc, "weights/agent{}/network", N, dtype).items()}
    pt = stacked(zc, "weights/agent{}/network", N, dtype)                   # the target: a copy, never synced here
    opt = torch.optim.Adam(list(p.values()), lr=lk["learning_rate"], eps=1e-8)
    steps = []
    for u in range(int(z["K"])):
        batch = chunk_batch(zc, z[f"upd/{u}/starts"], lk["history_len"], lk["replay_buffer_size"], dtype)
        ls, delta = td_loss(p, pt, *batch, lk["gamma"], loss)
        opt.zero_grad()
        ls.sum().backward()
        steps.append(dict(loss=ls.detach().clone(), delta=delta, grads={k: v.grad.clone() for k, v in p.items()}))
        opt.step()
    return steps, {k: v.detach() for k, v in p.items()}


def env_kwargs(cfg):
    return {k: (np.array(v["__nd__"], dtype=v["dtype"]) if isinstance(v, dict) else v) for k, v in cfg["env"].items()}
