"""TEST INFRASTRUCTURE ONLY.  A plain-torch oracle of the MLP behaviour policy (algorithms/ippo.py:54-90, 154-176):
Policy / Value forward, the Bernoulli (mean over channels) and Categorical log-probs with torch's float32 clamp,
deterministic and Philox-sampled actions with their tie masks.  Everything runs on the CPU at the dtype the caller
names (float64 for the reference, float32 for "what torch would give"); tests/test_mlp_oracle_cpu.py pins the
float32 instance to algorithms._core.Policy / Value and torch.distributions, and checks on the float64 instance
that the inputs the GPU tests draw from here are well conditioned.  The second half is the gradient oracle of the
fused PPO-update kernels (actor_grad_oracle / critic_grad_oracle, with the relu-flip envelope) and the input sets of
tests/test_update_edges_gpu.py, pinned and checked by tests/test_update_oracle_cpu.py.

Layouts are the kernels': parameters agent-stacked (w1 [N][H][F], b1 [N][H], w2 [N][A][H], b2 [N][A]; the critic
with A = 1), obs [E][N][F], probabilities [N][E][A], log-probs and values [N][E]."""
import math

import numpy as np
import torch

EPS = 2.0 ** -23     # torch.finfo(torch.float32).eps: the clamp of torch.distributions on float32 probabilities
TIE = 1e-5           # half-width of every tie mask


def make_params(N, F, H, A, seed, in_dims=None):
    """(actor, critic) dicts of float32 CPU tensors, every tensor -- biases included -- uniform in
    +-1/sqrt(fan_in) (nn.Linear's ranges) from a generator seeded with `seed`; w1's columns past in_dims[k] zero."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, fan: (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan)  # noqa: E731
    nets = []
    for a in (A, 1):
        nets.append({"w1": u((N, H, F), F), "b1": u((N, H), F), "w2": u((N, a, H), H), "b2": u((N, a), H)})
    for k, d in enumerate(in_dims or [F] * N):
        for net in nets:
            net["w1"][k, :, d:] = 0
    return nets[0], nets[1]


def make_obs(E, N, F, dims, seed, frac):
    """Env-like obs [E][N][F] float32: buffer counts in {0, 1, 2} in the first F // 3 columns, channel bits / ACKs in
    {-1, 0, 1} in the rest (all bf16-exact); frac adds uniform [0, 0.3) to every used column; columns past dims[k]
    are zero."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.zeros(E, N, F)
    D = F // 3
    obs[:, :, :D] = torch.randint(0, 3, (E, N, D), generator=g).float()
    obs[:, :, D:] = torch.randint(-1, 2, (E, N, F - D), generator=g).float()
    if frac:
        obs += torch.rand(obs.shape, generator=g) * 0.3
    for k, d in enumerate(dims or [F] * N):
        obs[:, k, d:] = 0
    return obs


def _hidden(net, obs, dtype):
    x = obs.to(dtype).transpose(0, 1)                                          # [N][E][F]
    return torch.relu(torch.baddbmm(net["b1"].to(dtype).unsqueeze(1), x, net["w1"].to(dtype).transpose(1, 2)))


def probs(actor, obs, dtype=torch.float64):
    """Policy.forward (ippo.py:69-75): softmax(W2 relu(W1 x + b1) + b2) -> [N][E][A]"""
    h = _hidden(actor, obs, dtype)
    return torch.softmax(torch.baddbmm(actor["b2"].to(dtype).unsqueeze(1), h, actor["w2"].to(dtype).transpose(1, 2)), -1)


def values(critic, obs, dtype=torch.float64):
    """Value.forward (ippo.py:84-90): V2 relu(V1 x + c1) + c2 -> [N][E]"""
    h = _hidden(critic, obs, dtype)
    return torch.baddbmm(critic["b2"].to(dtype).unsqueeze(1), h, critic["w2"].to(dtype).transpose(1, 2))[..., 0]


def bernoulli_logp(p, bits):
    """Bernoulli(probs=p).log_prob(bits).mean(-1): log(pc) / log(1 - pc) per channel, p clamped to [EPS, 1 - EPS]"""
    pc = p.clamp(EPS, 1 - EPS)
    return torch.where(bits.bool(), pc.log(), (1 - pc).log()).mean(-1)


def categorical_logp(p, ids):
    """Categorical(probs=p).log_prob(ids): log of the renormalised probability, clamped to [EPS, 1 - EPS]"""
    q = (p / p.sum(-1, keepdim=True)).clamp(EPS, 1 - EPS)
    return q.gather(-1, ids.long().unsqueeze(-1))[..., 0].log()


def logp(p, kind, actions):
    return bernoulli_logp(p, actions) if kind == "comb" else categorical_logp(p, actions)


def deterministic_actions(p, kind):
    """(actions, tie).  comb: bits [N][E][A] = p > 0.5 (ippo.py:166), tie |p - 0.5| < TIE per channel;
    chsel: ids [N][E] = lowest-index argmax (ippo.py:171), tie where the top two probabilities are closer than TIE."""
    if kind == "comb":
        return p > 0.5, (p - 0.5).abs() < TIE
    ids = p.argmax(-1)                                   # torch.argmax: the first maximal index
    if p.shape[-1] == 1:
        return ids, torch.zeros_like(ids, dtype=torch.bool)
    top = p.topk(2, -1).values
    return ids, (top[..., 0] - top[..., 1]) < TIE


def sampled_actions(p, kind, envs, agents, step, seed):
    """(actions, tie) of the kernel's Philox draw: stream 3, counter (env, agent, step, 3 << 24 | block), key seed.
    envs: the E global env indices (env_base + e); agents: the N agent indices.
    comb: word r of block ga is action 4 ga + r's, u = (w >> 8) / 2^24, bit = u < p; tie |u - p| < TIE.
    chsel: word 0 of block 0, the first j with u sum(p) < cdf_j, capped at A - 1; tie |u sum(p) - cdf_j| < TIE, any j."""
    from oracle import philox
    A = p.shape[-1]
    envs = np.asarray(envs, dtype=np.uint64)
    agents = np.asarray(agents, dtype=np.uint64)
    pn = p.double().numpy()
    if kind == "comb":
        w = philox.words(envs[None, :], agents[:, None], step, 3, 4 * ((A + 3) // 4), seed)[..., :A]   # [N][E][A]
        u = (w >> np.uint64(8)).astype(np.float64) / 16777216.0
        return torch.from_numpy(u < pn), torch.from_numpy(np.abs(u - pn) < TIE)
    w = philox.words(envs[None, :], agents[:, None], step, 3, 1, seed)[..., 0]                         # [N][E]
    u = (w >> np.uint64(8)).astype(np.float64) / 16777216.0
    cdf = np.cumsum(pn, -1)
    ut = (u * cdf[..., -1])[..., None]
    ids = np.minimum((ut >= cdf).sum(-1), A - 1)
    return torch.from_numpy(ids), torch.from_numpy((np.abs(ut - cdf) < TIE).any(-1))


def to_record(obs):
    """The compact obs record (d2dhip/record.py) of integer-valued fp32 obs [T][E][N][F] on the GPU: one byte per
    column (int8 where a column holds negatives), the bias byte 1 at column F, zeros past it."""
    from d2dhip.record import ObsRecord
    T, E, N, F = obs.shape
    R = 32 * ((F + 1 + 31) // 32)
    v = obs.round().to(torch.int32)
    assert torch.equal(v.float(), obs.float()), "record inputs must be integers"
    neg = (v < 0).reshape(-1, N, F).any(0)                                        # [N][F]
    data = torch.zeros((T, E, N, R), dtype=torch.uint8)
    data[..., :F] = (v & 0xFF).to(torch.uint8)
    data[..., F] = 1                                                                # the bias input
    sgn = torch.zeros((N, R // 32), dtype=torch.int64)
    for k in range(N):
        for c in range(F):
            if neg[k, c]:
                sgn[k, c // 32] |= 1 << (c % 32)
    sgn = torch.where(sgn >= 2 ** 31, sgn - 2 ** 32, sgn).to(torch.int32)
    return ObsRecord(data.cuda().contiguous(), F, sgn.cuda())


# ---- the shapes and batches of tests/test_policy_edges_gpu.py (here, so that the CPU test checks the same inputs)

# (kind, F, H, A): the smallest shapes at which each path of the two kernels exists
SHAPES = [
    ("comb", 1, 1, 1),        # smallest everything
    ("chsel", 2, 17, 2),
    ("comb", 3, 32, 3),
    ("chsel", 12, 33, 4),
    ("comb", 30, 64, 8),      # the headline shape
    ("chsel", 31, 65, 5),     # F + 1 = 32; nine hidden tiles' worth of rows, one row of the fifth used
    ("comb", 31, 128, 9),     # A > 8: unpaired epilogue, int16 masks; H at its maximum
    ("chsel", 23, 100, 16),
    ("comb", 32, 33, 16),     # smallest two-chunk input
    ("chsel", 46, 64, 9),
    ("comb", 63, 17, 8),      # F + 1 = 64
    ("chsel", 64, 64, 8),     # the fp32-MFMA kernel, whatever the option says
    ("comb", 64, 1, 2),
]
RNG = dict(seed=1234, env_base=77, rng_step=5)   # of every sampling launch (all nonzero)
E_EDGES = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129]
E_MAX = 129
# heterogeneous in_dims (N = 5) of two shapes
HET = {("comb", 30, 64, 8): [23, 30, 23, 30, 23], ("chsel", 12, 33, 4): [12, 9, 12, 10, 12]}


def shape_seed(kind, F, H, A):
    return (F * 131 + H) * 17 + A + (1000003 if kind == "chsel" else 0)


def batches(shape):
    """(N, E, in_dims) of a shape's runs beyond the E edges at N = 5: N = 1 and 8 at E = 129, N = 3 at E = 300 and,
    for two shapes, heterogeneous in_dims."""
    out = [(5, E_MAX, None), (1, E_MAX, None), (8, E_MAX, None), (3, 300, None)]
    if shape in HET:
        out.append((5, E_MAX, HET[shape]))
    return out


def case_inputs(shape, N, E, in_dims, frac):
    """(actor, critic, obs) of one run: the parameters depend on the shape, N and in_dims; the obs also on frac."""
    kind, F, H, A = shape
    s = shape_seed(*shape) * 64 + N * 2 + (1 if in_dims else 0)
    actor, critic = make_params(N, F, H, A, s, in_dims)
    return actor, critic, make_obs(E, N, F, in_dims, s + 7 + (100 if frac else 0), frac)


# ---- the gradient oracle of the fused PPO-update kernels (csrc/update_kernels.hip, ppo_epilogue.h): autograd over
# this file's own forward and log-prob functions at the dtype the caller names.  tests/test_update_oracle_cpu.py pins
# its float32 instance to algorithms._core.Policy / Value + torch.distributions and the reference's loss expressions.
# Samples are flat, b = t * E + e: obs [B][N][F], actions bits [N][B][A] / ids [N][B], logp_old / W / R [N][B].

U32 = 2.0 ** -24            # float32's unit roundoff
_CHUNK = 1 << 24            # [agents][B][H] elements of one autograd pass (a float64 tensor of 128 MiB)


def entropy(p, kind):
    """Bernoulli(probs=p).entropy().mean(-1) = mean_c -(p log pc + (1 - p) log(1 - pc)) (binary cross entropy of the
    clamped logits against the unclamped p), or Categorical(probs=p).entropy() = -sum q log qc, q = p / sum p"""
    if kind == "comb":
        pc = p.clamp(EPS, 1 - EPS)
        return -(p * pc.log() + (1 - p) * (1 - pc).log()).mean(-1)
    q = p / p.sum(-1, keepdim=True)
    return -(q * q.clamp(EPS, 1 - EPS).log()).sum(-1)


def _layer1(p, x, F, env):
    """relu(W1 x + b1) [n][B][H]; registers the relu-flip envelope (tools/gpu/ppo_grads_full_batch.py _flip_envelope):
    a (sample, unit) pair is ambiguous when |pre| <= 2 (F + 2) 2^-24 (|b1| + sum_j |w1_j x_j|), i.e. within twice the
    fp32 dot-product error bound of 0, where any fp32 evaluation may take either relu mask; a flipped mask at (s, h)
    moves dW1[h, :] by dA[s, h] x_s and db1[h] by dA[s, h] (dA = dL / d relu(pre))."""
    pre = torch.baddbmm(p["b1"].unsqueeze(1), x, p["w1"].transpose(1, 2))
    h = torch.relu(pre)
    with torch.no_grad():
        absum = p["b1"].abs().unsqueeze(1) + x.abs() @ p["w1"].abs().transpose(1, 2)
        amb = pre.abs() <= 2 * (F + 2) * U32 * absum
    env["n_amb"] = amb.sum((1, 2))

    def hook(dA):
        a = dA.detach().abs() * amb
        env["w1"] = a.transpose(1, 2) @ x.abs()
        env["b1"] = a.sum(1)
    h.register_hook(hook)
    return h


def _actor_part(net, obs, actions, logp_old, W, kind, clip, beta, scale, dtype):
    p = {k: v.to(dtype).clone().requires_grad_() for k, v in net.items()}
    x = obs.to(dtype).transpose(0, 1)
    env = {}
    h = _layer1(p, x, obs.shape[-1], env)
    pr = torch.softmax(torch.baddbmm(p["b2"].unsqueeze(1), h, p["w2"].transpose(1, 2)), -1)
    lp, ent = logp(pr, kind, actions), entropy(pr, kind)
    ratio, Wd = torch.exp(lp - logp_old.to(dtype)), W.to(dtype)
    s = torch.min(ratio * Wd, torch.clamp(ratio, 1 - clip, 1 + clip) * Wd)
    (scale * (-s - beta * ent).sum(1)).sum().backward()
    out = {"g_" + k: v.grad for k, v in p.items()}
    out.update(surr=s.detach().sum(1), ent=ent.detach().sum(1), probs=pr.detach(), logp=lp.detach(),
               n_amb=env["n_amb"], e_w1=env["w1"], e_b1=env["b1"])
    return out


def _critic_part(net, obs, R, scale, dtype):
    p = {k: v.to(dtype).clone().requires_grad_() for k, v in net.items()}
    x = obs.to(dtype).transpose(0, 1)
    env = {}
    h = _layer1(p, x, obs.shape[-1], env)
    v = torch.baddbmm(p["b2"].unsqueeze(1), h, p["w2"].transpose(1, 2))[..., 0]
    sq = (v - R.to(dtype)) ** 2
    (scale * sq.sum(1)).sum().backward()
    out = {"g_" + k: t.grad for k, t in p.items()}
    out.update(loss=sq.detach().sum(1), v=v.detach(), n_amb=env["n_amb"], e_w1=env["w1"], e_b1=env["b1"])
    return out


def _by_agents(fn, net, obs, per_agent, rest):
    """fn over chunks of agents (they are independent), so that no intermediate passes _CHUNK elements"""
    N, H = net["w1"].shape[:2]
    step = max(1, _CHUNK // max(1, obs.shape[0] * H))
    parts = [fn({k: v[a:a + step] for k, v in net.items()}, obs[:, a:a + step], *[t[a:a + step] for t in per_agent],
                *rest) for a in range(0, N, step)]
    out = {k: torch.cat([q[k] for q in parts]) for k in parts[0]}
    res = {"grads": {k: out.pop("g_" + k) for k in net}}
    res["env"] = {"w1": out.pop("e_w1"), "b1": out.pop("e_b1"), "w2": torch.zeros_like(res["grads"]["w2"]),
                  "b2": torch.zeros_like(res["grads"]["b2"])}
    res.update(out)
    return res


def actor_grad_oracle(actor, obs, kind, actions, logp_old, W, clip, beta, scale, dtype=torch.float64):
    """The actor loss of ppo_epilogue.h / include/d2d_hip.h per agent,
    scale * sum_s (-min(r W, clamp(r, 1 - clip, 1 + clip) W) - beta * entropy), r = exp(logp(a_s) - logp_old_s),
    with torch.min's and torch.clamp's gradient rules (a tie halves, the clamp passes inclusively) ->
    dict(grads {w1, b1, w2, b2} [N]..., env (the flip envelope, zero for w2 / b2), n_amb [N] (ambiguous pairs),
    surr [N] (sum of the min-surrogate), ent [N] (sum of the entropy), probs [N][B][A], logp [N][B])."""
    return _by_agents(_actor_part, actor, obs, (actions, logp_old, W), (kind, clip, beta, scale, dtype))


def critic_grad_oracle(critic, obs, R, scale, dtype=torch.float64):
    """scale * sum_s (V(x_s) - R_s)^2 per agent -> dict(grads, env, n_amb, loss [N] = sum (V - R)^2, v [N][B])"""
    return _by_agents(_critic_part, critic, obs, (R,), (scale, dtype))


def grad_excess(g, g64, env):
    """[N]: per agent, the largest elementwise max(|g - g64| - envelope, 0) as a share of max |g64[k]| (0 where the
    agent's float64 gradient is all zero)"""
    N = g64.shape[0]
    over = ((g.double() - g64).abs() - env).clamp(min=0).reshape(N, -1).max(1).values
    top = g64.abs().reshape(N, -1).max(1).values
    return torch.where(top > 0, over / top.clamp(min=1e-300), torch.zeros_like(over))


# ---- the cases of tests/test_update_edges_gpu.py (here, so that tests/test_update_oracle_cpu.py checks the same inputs)

# (kind, F, H, A).  KC = 2 when F + 1 > 32; HT = 2 / 4 / 8 for H <= 32 / 64 / 128; PAIR when A <= 8; on the record
# A == 8 is an instance of its own (AFIX).  Every (KC, HT, kind) x (A < 8, A == 8, A > 8) occurs.
UPD_SHAPES = [
    ("comb", 1, 1, 1),       # (1, 2)
    ("chsel", 2, 17, 2),
    ("comb", 3, 32, 3),
    ("comb", 15, 32, 4),     # the bias at column 16, the first of input tile 1
    ("comb", 5, 20, 8),
    ("comb", 10, 16, 16),
    ("chsel", 9, 16, 8),
    ("chsel", 7, 32, 12),
    ("chsel", 12, 33, 4),    # (1, 4)
    ("chsel", 12, 33, 8),
    ("chsel", 20, 40, 11),
    ("comb", 18, 40, 5),
    ("comb", 30, 64, 8),     # the headline shape
    ("comb", 24, 48, 13),
    ("chsel", 31, 65, 5),    # (1, 8); the bias in the last column of chunk 0
    ("chsel", 14, 120, 8),
    ("chsel", 23, 100, 16),
    ("comb", 9, 80, 6),
    ("comb", 22, 96, 8),
    ("comb", 31, 128, 9),
    ("comb", 35, 24, 2),     # (2, 2)
    ("comb", 63, 17, 8),     # F + 1 = 64
    ("comb", 40, 30, 12),
    ("chsel", 47, 20, 3),
    ("chsel", 52, 32, 8),
    ("chsel", 33, 32, 10),
    ("comb", 50, 50, 7),     # (2, 4)
    ("comb", 38, 64, 8),
    ("comb", 32, 33, 16),    # the bias in the first column of chunk 1
    ("chsel", 36, 64, 4),
    ("chsel", 60, 36, 8),
    ("chsel", 46, 64, 9),
]
UPD_SWEEP = dict(N=5, T=3, E=45)       # (a): 135 samples per agent, a ragged second tile


def upd_dims(F):
    """the heterogeneous in_dims of the N = 5 runs: agents 1 and 3 narrower (F <= 2: none)"""
    return None if F < 3 else [F, F - F // 4 - 1, F, F - 1, F]


UPD_EDGE_SHAPES = [("comb", 30, 64, 8), ("chsel", 46, 64, 9), ("comb", 31, 128, 9), ("chsel", 2, 17, 2)]
UPD_TE = [(1, 1), (1, 15), (1, 16), (1, 17), (1, 31), (1, 32), (1, 33), (3, 1), (2, 64), (5, 65), (4, 97)]
UPD_EDGE_N = [1, 5]
# (c): N = 256; (25, 70): tiles_per_t = 3 with a ragged last tile; (75, 9): tiles_per_t = 1.  75 tiles each.
UPD_TILE_N = 256
UPD_TILE_CASES = [
    (("comb", 15, 32, 4), 25, 70), (("chsel", 7, 32, 12), 75, 9),          # (1, 2)
    (("comb", 30, 64, 8), 75, 9), (("chsel", 12, 33, 4), 25, 70),          # (1, 4)
    (("comb", 31, 128, 9), 25, 70), (("chsel", 31, 65, 5), 75, 9),         # (1, 8)
    (("comb", 63, 17, 8), 75, 9), (("chsel", 33, 32, 10), 25, 70),         # (2, 2)
    (("comb", 32, 33, 16), 25, 70), (("chsel", 46, 64, 9), 75, 9),         # (2, 4)
]
# (d): (shape, T, E, mode); the last entry's only inexact value is one element (mode "single")
UPD_MIXED_CASES = [
    (("chsel", 12, 33, 4), 25, 70, "mixed"), (("comb", 32, 33, 16), 25, 70, "mixed"),
    (("comb", 31, 128, 9), 75, 9, "mixed"), (("comb", 30, 64, 8), 25, 70, "mixed"),
    (("comb", 63, 17, 8), 25, 70, "mixed"), (("comb", 30, 64, 8), 25, 70, "single"),
]
UPD_SATURATED = [("comb", 30, 64, 8), ("chsel", 12, 33, 4)]
SINGLE_AT = (7, 69, 3)      # (t, e, k) of mode "single"'s element: the last real sample of the ragged tile of slot 7


CLIP_EDGES = (0.8, 0.9, 1.1, 1.2)      # 1 -+ clip of the clips the GPU tests use (0.1, 0.2)


def _tile_hash(T, tiles, N):
    """a 64-bit mix of (slot, 32-env tile, agent) -> uint64 [T][tiles][N] (no period in any index)"""
    t, j, k = np.meshgrid(np.arange(T, dtype=np.uint64), np.arange(tiles, dtype=np.uint64),
                          np.arange(N, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = t * np.uint64(0x9E3779B97F4A7C15) + j * np.uint64(0xBF58476D1CE4E5B9) + k * np.uint64(0x94D049BB133111EB)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fractional_tiles(T, E, N):
    """bool [T][tiles][N]: the (slot, 32-env tile, agent) triples of mode "mixed" that hold bf16-inexact values"""
    return torch.from_numpy(((_tile_hash(T, (E + 31) // 32, N) >> np.uint64(40)) & np.uint64(1)).astype(bool))


def mix_fractions(obs, dims, seed):
    """Mode "mixed" on integer obs [T][E][N][F]: in columns 0, F // 2 and F - 1 (where the agent has them), half the
    samples of every tile -- its first always -- get 1 / n: n in {3, 5, 6, 7} (bf16-inexact) in a fractional tile,
    n in {2, 4} (bf16-exact non-integers) in every other, one n per (slot, tile, agent)."""
    T, E, N, F = obs.shape
    h = _tile_hash(T, (E + 31) // 32, N)
    frac = (h >> np.uint64(40)) & np.uint64(1)
    sel = (h >> np.uint64(44)).astype(np.int64)
    n = np.where(frac == 1, np.array([3, 5, 6, 7])[sel % 4], np.array([2, 4])[sel % 2])
    val = (1.0 / torch.from_numpy(n).float()).repeat_interleave(32, dim=1)[:, :E]          # [T][E][N]
    g = torch.Generator().manual_seed(seed)
    put = torch.rand((T, E, N), generator=g) < 0.5
    put[:, ::32] = True
    out = obs.clone()
    for c in sorted({0, F // 2, F - 1}):
        ok = put & torch.tensor([c < d for d in (dims or [F] * N)])
        out[..., c] = torch.where(ok, val, out[..., c])
    return out


def update_inputs(shape, N, T, E, dims=None, mode="int", saturated=False):
    """One run's inputs, all CPU float32 unless noted: actor / critic (make_params; saturated: b2[:, 0] += 40), obs
    [T][E][N][F] (make_obs; mode "frac": every used column + U[0, 0.3); "mixed" / "single": see mix_fractions /
    SINGLE_AT), acts (bits bool [N][B][A] / ids int64 [N][B]), logp_old = the float64 oracle's log-prob + U(-0.3, 0.3)
    (ratios in [0.74, 1.35]: inside and on both sides of a clip of 0.1 or 0.2, none within 5e-4 of CLIP_EDGES), W
    (normal, one in ten exactly 0), R (normal around 1: returns of nonnegative rewards, so that the critic's db2 is no
    cancelling sum), each [N][B] with b = t * E + e."""
    kind, F, H, A = shape
    B = T * E
    s = (shape_seed(*shape) * 64 + N * 2 + (1 if dims else 0)) * 1009 + T * 131 + E
    actor, critic = make_params(N, F, H, A, s, dims)
    if saturated:
        actor["b2"][:, 0] += 40
    obs = make_obs(B, N, F, dims, s + 7 + (100 if mode == "frac" else 0), mode == "frac").view(T, E, N, F)
    if mode == "mixed":
        obs = mix_fractions(obs, dims, s + 11)
    elif mode == "single":
        t, e, k = SINGLE_AT
        assert t < T and e == E - 1 and E % 32 and k < N
        obs[t, e, k, F // 2] = 1.0 / 3.0
    g = torch.Generator().manual_seed(s + 13)
    acts = (torch.rand((N, B, A), generator=g) < 0.4) if kind == "comb" else torch.randint(0, A, (N, B), generator=g)
    lp = logp(probs(actor, obs.view(B, N, F)), kind, acts)
    d = torch.rand((N, B), generator=g, dtype=torch.float64) * 0.6 - 0.3
    for edge in CLIP_EDGES:          # the surrogate's gradient jumps where the ratio crosses a clip edge: keep clear
        d = torch.where((torch.exp(-d) - edge).abs() < 1e-3, d + 4e-3, d)
    logp_old = (lp + d).float()
    W = torch.randn((N, B), generator=g)
    W[torch.rand((N, B), generator=g) < 0.1] = 0.0
    R = 1.0 + torch.randn((N, B), generator=g)
    return dict(shape=shape, N=N, T=T, E=E, dims=dims, mode=mode, actor=actor, critic=critic, obs=obs, acts=acts,
                logp_old=logp_old, W=W, R=R)


def update_input_sets():
    """(label, update_inputs arguments) of every input set tests/test_update_edges_gpu.py runs"""
    out = []
    for shape in UPD_SHAPES:
        for mode in ("int", "frac"):
            out.append((f"sweep {shape} {mode}", dict(shape=shape, dims=upd_dims(shape[1]), mode=mode, **UPD_SWEEP)))
    for shape in UPD_EDGE_SHAPES:
        for N in UPD_EDGE_N:
            for T, E in UPD_TE:
                out.append((f"edge {shape} N{N} T{T} E{E}", dict(shape=shape, N=N, T=T, E=E)))
    for shape, T, E in UPD_TILE_CASES:
        out.append((f"tiles {shape} T{T} E{E}", dict(shape=shape, N=UPD_TILE_N, T=T, E=E)))
    for shape, T, E, mode in UPD_MIXED_CASES:
        out.append((f"{mode} {shape} T{T} E{E}", dict(shape=shape, N=UPD_TILE_N, T=T, E=E, mode=mode)))
    for shape in UPD_SATURATED:
        out.append((f"saturated {shape}", dict(shape=shape, dims=upd_dims(shape[1]), saturated=True, **UPD_SWEEP)))
    return out
