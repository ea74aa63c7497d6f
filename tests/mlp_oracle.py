"""TEST INFRASTRUCTURE ONLY.  A plain-torch oracle of the MLP behaviour policy (algorithms/ippo.py:54-90, 154-176):
Policy / Value forward, the Bernoulli (mean over channels) and Categorical log-probs with torch's float32 clamp,
deterministic and Philox-sampled actions with their tie masks.  Everything runs on the CPU at the dtype the caller
names (float64 for the reference, float32 for "what torch would give"); tests/test_mlp_oracle_cpu.py pins the
float32 instance to algorithms._core.Policy / Value and torch.distributions, and checks on the float64 instance
that the inputs the GPU tests draw from here are well conditioned.

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
