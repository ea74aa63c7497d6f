"""TEST INFRASTRUCTURE ONLY.  The shapes and input sets of the tests of the MLP kernels with 17..32 action ids
(csrc/mlp_actions_kernels.hip), shared by tests/test_mlp_actions_cpu.py -- which checks on the float64 oracle alone
that they are well conditioned -- and the GPU files.  The oracle is tests/mlp_oracle.py's, whose functions are general
in the action count; the inputs are built here, because with 25..32 ids an output layer drawn from +-1/sqrt(fan_in)
can put probabilities below 1e-3: w2 and b2 are scaled by OUT_SCALE = 0.8.  (The GRU head's tests use 0.15; here
that draws the 17..32 probabilities so close together that the top two lie within the 1e-5 tie mask in 1..2 % of the
cells, over the 1 % cap; at 0.8 the smallest probability of any set is 8e-3 and the largest tie share 0.8 %.)
Everything else is mlp_oracle's (make_params, make_obs, mix_fractions) with seeds of this file."""
import functools

import numpy as np
import torch

import mlp_oracle as O

KIND = "chsel"
OUT_SCALE = 0.8
# (kind, F, H, A): the smallest shapes at which each path can go wrong
SHAPES = [
    (KIND, 24, 64, 17),      # xp_gamma.py's env (16 channels); one id in tile 1
    (KIND, 24, 128, 17),     # the learners' default hidden size
    (KIND, 31, 128, 32),     # F + 1 = 32; a full second tile
    (KIND, 32, 65, 25),      # F + 1 = 33; a lane group with one id; one row of hidden tile 5
    (KIND, 47, 64, 29),
    (KIND, 12, 16, 20),      # one hidden tile
    (KIND, 39, 100, 24),     # ragged hidden
    (KIND, 63, 128, 32),     # the envelope's corner
    (KIND, 1, 1, 17),        # the smallest of everything
]
SID = lambda s: f"F{s[1]}-H{s[2]}-A{s[3]}"  # noqa: E731
IDS = [SID(s) for s in SHAPES]
HET = {(KIND, 24, 64, 17): [24, 20, 24, 17, 24], (KIND, 24, 128, 17): [24, 20, 24, 17, 24],
       (KIND, 63, 128, 32): [63, 31, 32, 63, 40]}
E_EDGES = [1, 15, 16, 17, 31, 32, 33, 129]
E_MAX = 129
TILE1_SHAPES = [(KIND, 24, 64, 17), (KIND, 31, 128, 32)]      # A = 17 and A = 32: the sampler draws every id of tile 1


def batches(shape):
    """(N, E, in_dims) of a shape's policy runs: the E edges are slices of the first"""
    out = [(5, E_MAX, None), (1, E_MAX, None), (8, E_MAX, None)]
    if shape in HET:
        out.append((5, E_MAX, HET[shape]))
    return out


def _scaled(actor):
    actor["w2"] *= OUT_SCALE
    actor["b2"] *= OUT_SCALE
    return actor


def case_inputs(shape, N, E, dims, frac):
    """(actor, critic, obs) of one policy run"""
    kind, F, H, A = shape
    s = O.shape_seed(*shape) * 64 + N * 2 + (1 if dims else 0) + 500009
    actor, critic = O.make_params(N, F, H, A, s, dims)
    return _scaled(actor), critic, O.make_obs(E, N, F, dims, s + 7 + (100 if frac else 0), frac)


class PolicyRef:
    """Inputs and float64 / CPU-float32 references of one (shape, N, E, in_dims, frac) policy run, with the
    attributes of tests/test_policy_edges_gpu.py's Ref; rows(lo, hi) is the same for envs [lo, hi)."""
    PER_ENV = ("p64", "p32", "v64", "v32", "forced", "det", "det_tie", "smp", "smp_tie")

    def __init__(self, shape, N, E, dims, frac, parts=None):
        self.shape, self.N, self.E, self.dims, self.frac = shape, N, E, dims, frac
        kind, F, H, A = shape
        self.full = parts is None
        if parts is not None:
            self.__dict__.update(parts)
            return
        self.actor, self.critic, self.obs = case_inputs(shape, N, E, dims, frac)
        self.p64, self.p32 = O.probs(self.actor, self.obs), O.probs(self.actor, self.obs, torch.float32)
        self.v64, self.v32 = O.values(self.critic, self.obs), O.values(self.critic, self.obs, torch.float32)
        g = torch.Generator().manual_seed(O.shape_seed(*shape) + 3)
        self.forced = torch.randint(0, A, (N, E), generator=g)
        self.forced.view(-1)[:A] = torch.arange(A)                      # every id is forced at least once
        self.det, self.det_tie = O.deterministic_actions(self.p64, kind)
        self.smp, self.smp_tie = O.sampled_actions(self.p64, kind, O.RNG["env_base"] + np.arange(E), np.arange(N),
                                                   O.RNG["rng_step"], O.RNG["seed"])

    def rows(self, lo, hi):
        parts = {n: getattr(self, n)[:, lo:hi] for n in self.PER_ENV}
        parts.update(actor=self.actor, critic=self.critic, obs=self.obs[lo:hi])
        return PolicyRef(self.shape, self.N, hi - lo, self.dims, self.frac, parts)


@functools.lru_cache(maxsize=None)
def policy_ref(shape, N, E, dims, frac):
    return PolicyRef(shape, N, E, None if dims is None else list(dims), frac)


# ---- the update kernel's input sets
SWEEP = dict(N=5, T=3, E=45)
EDGE_SHAPES = [(KIND, 24, 64, 17), (KIND, 63, 128, 32)]
EDGE_N = [1, 5]
TILE_N = 256
TILE_CASE = ((KIND, 24, 64, 17), 25, 70, "mixed")      # 125 16-sample tiles per agent over the 4 waves of G = 1


def sweep_dims(shape):
    return HET.get(shape, O.upd_dims(shape[1]))


def update_inputs(shape, N, T, E, dims=None, mode="int"):
    """mlp_oracle.update_inputs for this head: the actor's output layer scaled by OUT_SCALE, ids int64 [N][B] that use
    every id where the set has A samples (the first A cells of agent-major order hold 0 .. A - 1: ids 16 and A - 1
    included), logp_old = the float64 log-prob + U(-0.3, 0.3) kept 1e-3 clear of the clip edges, W normal with one in
    ten exactly 0, R normal around 1."""
    kind, F, H, A = shape
    B = T * E
    s = (O.shape_seed(*shape) * 64 + N * 2 + (1 if dims else 0)) * 1009 + T * 131 + E + 700001
    actor, critic = O.make_params(N, F, H, A, s, dims)
    _scaled(actor)
    obs = O.make_obs(B, N, F, dims, s + 7 + (100 if mode == "frac" else 0), mode == "frac").view(T, E, N, F)
    if mode == "mixed":
        obs = O.mix_fractions(obs, dims, s + 11)
    g = torch.Generator().manual_seed(s + 13)
    acts = torch.randint(0, A, (N, B), generator=g)
    if N * B >= A:
        acts.view(-1)[:A] = torch.arange(A)
    lp = O.logp(O.probs(actor, obs.view(B, N, F)), kind, acts)
    d = torch.rand((N, B), generator=g, dtype=torch.float64) * 0.6 - 0.3
    for edge in O.CLIP_EDGES:
        d = torch.where((torch.exp(-d) - edge).abs() < 1e-3, d + 4e-3, d)
    logp_old = (lp + d).float()
    W = torch.randn((N, B), generator=g)
    W[torch.rand((N, B), generator=g) < 0.1] = 0.0
    R = 1.0 + torch.randn((N, B), generator=g)
    return dict(shape=shape, N=N, T=T, E=E, dims=dims, mode=mode, actor=actor, critic=critic, obs=obs, acts=acts,
                logp_old=logp_old, W=W, R=R)


def update_input_sets():
    """(label, update_inputs arguments) of every input set tests/test_mlp_actions_update_gpu.py runs"""
    out = []
    for shape in SHAPES:
        for mode in ("int", "frac"):
            out.append((f"sweep {SID(shape)} {mode}", dict(shape=shape, dims=sweep_dims(shape), mode=mode, **SWEEP)))
    for shape in EDGE_SHAPES:
        for N in EDGE_N:
            for T, E in O.UPD_TE:
                out.append((f"edge {SID(shape)} N{N} T{T} E{E}", dict(shape=shape, N=N, T=T, E=E)))
    shape, T, E, mode = TILE_CASE
    out.append((f"tiles {SID(shape)} T{T} E{E} {mode}", dict(shape=shape, N=TILE_N, T=T, E=E, mode=mode)))
    return out


def actions_blocks(N, n_tiles):
    """The gradient kernel's grid rule restated (csrc/mlp_actions_kernels.hip actions_blocks): G workgroups of 4 waves
    per agent; wave w of an agent's 4 G takes the 16-sample tiles w, w + 4 G, ..."""
    G = min((n_tiles + 3) // 4, max(1, 256 // max(1, N)))
    G = max(G, (n_tiles + 1023) // 1024)
    return max(1, min(G, 65535))


def workspace_floats(N, T, E, F, H, A):
    """d2d_ppo_actions_workspace restated: one partial of P floats per (wave, agent); 0 without a sample"""
    if N <= 0 or T <= 0 or E <= 0:
        return 0
    return 4 * actions_blocks(N, T * ((E + 15) // 16)) * N * (H * F + H + A * H + A + 2)
