"""TEST INFRASTRUCTURE ONLY.  The plain-torch oracle of the GRU window kernels (csrc/gru_kernels.hip) and the input
sets of tests/test_gru_edges_gpu.py: the reference's RNN module over every slot's window (gru_ref), autograd of its
PPO / MSE losses (ref_loss_grads), networks and observations, a guarded device allocator and the ambiguous-relu
counter.  Everything but `guarded` (and mlp_oracle.to_record) runs on the CPU at the dtype the caller names;
tests/test_gru_oracle_cpu.py pins algorithms._core.gru_window to torch.nn.GRU and asserts, for every input set of
the GPU file, the conditions that let its tests hold every sample to the strict tolerance.

Layouts are the kernels': parameters agent-stacked (StackedNets kind "rnn"), obs [T][E][N][F], outputs [N][T][E](A),
per-sample inputs [N][T][E] here and [T][E][N] (or [N][E*T]) on the device."""
import collections
import math

import torch

U32 = 2.0 ** -24            # float32's unit roundoff
P_LO = 1e-3                 # every action probability of every input set lies in [P_LO, 1 - P_LO]
TIE = 1e-5                  # margin below which a deterministic action may fall either way
GRAD_RTOL, GRAD_ATOL = 2e-5, 1e-7   # |g - g64| <= GRAD_RTOL * max|g64| + GRAD_ATOL (tests/test_gru_gpu.py)
CLIP_EDGES = (0.8, 0.9, 1.1, 1.2)   # 1 -+ clip of the clips the GPU tests use (0.1, 0.2)
NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w1", "b1", "w2", "b2")


# ---------------------------------------------------------------------------------------------------
# moved from tests/test_gru_gpu.py (which imports them)

def make_obs(T, E, N, F, dims, seed, frac=False):
    g = torch.Generator().manual_seed(seed)
    obs = torch.zeros(T, E, N, F)
    D = max(1, F // 3)
    obs[..., :D] = torch.randint(0, 4, (T, E, N, D), generator=g).float()
    obs[..., D:] = torch.randint(-1, 2, (T, E, N, F - D), generator=g).float()
    if frac:
        obs += torch.rand(obs.shape, generator=g) * 0.3
    for k, d in enumerate(dims):
        obs[:, :, k, d:] = 0
    return obs


def gru_ref(p, obs, ep_len, L, padded, kind, dtype=torch.float64):
    """torch reference: outputs [N][T][E][A] (probs, or values [N][T][E]) of every slot's window."""
    from algorithms._core import gru_window
    T, E, N, F = obs.shape
    q = {k: v.to(dtype) for k, v in p.items()}
    outs = []
    for t in range(T):
        S = min(t % ep_len + 1, L)
        win = obs[t - S + 1: t + 1].to(dtype).permute(2, 1, 0, 3)                # [N][E][S][F]
        if padded and S < L:
            win = torch.cat([torch.zeros(N, E, L - S, F, dtype=dtype), win], 2)
        h = gru_window(win, q["w_ih"], q["w_hh"], q["b_ih"], q["b_hh"])          # [N][E][H]
        y = torch.relu(torch.baddbmm(q["b1"].unsqueeze(1), h, q["w1"].transpose(1, 2)))
        z = torch.baddbmm(q["b2"].unsqueeze(1), y, q["w2"].transpose(1, 2))        # [N][E][A]
        outs.append(torch.sigmoid(z) if kind == "sigmoid" else torch.softmax(z, -1) if kind == "softmax" else z[..., 0])
    return torch.stack(outs, 1)


def ref_loss_grads(p, obs, ep, L, kind, acts, logp_old, W, clip, beta, dtype):
    """autograd of the per-agent losses summed over agents (each agent's gradient is its own)."""
    from torch.distributions import Bernoulli, Categorical
    q = {k: v.to(dtype).clone().requires_grad_() for k, v in p.items()}
    out = gru_ref(q, obs, ep, L, True, kind, dtype)                            # [N][T][E](A)
    N = out.shape[0]
    if kind is None:
        loss = ((out - W.to(dtype)) ** 2).reshape(N, -1).mean(1)
        sq = ((out - W.to(dtype)) ** 2).reshape(N, -1).sum(1)
        stats = torch.stack([sq, torch.zeros_like(sq)], 1)
    else:
        if kind == "sigmoid":
            d = Bernoulli(probs=out, validate_args=False)
            logp = d.log_prob(acts.to(dtype)).mean(-1)
            ent = d.entropy().mean(-1)
        else:
            d = Categorical(probs=out, validate_args=False)
            logp = d.log_prob(acts)
            ent = d.entropy()
        ratio = torch.exp(logp - logp_old.to(dtype))
        Wd = W.to(dtype)
        s = torch.min(ratio * Wd, torch.clamp(ratio, 1 - clip, 1 + clip) * Wd)
        loss = -s.reshape(N, -1).mean(1) - beta * ent.reshape(N, -1).mean(1)
        stats = torch.stack([s.reshape(N, -1).sum(1), ent.reshape(N, -1).sum(1)], 1)
    loss.sum().backward()
    # (history_len 1: h0 = 0 is the window's only hidden input, so W_hh never enters the graph -- its gradient
    # is exactly zero)
    return ({k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in q.items()}, stats.detach(),
            out.detach())


def window_groups(obs, ep, L, padded):
    """The windows of every slot, grouped by length: [(slots, x [N][len(slots) * E][S][F])].  Training
    windows are front-zero-padded to L (one group, ippo.py:390-403); rollout windows hold the last
    S = min(p + 1, L) obs of the episode (ippo.py:302-304), one group per S."""
    T, E, N, F = obs.shape
    pos = torch.arange(T) % ep
    S_of = torch.clamp(pos + 1, max=L)
    groups = []
    for S in ([L] if padded else sorted(set(S_of.tolist()))):
        slots = torch.arange(T) if padded else torch.nonzero(S_of == S)[:, 0]
        xs = []
        for t in slots.tolist():
            s = min(int(pos[t]) + 1, L)
            w = obs[t - s + 1: t + 1]                                                 # [s][E][N][F]
            if s < S:
                w = torch.cat([torch.zeros(S - s, E, N, F, dtype=obs.dtype, device=obs.device), w], 0)
            xs.append(w)
        x = torch.stack(xs, 0).permute(3, 0, 2, 1, 4).reshape(N, len(xs) * E, S, F)   # [N][slots*E][S][F]
        groups.append((slots, x))
    return groups


def head(q, h, kind, flip=None):
    """The RNN head; flip (bool [N][B][H]) inverts the relu mask of those (sample, unit) pairs (their
    pre-activations are within fp32 rounding of 0, so y ~ 0 either way and only the gradient's mask changes)."""
    pre = torch.baddbmm(q["b1"].unsqueeze(1), h, q["w1"].transpose(1, 2))
    y = torch.relu(pre) if flip is None else pre * ((pre > 0) ^ flip).to(pre.dtype)
    z = torch.baddbmm(q["b2"].unsqueeze(1), y, q["w2"].transpose(1, 2))
    return torch.sigmoid(z) if kind == "sigmoid" else torch.softmax(z, -1) if kind == "softmax" else z[..., 0]


# ---------------------------------------------------------------------------------------------------
# networks, observations, guards, the ambiguous-relu rule

OUT_SCALE = 0.3


def make_net(N, F, H, A, seed, in_dims=None, out_scale=OUT_SCALE):
    """Agent-stacked RNN params (float32, CPU) of per-agent input widths in_dims (columns past them zero).  torch's
    default GRU init (uniform +-1/sqrt(H)) doubled, so that the gates leave their linear regime (as
    tests/test_gru_gpu.py's make_net), and the output layer (w2, b2) scaled by out_scale: with the init as it is some
    sets' softmax probabilities fall to 5e-9, where torch's float32 epsilon clamp takes float32 autograd 1.8e4 x the
    gradient tolerance away from float64 and no float32 kernel could be held to it."""
    from algorithms._core import RNN, StackedNets
    torch.manual_seed(seed)
    dims = list(in_dims) if in_dims else [F] * N
    assert len(dims) == N and max(dims) == F
    st = StackedNets([RNN(d, A, H) for d in dims], dims, "rnn", "cpu")
    p = {k: v.detach().clone() for k, v in st.params.items()}
    p["w_ih"] *= 2.0
    p["w_hh"] *= 2.0
    p["w2"] *= out_scale
    p["b2"] *= out_scale
    for k, d in enumerate(dims):
        assert bool((p["w_ih"][k, :, d:] == 0).all())
    return p, dims


FRAC_MODES = ("none", "all", "one", "column")
THIRD = 1.0 / 3.0           # float32(1/3) = 0x3EAAAAAB: 24 significant bits, three nonzero bf16 parts


def frac_obs(T, E, N, F, dims, seed, frac="none"):
    """make_obs's env-like integers (all bf16-exact), then by `frac`:
    all     every used column + U[0, 0.3);
    one     exactly one element of the whole batch is fractional (1/3): the last agent's column 0 of the last real
            sample of the last 16-env tile in the second-to-last slot -- one step of one tile takes the inexact branch;
    column  column min(dims) // 2 holds 1/3 in every sample of every agent (the categorical env's 1/n ACK fraction,
            whose bf16 truncation error is the same in every sample and adds up coherently in dW_ih)."""
    assert frac in FRAC_MODES
    obs = make_obs(T, E, N, F, dims, seed, frac == "all")
    if frac == "one":
        obs[T - 2, E - 1, N - 1, 0] = THIRD
    elif frac == "column":
        obs[..., min(dims) // 2] = THIRD
    return obs


def bf16_exact(x):
    """bool: float32 values whose low 16 bits are zero"""
    return (x.contiguous().view(torch.int32) & 0xFFFF) == 0


GUARD_BYTES = 256


def guarded(src=None, shape=None, dtype=None, device="cuda"):
    """A tensor of `shape` / `dtype` (or a copy of `src`) placed at a 16-byte aligned offset inside a larger device
    buffer filled with 0xFF bytes (NaN as float32, -1 / 255 as integers), GUARD_BYTES on each side.  Returns
    (view, check): check() asserts that every guard byte still holds 0xFF.  Without src the inside is 0xFF too, so an
    output the launch did not write reads as NaN."""
    if src is not None:
        shape, dtype = tuple(src.shape), src.dtype
    n = int(math.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    tail = GUARD_BYTES + (-n) % 16
    buf = torch.full((GUARD_BYTES + n + tail,), 0xFF, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(shape)
    if src is not None:
        view.copy_(src)

    def check(what=""):
        assert bool((buf[:GUARD_BYTES] == 0xFF).all()), f"{what}: written before the tensor"
        assert bool((buf[GUARD_BYTES + n:] == 0xFF).all()), f"{what}: written past the tensor"
    return view, check


def ambiguous_relu_pairs(p, obs, ep, L, padded, H=None):
    """Number of (sample, head unit) pairs whose first-layer pre-activation is within twice the fp32 dot-product
    error bound of 0 -- |pre| <= 2 (H + 2) 2^-24 (|b1| + sum |w1| |h|), the rule of tests/test_gru_gpu.py's
    xp_grads_check -- over every slot's window, float64.  Any fp32 evaluation may take either relu mask there."""
    from algorithms._core import gru_window
    q = {k: v.double() for k, v in p.items()}
    H = H or q["w1"].shape[1]
    n = 0
    for _, x in window_groups(obs.double(), ep, L, padded):
        hL = gru_window(x, q["w_ih"], q["w_hh"], q["b_ih"], q["b_hh"])
        pre = torch.baddbmm(q["b1"].unsqueeze(1), hL, q["w1"].transpose(1, 2))
        ab = torch.baddbmm(q["b1"].abs().unsqueeze(1), hL.abs(), q["w1"].abs().transpose(1, 2))
        n += int((pre.abs() <= 2 * (H + 2) * U32 * ab).sum())
    return n


def strides_address_same(t, ref_tEN):
    """Whether the stride triple d2dhip.gru._strides3 derives for t addresses, for every (slot, env, agent), the
    element ref_tEN [T][E][N] holds there."""
    from d2dhip.gru import _strides3
    T, E, N = ref_tEN.shape
    s0, s1, s2 = _strides3(t, T, E, N)
    flat = torch.as_strided(t, (T, E, N), (s0, s1, s2), t.storage_offset())
    return torch.equal(flat, ref_tEN)


# ---------------------------------------------------------------------------------------------------
# the input sets of tests/test_gru_edges_gpu.py

Case = collections.namedtuple("Case", "kind F H A L ep T E N dims frac bump")
A_OF = {"sigmoid": 8, "softmax": 5, None: 1}


def case(kind, F, H, A=None, L=3, ep=5, T=None, E=17, N=2, dims=None, frac="none"):
    A = A_OF[kind] if A is None else A
    c = Case(kind, F, H, A, L, ep, 2 * ep if T is None else T, E, N, None if dims is None else tuple(dims), frac, 0)
    return c._replace(bump=SEED_BUMP.get(cid(c), 0))


def cid(c):
    s = f"{c.kind or 'value'}-F{c.F}-H{c.H}-A{c.A}-L{c.L}-ep{c.ep}-T{c.T}-E{c.E}-N{c.N}"
    if c.dims:
        s += "-d" + "_".join(str(d) for d in c.dims)
    return s + ("" if c.frac == "none" else "-" + c.frac)


# sets whose first seed left an ambiguous head-relu pair (or a clip edge within fp32 rounding): the next seed
SEED_BUMP = {
    'sigmoid-F1-H50-A8-L3-ep5-T10-E17-N2': 1,
    'sigmoid-F12-H50-A8-L3-ep5-T10-E17-N2-all': 1,
    'sigmoid-F12-H50-A8-L3-ep5-T10-E17-N2-column': 1,
    'sigmoid-F15-H64-A8-L3-ep5-T10-E17-N2': 3,
    'sigmoid-F30-H32-A8-L3-ep5-T10-E17-N2-column': 2,
    'sigmoid-F30-H33-A8-L3-ep5-T10-E17-N2': 1,
    'sigmoid-F30-H48-A8-L3-ep5-T10-E17-N2': 5,
    'sigmoid-F30-H50-A1-L3-ep5-T10-E17-N2': 2,
    'sigmoid-F30-H50-A2-L3-ep5-T10-E17-N2': 3,
    'sigmoid-F30-H50-A8-L3-ep5-T10-E17-N2-one': 1,
    'sigmoid-F30-H50-A8-L3-ep5-T5-E80-N2': 7,
    'sigmoid-F30-H50-A9-L3-ep5-T10-E17-N2': 2,
    'sigmoid-F30-H63-A8-L3-ep5-T10-E17-N2': 3,
    'sigmoid-F31-H16-A8-L3-ep5-T10-E17-N2': 1,
    'sigmoid-F31-H64-A8-L3-ep5-T10-E17-N2': 6,
    'sigmoid-F40-H32-A8-L3-ep5-T10-E17-N2-one': 1,
    'sigmoid-F40-H50-A8-L3-ep5-T10-E17-N2-all': 10,
    'sigmoid-F40-H50-A8-L3-ep5-T10-E17-N2-one': 1,
    'sigmoid-F47-H64-A8-L3-ep5-T10-E17-N2': 1,
    'sigmoid-F63-H50-A8-L3-ep5-T10-E17-N2-one': 5,
    'sigmoid-F63-H64-A8-L3-ep5-T10-E17-N2': 3,
    'softmax-F12-H32-A5-L3-ep5-T10-E17-N2-column': 1,
    'softmax-F12-H50-A5-L3-ep5-T10-E17-N2': 3,
    'softmax-F12-H50-A5-L3-ep5-T10-E17-N2-column': 2,
    'softmax-F15-H64-A5-L3-ep5-T10-E17-N2': 2,
    'softmax-F16-H50-A5-L3-ep5-T10-E17-N2': 3,
    'softmax-F30-H10-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F30-H48-A5-L3-ep5-T10-E17-N2': 3,
    'softmax-F30-H50-A2-L3-ep5-T10-E17-N2': 1,
    'softmax-F30-H50-A5-L3-ep5-T10-E15-N2': 2,
    'softmax-F30-H50-A5-L3-ep5-T10-E17-N1': 1,
    'softmax-F30-H50-A5-L3-ep5-T10-E17-N2': 2,
    'softmax-F30-H50-A5-L3-ep5-T10-E17-N2-column': 1,
    'softmax-F30-H50-A5-L3-ep5-T10-E17-N2-one': 1,
    'softmax-F30-H50-A5-L64-ep6-T6-E3-N2': 1,
    'softmax-F31-H64-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F40-H32-A5-L3-ep5-T10-E17-N2-all': 2,
    'softmax-F47-H32-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F47-H64-A5-L3-ep5-T10-E17-N2': 2,
    'softmax-F48-H50-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F63-H16-A5-L3-ep5-T10-E17-N2': 1,
    'softmax-F63-H16-A5-L3-ep5-T10-E17-N2-column': 1,
    'softmax-F63-H32-A5-L3-ep5-T10-E17-N2': 2,
    'softmax-F63-H50-A5-L3-ep5-T10-E17-N2-all': 1,
    'softmax-F63-H50-A5-L3-ep5-T10-E17-N2-column': 4,
    'softmax-F63-H64-A5-L3-ep5-T10-E17-N2': 3,
    'value-F12-H50-A1-L3-ep5-T10-E17-N2': 1,
    'value-F12-H50-A1-L3-ep5-T10-E17-N2-column': 4,
    'value-F12-H50-A1-L3-ep5-T10-E17-N2-one': 1,
    'value-F15-H64-A1-L3-ep5-T10-E17-N2': 2,
    'value-F30-H48-A1-L3-ep5-T10-E17-N2': 1,
    'value-F30-H50-A1-L1-ep5-T10-E17-N2': 1,
    'value-F30-H50-A1-L129-ep6-T6-E3-N2': 1,
    'value-F30-H50-A1-L8-ep5-T10-E17-N2': 1,
    'value-F31-H32-A1-L3-ep5-T10-E17-N2': 1,
    'value-F31-H64-A1-L3-ep5-T10-E17-N2': 1,
    'value-F40-H32-A1-L3-ep5-T10-E17-N2-column': 2,
    'value-F40-H50-A1-L3-ep5-T10-E17-N2': 1,
    'value-F40-H50-A1-L3-ep5-T10-E17-N2-all': 2,
    'value-F40-H50-A1-L3-ep5-T10-E17-N2-one': 1,
    'value-F63-H16-A1-L3-ep5-T10-E17-N2-all': 1,
    'value-F63-H32-A1-L3-ep5-T10-E17-N2-all': 1,
}

KINDS = ("sigmoid", "softmax", None)
# the ragged base case: H = 50 (HT = 4, 50 of 64 rows), F = 30 (IT = 2), E = 17 (a second env tile of one env)

# (1) the instance matrix: (HT, IT) <- H in {16, 32, 64} x F + 1 in {16, 32, 48, 64}; the policy has no IT = 3
MATRIX_H, MATRIX_F = (16, 32, 64), (15, 31, 47, 63)
MATRIX = [case(k, F, H) for H in MATRIX_H for F in MATRIX_F for k in KINDS]
# (2) ragged sizes around the base case
# (H = 1 as a value network only: with the one head unit's relu off every probability is sigmoid(b2) / softmax(b2) of
# the constant-initialised b2 -- exact ties, which a deterministic comparison must skip)
RAGGED_H = [case((None, "sigmoid", "softmax")[i % 3], 30, H) for i, H in enumerate((1, 10, 17, 31, 33, 48, 50, 63))] + \
           [case("sigmoid", 30, 50), case("softmax", 30, 50), case("softmax", 30, 10), case(None, 30, 33),
            case("softmax", 30, 33), case("sigmoid", 30, 48), case(None, 30, 48)]
RAGGED_F = [case(KINDS[i % 3], F, 50) for i, F in enumerate((1, 16, 32, 47, 48))]
RAGGED_DIMS = [case("sigmoid", 30, 50, dims=(30, 22)), case("softmax", 48, 50, dims=(33, 48)),
               case(None, 16, 17, dims=(16, 9))]
RAGGED_A = [case("sigmoid", 30, 50, A=A) for A in (1, 2, 9, 16)] + [case("softmax", 30, 50, A=A) for A in (2, 16)]
RAGGED_E = [case(KINDS[i % 3], 30, 50, E=E) for i, E in enumerate((1, 15, 16, 33))] + \
           [case("sigmoid", 30, 50, E=15, N=1), case("softmax", 30, 50, E=17, N=1), case("sigmoid", 30, 50, E=80, T=5)]
RAGGED = RAGGED_H + RAGGED_F + RAGGED_DIMS + RAGGED_A + RAGGED_E
# (3) the input branches: an IT = 1 shape and an IT = 3 shape (the policy's IT = 4, fp32 MFMA only)
FRAC = [case(k, F, 50, frac=fr) for F in (12, 40) for k in KINDS for fr in FRAC_MODES]
# (the grad kernel alone has instances with HT = 4 and IT = 4 on fp32 rows; IT = 3 and 4 there shared a fault)
FRAC_WIDE = [case(k, 63, 50, frac=fr) for k in KINDS for fr in FRAC_MODES[1:]]
# Every instance that chooses between three and six W_ih part products by the per-step ballot runs its inexact side:
# HT = 1 and 2 at every IT, and (4, 2) -- the policy's split kernel at IT <= 2, the grad kernel at all four
FRAC_LOW = [case(k, F, H, frac=fr) for H in (16, 32) for F in (12, 30, 40, 63) for k in KINDS for fr in FRAC_MODES[1:]] + \
           [case(k, 30, 50, frac=fr) for k in KINDS for fr in FRAC_MODES[1:]]
# (4) window thresholds at ragged H: the 63-step padding table / the 64-step flush, a second flush, L > episode, L = 1
WINDOW_SHORT = [case(k, 30, 50, L=L, ep=6, T=6, E=3) for L in (64, 65, 129) for k in KINDS]
WINDOW_LONG = [case("sigmoid", 30, 50, L=129, ep=70, T=70, E=3), case(None, 23, 33, L=65, ep=70, T=70, E=3)]
WINDOW_MISC = [case("sigmoid", 30, 50, L=8), case("softmax", 30, 50, L=8), case(None, 30, 50, L=8),
               case("sigmoid", 30, 50, L=1), case("softmax", 30, 50, L=1), case(None, 30, 50, L=1)]
WINDOW = WINDOW_SHORT + WINDOW_LONG + WINDOW_MISC
BASE_CASES = [case(k, 30, 50) for k in KINDS]


def all_cases():
    seen, out = set(), []
    for c in MATRIX + RAGGED + FRAC + FRAC_WIDE + FRAC_LOW + WINDOW + BASE_CASES:
        if cid(c) not in seen:
            seen.add(cid(c))
            out.append(c)
    return out


def case_seed(c):
    s = ((c.F * 67 + c.H) * 19 + c.A) * 131 + c.L * 7 + c.E * 3 + c.N + FRAC_MODES.index(c.frac) * 100003
    return s + {"sigmoid": 0, "softmax": 1000003, None: 2000003}[c.kind] + (17 if c.dims else 0) + 7919 * c.bump


class Ref:
    """One input set and its references, each computed once and left unchanged: the network, the obs, the float64 /
    float32 outputs of every slot's window, the forced actions, the update's per-sample inputs, and autograd's
    gradients and loss sums."""

    def __init__(self, c):
        self.c = c
        s = case_seed(c)
        self.p, self.dims = make_net(c.N, c.F, c.H, c.A, s, c.dims)
        self.obs = frac_obs(c.T, c.E, c.N, c.F, self.dims, s + 7, c.frac)
        self._out, self._train, self._grads, self._amb = {}, None, {}, {}

    def out(self, padded, dtype=torch.float64):
        """[N][T][E](A): probabilities / values of every slot's window"""
        key = (bool(padded), dtype)
        if key not in self._out:
            c = self.c
            with torch.no_grad():
                o = gru_ref(self.p, self.obs, c.ep, c.L, padded, c.kind, dtype)
            self._out[key] = o.double()
        return self._out[key]

    def ambiguous(self, padded):
        if padded not in self._amb:
            c = self.c
            self._amb[padded] = ambiguous_relu_pairs(self.p, self.obs, c.ep, c.L, padded)
        return self._amb[padded]

    def actions(self):
        """the forced actions: bits double [N][T][E][A] (Bernoulli, p = 0.4) / ids int64 [N][T][E]"""
        return self.train()[0]

    def train(self):
        """(acts, logp_old [N][T][E] float32, W [N][T][E] float32).  logp_old = the float64 log-prob of the padded
        window + U(-0.3, 0.3): ratios on both sides of and inside a clip of 0.1 / 0.2, none within 1e-3 of an edge
        (the surrogate's gradient jumps there)."""
        if self._train is None:
            c = self.c
            g = torch.Generator().manual_seed(case_seed(c) + 13)
            shape = (c.N, c.T, c.E)
            if c.kind is None:
                self._train = (None, None, torch.randn(shape, generator=g))
            else:
                out = self.out(True)
                if c.kind == "sigmoid":
                    acts = (torch.rand(shape + (c.A,), generator=g) < 0.4).double()
                else:
                    acts = torch.randint(0, c.A, shape, generator=g)
                lp = self.logp(out, acts)
                d = torch.rand(shape, generator=g, dtype=torch.float64) * 0.6 - 0.3
                for edge in CLIP_EDGES:
                    d = torch.where((torch.exp(-d) - edge).abs() < 1e-3, d + 4e-3, d)
                self._train = (acts, (lp + d).float(), torch.randn(shape, generator=g))
        return self._train

    def logp(self, probs, acts):
        from torch.distributions import Bernoulli, Categorical
        if self.c.kind == "sigmoid":
            return Bernoulli(probs=probs, validate_args=False).log_prob(acts.to(probs.dtype)).mean(-1)
        return Categorical(probs=probs, validate_args=False).log_prob(acts)

    def grads(self, clip=0.1, beta=0.05):
        """(float64 grads, float64 stats [N][2], float32 grads, float32 stats) of the mean losses"""
        key = (clip, beta)
        if key not in self._grads:
            c = self.c
            acts, lo, W = self.train()
            r64, s64, _ = ref_loss_grads(self.p, self.obs, c.ep, c.L, c.kind, acts, lo, W, clip, beta, torch.float64)
            r32, s32, _ = ref_loss_grads(self.p, self.obs, c.ep, c.L, c.kind, acts, lo, W, clip, beta, torch.float32)
            self._grads[key] = (r64, s64, {k: v.double() for k, v in r32.items()}, s32.double())
        return self._grads[key]

    def margin(self, padded):
        """[N][T][E]: distance of the deterministic decision from a tie"""
        o = self.out(padded)
        if self.c.kind == "sigmoid":
            return (o - 0.5).abs().min(-1).values
        if o.shape[-1] == 1:
            return torch.ones(o.shape[:-1], dtype=o.dtype)
        top = o.topk(2, -1).values
        return top[..., 0] - top[..., 1]


_REFS = {}


def ref(c):
    if cid(c) not in _REFS:
        _REFS[cid(c)] = Ref(c)
    return _REFS[cid(c)]
