"""TEST INFRASTRUCTURE ONLY.  The input sets of the iRDQN kernels' edge tests (csrc/rdqn_kernels.hip and the helpers
it takes from csrc/gru_l2_common.h) and one cached reference per set: tests/test_irdqn_edges_cpu.py asserts on the CPU
the conditions that let tests/test_irdqn_edges_gpu.py hold every block of every gradient to one strict tolerance, as
tests/gru_wide_cases.py / tests/test_gru_wide_cpu.py do for the wide GRU kernels.

A set is a Case tuple.  The base set has N = 2 agents, E = 3 envs, B = 17 samples (a full 16-sample tile and a tile of
one), L = 3, a plain ring of L + 4 rows with some windows wrapping it, F = 30, H = 50, A = 8; one size varies at a time.
Parameters are test_irdqn_gpu.make_params' (torch's init ranges, the GRU's doubled, agent k using the first F - 2k
inputs), the ring is test_irdqn_gpu.make_ring's (integers in [-1, 3] + U[0, 0.3), unused columns zero) times `scale`.
Each set has two sample lists: `samples`, B windows of exactly L steps for the TD update, and `qsamples`, B windows of
lengths 1, 2 and L mixed inside one tile for the Q kernel.  References are float64 and float32 torch of
irdqn_oracle.net_q and autograd of the TD loss through it, each computed once and left unchanged."""
import collections
import contextlib

import numpy as np
import torch

from gru_oracle import GRAD_ATOL, GRAD_RTOL, TIE, U32  # noqa: F401  (the tolerances of every edges suite)
from irdqn_oracle import net_q
from test_irdqn_gpu import make_params, make_ring

NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w1", "b1", "w2", "b2", "w3", "b3")
LOSSES = ("huber", "mse")
GAMMA = 0.4
EP, N_EP = 6, 3              # the episode ring: ring_episode = 6, three episodes (21 rows, 18 transitions)


@contextlib.contextmanager
def one_thread():
    """The references are thousands of tiny matrix products (a 256-step window of [17][50] states): a thread pool only
    adds its hand-over to each, a hundredfold here.  Scoped, so that no other test's setting changes."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


Case = collections.namedtuple("Case", "F H A N E B L ep scale bump")


def cid(c):
    return f"F{c.F}-H{c.H}-A{c.A}-N{c.N}-E{c.E}-B{c.B}-L{c.L}" + ("-ep" if c.ep else "") + \
        ("" if c.scale == 1 else f"-x{c.scale}")


# cid -> the first seed bump that meets the conditions of test_irdqn_edges_cpu.py::test_input_set_conditions (sets
# not listed: bump 0).  Found by running those conditions over bumps 0, 1, 2, ... on the CPU (`first_bump` below).
BUMP = {
    'F15-H128-A8-N2-E3-B17-L3': 3,
    'F33-H50-A8-N2-E3-B17-L3': 1,
    'F47-H128-A8-N2-E3-B17-L3': 3,
    'F48-H50-A8-N2-E3-B17-L3': 1,
}


def case(F=30, H=50, A=8, N=2, E=3, B=17, L=3, ep=0, scale=1):
    c = Case(F, H, A, N, E, B, L, ep, scale, 0)
    return c._replace(bump=BUMP.get(cid(c), 0))


def tiles(c):
    """(HT, IT): the kernels' run-time hidden and input tile counts"""
    return (c.H + 15) // 16, (c.F + 15) // 16


def rows_of_ring(c):
    return N_EP * (EP + 1) if c.ep else c.L + 4


BASE = case()
MATRIX_F = (15, 31, 47, 63)
# (1) the tile matrix: HT = 1 and 8 at IT = 1 .. 4; HT = 2 .. 7 with F rotating through the same four
MATRIX = [case(F=F, H=H) for H in (16, 128) for F in MATRIX_F] + \
         [case(F=MATRIX_F[i % 4], H=H) for i, H in enumerate((32, 48, 64, 80, 96, 112))]
# (2) ragged H at F = 30: last hidden tiles of 1, 2, 4, 10 and 15 units, vecH = 0 at narrow and wide HT
RAGGED_H = [case(H=H) for H in (1, 10, 17, 31, 33, 50, 63, 65, 100, 113, 127)]
# (3) ragged F at H = 50, and (16, 52), (17, 52): with the above all four (vecF, vecH) combinations
RAGGED_F = [case(F=F) for F in (1, 16, 17, 32, 33, 48, 49, 63)] + [case(F=16, H=52), case(F=17, H=52)]
# (4) ragged A: uint8 and int16 masks, bit 15, the rows of w3 past A in every lane group
RAGGED_A = [case(A=A) for A in (1, 2, 3, 5, 9, 15, 16)]
# (5) the batch: one ragged tile, 15 of 16, exactly one, three tiles with a ragged and with a full last one
BATCH = [case(B=B, N=1, E=1) for B in (1, 15, 16, 33, 48)]
# (6) windows: L = 1 (W_hh never enters), 2, and the long ones at B = 2 (the float64 reference's cost)
WINDOW = [case(L=L) for L in (1, 2)] + [case(L=L, B=2) for L in (64, 65, 256)]
# (7) a ring of whole episodes at a ragged H: windows across an episode boundary and across the wrap
EPISODE = [case(ep=EP)]
# (8) saturated gates: the ring times 40, the range the compact record's byte columns reach
SATURATED = [case(scale=40), case(H=100, scale=40)]
UNALIGNED = case(F=16, H=52)
INVALID = case(A=5)


def all_cases():
    seen, out = set(), []
    for c in [BASE] + MATRIX + RAGGED_H + RAGGED_F + RAGGED_A + BATCH + WINDOW + EPISODE + SATURATED:
        if cid(c) not in seen:
            seen.add(cid(c))
            out.append(c)
    return out


def case_seed(c):
    s = (((c.F * 67 + c.H) * 19 + c.A) * 131 + c.L * 7 + c.B) * 5 + c.N + 3 * c.E + (1009 if c.ep else 0) + 31 * c.scale
    return s + 7919 * c.bump


def blocks(c):
    """[(label, tensor name, index)]: the blocks of the agent-stacked gradient tensors that are held to their own
    scale -- each gate (r, z, n) of the four GRU tensors and the two hidden head layers, split into the rows of the last
    hidden tile ('last': units 16 (HT - 1) .. H - 1) and the rest; w3 and b3 whole."""
    H = c.H
    cut = 16 * (tiles(c)[0] - 1)
    parts = [("last", cut, H)] + ([("rest", 0, cut)] if cut else [])
    out = []
    for name in ("w_ih", "w_hh", "b_ih", "b_hh"):
        for G, gate in enumerate("rzn"):
            out += [(f"{name}.{gate}.{part}", name, (slice(None), slice(G * H + lo, G * H + hi)))
                    for part, lo, hi in parts]
    for name in ("w1", "b1", "w2", "b2"):
        out += [(f"{name}.{part}", name, (slice(None), slice(lo, hi))) for part, lo, hi in parts]
    return out + [("w3", "w3", (slice(None),)), ("b3", "b3", (slice(None),))]


def block_tol(g64_block):
    return GRAD_RTOL * g64_block.abs().max().item() + GRAD_ATOL


def ring_rows(c, last, S, shift=0):
    """the ring rows of the S-step window that ends at `last`, as csrc/rdqn_kernels.hip's ring_row states them"""
    rows = rows_of_ring(c)
    if c.ep:
        ntrans = rows // (c.ep + 1) * c.ep
        ms = [(last - S + 1 + j) % ntrans for j in range(S)]
        return [(m + m // c.ep + shift) % rows for m in ms]
    return [(last - S + 1 + j) % rows for j in range(S)]


def windows(c, ring, samples, shift=0):
    """{S: (sample indices, win [N][n][S][F])} of samples [(env, last, S)]"""
    out = {}
    for b, (e, last, S) in enumerate(samples):
        out.setdefault(S, ([], []))
        out[S][0].append(b)
        out[S][1].append(ring[ring_rows(c, last, S, shift), e])                 # [S][N][F]
    return {S: (idx, torch.stack(w).permute(2, 0, 1, 3)) for S, (idx, w) in out.items()}


def q_ref(c, p, ring, samples, dtype, shift=0):
    """Q [N][B][A] (double) of the samples' windows, evaluated at `dtype`"""
    q = {k: v.to(dtype) for k, v in p.items()}
    out = torch.zeros(c.N, len(samples), c.A, dtype=torch.float64)
    with torch.no_grad():
        for S, (idx, win) in windows(c, ring.to(dtype), samples, shift).items():
            out[:, idx] = net_q(q, win).double()
    return out


def td_ref(c, p, ring, samples, act, reward, done, qt, loss, dtype, weight=None):
    """autograd of the TD loss of DQN.train_step (mean over the B samples, summed over agents: each agent's gradient
    is its own): (grads, loss [N], delta [N][B]), all double.  weight [B][N] in {0, 1}: samples the kernel excludes
    (their coefficient is zero; the mean still divides by B)."""
    q = {k: v.to(dtype).clone().requires_grad_() for k, v in p.items()}
    (idx, win), = windows(c, ring.to(dtype), samples).values()                # one window length
    Q = net_q(q, win)                                                         # [N][B][A]
    qa = Q.gather(2, act.t().unsqueeze(-1)).squeeze(-1)                       # [N][B]
    td = reward.t().to(dtype) + (1 - done.to(dtype)).unsqueeze(0) * GAMMA * qt.to(dtype)
    if loss == "huber":
        per = torch.nn.functional.smooth_l1_loss(qa, td, reduction="none")
    else:
        per = (qa - td) ** 2
    if weight is not None:
        per = per * weight.t().to(dtype)
    ls = per.mean(1)
    ls.sum().backward()
    return ({k: (v.grad if v.grad is not None else torch.zeros_like(v)).double() for k, v in q.items()},
            ls.detach().double(), (qa - td).detach().double())


def head_pre(p64, h):
    """float64 pre-activations of the two relu layers and the rule's bound on their fp32 dot-product error:
    [(pre, 2 (H + 2) 2^-24 (|b| + sum |w| |v|))]"""
    H = p64["w1"].shape[1]
    out, v = [], h
    for w, b in (("w1", "b1"), ("w2", "b2")):
        pre = torch.baddbmm(p64[b].unsqueeze(1), v, p64[w].transpose(1, 2))
        ab = torch.baddbmm(p64[b].abs().unsqueeze(1), v.abs(), p64[w].abs().transpose(1, 2))
        out.append((pre, 2 * (H + 2) * U32 * ab))
        v = torch.relu(pre)
    return out


def gru_h(p, win):
    """the GRU's last hidden state [N][B][H] of windows [N][B][S][F] (net_q's recurrence)"""
    n, B, S, _ = win.shape
    H = p["w_hh"].shape[2]
    h = torch.zeros(n, B, H, dtype=win.dtype)
    for s in range(S):
        gi = torch.baddbmm(p["b_ih"].unsqueeze(1), win[:, :, s], p["w_ih"].transpose(1, 2))
        gh = torch.baddbmm(p["b_hh"].unsqueeze(1), h, p["w_hh"].transpose(1, 2))
        r = torch.sigmoid(gi[..., :H] + gh[..., :H])
        z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
        n_ = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
        h = (1 - z) * n_ + z * h
    return h


class Ref:
    """One input set and its references."""

    def __init__(self, c):
        self.c = c
        s = case_seed(c)
        self.rows = rows_of_ring(c)
        self.p, self.dims = make_params(c.F, c.H, c.A, s, n=c.N)
        self.ring = make_ring(self.rows, c.E, c.F, self.dims, s + 1) * float(c.scale)
        rng = np.random.default_rng(s + 2)
        span = self.rows // (c.ep + 1) * c.ep if c.ep else self.rows          # transitions / rows a window may end at
        lasts = [int(rng.integers(span)) for _ in range(c.B)]
        if c.ep:                       # inside an episode, across boundaries, the ring's last, wrapping to the end
            lasts[:6] = [4, 7, 9, 17, 2, 0]
        else:
            lasts[0] = 0               # wraps the ring for every L > 1
            if c.B > 1:
                lasts[1] = self.rows - 1
        self.samples = [(int(rng.integers(c.E)), lasts[b], c.L) for b in range(c.B)]
        lens = [(c.L, 1, 2)[b % 3] for b in range(c.B)]
        if c.B >= 3:
            rng.shuffle(lens)
        self.qsamples = [(int(rng.integers(c.E)), int(rng.integers(span)), int(S)) for S in lens]
        g = torch.Generator().manual_seed(s + 3)
        self.act = torch.randint(0, c.A, (c.B, c.N), generator=g)
        self.reward = torch.randn(c.B, c.N, generator=g) * 1.5                 # delta on both sides of +-1
        self.done = torch.arange(c.B) % 2 == 1
        self.qt = torch.randn(c.N, c.B, generator=g)
        self._q, self._td, self._amb = {}, {}, None

    def q(self, dtype=torch.float64, shift=0):
        key = (dtype, shift)
        if key not in self._q:
            with one_thread():
                self._q[key] = q_ref(self.c, self.p, self.ring, self.qsamples, dtype, shift)
        return self._q[key]

    def td(self, loss):
        """(g64, loss64 [N], delta64 [N][B], g32, loss32), all double"""
        if loss not in self._td:
            a = (self.c, self.p, self.ring, self.samples, self.act, self.reward, self.done, self.qt, loss)
            with one_thread():
                g64, l64, d64 = td_ref(*a, torch.float64)
                g32, l32, _ = td_ref(*a, torch.float32)
            self._td[loss] = (g64, l64, d64, g32, l32)
        return self._td[loss]

    def ambiguous(self):
        """(pairs of head layer 1, of head layer 2) of the update's windows whose pre-activation lies within the
        rule's bound of zero: any fp32 evaluation may take either relu mask there"""
        if self._amb is None:
            p64 = {k: v.double() for k, v in self.p.items()}
            (_, win), = windows(self.c, self.ring.double(), self.samples).values()
            with torch.no_grad(), one_thread():
                self._amb = tuple(int((pre.abs() <= bound).sum()) for pre, bound in head_pre(p64, gru_h(p64, win)))
        return self._amb

    def margin(self, shift=0):
        """[N][B]: the float64 distance of the greedy decision of every Q sample from a tie"""
        q = self.q(torch.float64, shift)
        if q.shape[-1] == 1:
            return torch.ones(q.shape[:-1], dtype=q.dtype)
        top = q.topk(2, -1).values
        return top[..., 0] - top[..., 1]

    def shifts(self):
        return (0, 1) if self.c.ep else (0,)


_REFS = {}


def ref(c):
    if cid(c) not in _REFS:
        _REFS[cid(c)] = Ref(c)
    return _REFS[cid(c)]


def conditions(c):
    """The conditions on the reference alone under which the GPU file needs one strict branch; returns torch fp32's
    largest share of a block's gradient tolerance (see test_irdqn_edges_cpu.py::test_input_set_conditions)."""
    r = ref(c)
    for k, d in enumerate(r.dims):
        assert bool((r.ring[:, :, k, d:] == 0).all()) and bool((r.p["w_ih"][k, :, d:] == 0).all())
    amb = r.ambiguous()
    assert amb == (0, 0), f"{amb} ambiguous head-relu pairs: take the next seed"
    for shift in r.shifts():
        assert bool(torch.isfinite(r.q(torch.float64, shift)).all())
        skipped = (r.margin(shift) <= TIE).double().mean().item()
        assert skipped <= 0.01, (shift, skipped)
    if c.B >= 2:
        assert bool(r.done.any()) and not bool(r.done.all())
    worst = 0.0
    for loss in LOSSES:
        g64, l64, d64, g32, l32 = r.td(loss)
        if c.B >= 16:
            assert bool((d64.abs() < 1).any()) and bool((d64.abs() > 1).any())
        for label, name, idx in blocks(c):
            tol = block_tol(g64[name][idx])
            band = (g32[name][idx] - g64[name][idx]).abs().max().item()
            worst = max(worst, band / tol)
            assert band <= tol, (loss, label, band, tol)
        if c.L == 1:
            assert bool((g64["w_hh"] == 0).all())
        for k, d in enumerate(r.dims):
            assert bool((g64["w_ih"][k, :, d:] == 0).all())
    return worst


def first_bump(c, limit=200):
    """the first seed bump at which `conditions` hold (how BUMP was made)"""
    for bump in range(limit):
        cc = c._replace(bump=bump)
        _REFS.pop(cid(cc), None)
        try:
            conditions(cc)
            return bump
        except AssertionError:
            continue
        finally:
            _REFS.pop(cid(cc), None)
    raise RuntimeError(f"no bump below {limit} for {cid(c)}")


def single(r, b):
    """sample b of the update alone (B = 1): (samples, act, reward, done, qmax_target)"""
    return [r.samples[b]], r.act[b:b + 1], r.reward[b:b + 1], r.done[b:b + 1], r.qt[:, b:b + 1].contiguous()


SINGLES = (0, 5, 16)         # samples of the base set launched alone: the ring's wrap, done set, the tile of one


def invalid_actions(r):
    """The INVALID set (A = 5) with action masks the kernel excludes or reduces: (masks int64 [B][N], the action index
    autograd gathers [B][N], weight [B][N] in {0, 1}).  Excluded: mask 0, and a lone bit at or above A (bits 6 and 7).
    Reduced to its lowest bit: two bits below A, and a bit below A with bit 6."""
    assert r.c.A == 5 and r.c.B == 17
    act = r.act.clone()
    masks = torch.ones_like(act) << act
    weight = torch.ones(act.shape, dtype=torch.float64)
    masks[1], weight[1] = 0, 0
    masks[3], weight[3] = 1 << 6, 0
    masks[5], act[5] = (1 << 1) | (1 << 3), 1
    masks[7], act[7] = (1 << 2) | (1 << 6), 2
    masks[16, 1], weight[16, 1] = 1 << 7, 0                                   # the tile of one: agent 1 only
    act[weight == 0] = 0
    return masks, act, weight
