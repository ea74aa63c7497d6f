"""Float64 oracle of d2d_adam_step (csrc/optim_kernels.hip) in plain torch ops, the tensor sets the optimizer tests
run, and the error bars a step is held to.

clip_adam64 is torch.nn.utils.clip_grad_norm_ per agent followed by torch.optim.Adam at its defaults, written out:
    norm_k = sqrt(sum g^2) over agent k's tensors, coef_k = min(1, max_norm / (norm_k + 1e-6)), g <- coef_k g
    m <- m + (g - m)(1 - beta1);  v <- beta2 v + (1 - beta2) g g
    p <- p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
tests/test_optim_cpu.py pins it to torch's own float64 Adam + clip_grad_norm_.

The bars (u = 2^-24; one step from identical fp32 state, so only local arithmetic is measured):
    |m' - m'64| <= 3u (|m| + |g|)       |v' - v'64| <= 6u (v + g^2)       |p' - p'64| <= 8u (|p'64| + |delta64|)
    clipped |g - g64| <= 8u |g64|       grad_norm within 8u relative
with g the gradient that enters Adam (after clipping).  torch's fp32 Adam + grad_norm_clip_ reaches at most 0.97u, 2.2u,
3.1u and 2.6u in the first four units; the bars leave the room a differently ordered but equally valid formulation needs
(at most about 8 roundings per output) and are not fitted to the kernel.
"""
import torch

U = 2.0 ** -24
BETAS = (0.9, 0.999)


def tensor_shapes(name, N):
    """Per-agent-stacked shapes of the tensor sets: the smallest at which each branch of the kernel can go wrong."""
    if name == "mlp_tiny":      # (H, F, A) = (5, 3, 2): 15-, 5-, 10- and 2-element slices, unaligned for odd agents
        H, F, A = 5, 3, 2
        return [(N, H, F), (N, H), (N, A, H), (N, A)]
    if name == "mlp":           # (64, 31, 8)
        H, F, A = 64, 31, 8
        return [(N, H, F), (N, H), (N, A, H), (N, A)]
    if name == "rnn":           # the GRU nets' 8 tensors at H = 20, F = 12
        H, F, A = 20, 12, 4
        return [(N, 3 * H, F), (N, 3 * H, H), (N, 3 * H), (N, 3 * H), (N, H, H), (N, H), (N, A, H), (N, A)]
    if name == "rdqn":          # the iRDQN Q-net's 10 tensors at H = 16
        H, F, A = 16, 10, 8
        return [(N, 3 * H, F), (N, 3 * H, H), (N, 3 * H), (N, 3 * H), (N, H, H), (N, H), (N, H, H), (N, H), (N, A, H),
                (N, A)]
    if name == "critic":        # n_agents = 1: a lone large tensor over many workgroups with a ragged tail
        assert N == 1
        return [(128, 771), (128,), (1, 128), (1,)]
    raise KeyError(name)


def random_state(shapes, seed, grad_scale=1.0, zero_grad=False):
    """fp32 CPU lists p, g, m, v of a run in progress.  The moments are a state Adam can reach: the float64 moving
    averages of one history of 4 random gradients, m = sum 0.1 * 0.9^j g_j and v = sum 0.001 * 0.999^j g_j^2, rounded to
    fp32.  Moments drawn independently of each other would not be: by Cauchy-Schwarz every Adam state has
    |m| <= 7.3 sqrt(v) at the default betas, while an independent v near zero under a large m makes the step
    lr m / sqrt(v) arbitrarily sensitive to the rounding of m in ANY fp32 formulation (torch's included), which is a
    property of such an input and not of the arithmetic under test.
    The parameters are 0.05 .. 0.15 in size with a random sign, never near zero: the bar on p' is relative to
    |p'| + |delta|, while the bar on m' is absolute, 3u (|m| + |g|).  Where 0.9 m and 0.1 g cancel, delta is small and
    inherits an error of up to step_size * 3u (|m| + |g|) / (sqrt(v') / bc2s) <= lr * 0.8 * 3u * 39 = 0.28u at
    lr = 3e-3 (39: the Cauchy-Schwarz bound above plus 1 / sqrt(1 - beta2)), which the p bar covers only once
    8u |p'| exceeds it: 0.36u at |p| >= 0.05 does, a parameter that happens to be 1e-5 does not -- for torch's
    own formulation either (tests/test_optim_cpu.py shows torch's fp32 Adam missing the bar at |p| = 1e-5 on such moments
    and meeting it on the same moments at these sizes)."""
    gen = torch.Generator().manual_seed(seed)
    p = [(0.05 + 0.1 * torch.rand(s, generator=gen)) * (torch.randint(0, 2, s, generator=gen) * 2 - 1) for s in shapes]
    g = [torch.zeros(s) if zero_grad else torch.randn(s, generator=gen) * grad_scale for s in shapes]
    m, v = [], []
    for s in shapes:
        mi, vi = torch.zeros(s, dtype=torch.float64), torch.zeros(s, dtype=torch.float64)
        for _ in range(4):
            h = torch.randn(s, generator=gen).double() * grad_scale
            mi = mi + (h - mi) * (1 - BETAS[0])
            vi = BETAS[1] * vi + (1 - BETAS[1]) * h * h
        m.append(mi.float())
        v.append(vi.float())
    return p, g, m, v


def agent_norms64(g, N):
    sq = sum(x.double().reshape(N, -1).pow(2).sum(1) for x in g)
    return sq.sqrt()


def clip_adam64(p, g, m, v, N, t, lr=1e-3, betas=BETAS, eps=1e-8, max_norm=None):
    """One step in float64 from the given state (lists of tensors of any float dtype, [N, ...] each or whole tensors
    with N = 1).  Returns dict(p, g, m, v, delta: lists of float64 tensors; norm: [N] float64 or None)."""
    b1, b2 = betas
    p, g, m, v = ([x.double() for x in xs] for xs in (p, g, m, v))
    norm = None
    if max_norm is not None and max_norm > 0:
        norm = agent_norms64(g, N)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        g = [x * coef.view((N,) + (1,) * (x.dim() - 1)) if N > 1 else x * coef[0] for x in g]
    m2 = [mi + (gi - mi) * (1 - b1) for mi, gi in zip(m, g)]
    v2 = [b2 * vi + (1 - b2) * gi * gi for vi, gi in zip(v, g)]
    bc2s = (1 - b2 ** t) ** 0.5
    step_size = lr / (1 - b1 ** t)
    delta = [step_size * mi / (vi.sqrt() / bc2s + eps) for mi, vi in zip(m2, v2)]
    p2 = [pi - di for pi, di in zip(p, delta)]
    return dict(p=p2, g=g, m=m2, v=v2, delta=delta, norm=norm)


def _worst(err, bar):
    """max of err / bar over the elements (0 / 0 counts as 0: an exact result where the bar is zero)"""
    r = torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def one_step_ratios(got, ref, m0, v0):
    """The step's errors in units of their bars (each must be <= 1).  got: dict(p, g, m, v: lists of fp32 tensors,
    norm); ref: clip_adam64's result; m0, v0: the state before the step."""
    out = {"m": 0.0, "v": 0.0, "p": 0.0, "g": 0.0, "norm": 0.0}
    for i in range(len(ref["p"])):
        g64 = ref["g"][i]
        out["m"] = max(out["m"], _worst((got["m"][i].double() - ref["m"][i]).abs(),
                                        3 * U * (m0[i].double().abs() + g64.abs())))
        out["v"] = max(out["v"], _worst((got["v"][i].double() - ref["v"][i]).abs(), 6 * U * (v0[i].double() + g64 * g64)))
        out["p"] = max(out["p"], _worst((got["p"][i].double() - ref["p"][i]).abs(),
                                        8 * U * (ref["p"][i].abs() + ref["delta"][i].abs())))
        if ref["norm"] is not None:
            out["g"] = max(out["g"], _worst((got["g"][i].double() - g64).abs(), 8 * U * g64.abs()))
    if ref["norm"] is not None:
        out["norm"] = _worst((got["norm"].double() - ref["norm"]).abs(), 8 * U * ref["norm"])
    return out
