"""d2d_adam_step (csrc/optim_kernels.hip) and d2dhip.optim.StackedAdam on the GPU (pytest -m gpu).

One step from identical fp32 state against the float64 oracle (tests/optim_oracle.py), held to the bars stated there,
on the smallest tensor sets at which each branch of the kernel can go wrong: per-agent slices that start unaligned,
a lone large tensor over many workgroups with a ragged tail, 1 / 3 / 5 / 64 agents, clipping off / inactive / one agent
far over the norm / all-zero gradients, host and device step counters at t = 1 and 1,000, two eps, and three buffer
alignments (16-byte aligned, all four pointers of a tensor one float off, the gradient alone two floats off -- the
scalar-access path).  Every buffer, the workspace included, sits between canary regions.  Then determinism, graph
capture, 5 steps against torch's fp32 Adam, and the state dict round trip through torch.optim.Adam."""
import ctypes
import types

import pytest

import optim_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAD = 64            # canary floats on either side of a buffer (256 bytes: the payload keeps the pad's alignment)
CANARY = 1234.5
LR = 3e-3
MAX_NORM = 20.0

SETS = [(name, N) for name in ("mlp_tiny", "mlp", "rnn", "rdqn") for N in (1, 3, 5, 64)] + [("critic", 1)]
CLIPS = ["off", "inactive", "one_over", "zero_grad"]
# (t, step on the device, eps, float offsets of (param, grad, exp_avg, exp_avg_sq) from 16-byte alignment)
COMBOS = [(1, False, 1e-8, (0, 0, 0, 0)), (1000, False, 1.5e-4, (1, 1, 1, 1)), (1, True, 1.5e-4, (0, 2, 0, 0)),
          (1000, True, 1e-8, (0, 0, 0, 0))]


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    from d2dhip import _lib
    return _lib, _lib.require_gpu()


class Guarded:
    """A device copy of `t` at exactly its size between two canary regions, `shift` floats off 16-byte alignment."""

    def __init__(self, t, shift=0):
        n = t.numel()
        self.buf = torch.full((PAD + shift + n + PAD,), CANARY, dtype=torch.float32, device="cuda")
        self.lo, self.hi = PAD + shift, PAD + shift + n
        self.t = self.buf[self.lo:self.hi].view(t.shape)
        self.t.copy_(t)
        assert self.t.data_ptr() % 16 == 4 * shift % 16

    def intact(self):
        return bool((self.buf[:self.lo] == CANARY).all()) and bool((self.buf[self.hi:] == CANARY).all())


def run_step(state, N, t, on_device, eps, max_norm, shifts=(0, 0, 0, 0), lr=LR, short_ws=0):
    """One d2d_adam_step on guarded device copies of state = (p, g, m, v) (lists of fp32 CPU tensors).  Returns the
    results on the CPU, after asserting that every canary is intact."""
    _lib, lib = _gpu()
    G = [[Guarded(x, s) for x in xs] for xs, s in zip(state, shifts)]
    d = _lib.AdamDesc()
    d.n_agents, d.n_tensors = N, len(state[0])
    for i in range(len(state[0])):
        ten = d.tensors[i]
        ten.param, ten.grad, ten.exp_avg, ten.exp_avg_sq = (G[j][i].t.data_ptr() for j in range(4))
        ten.numel = state[0][i].numel() // N
    d.lr, d.beta1, d.beta2, d.eps = lr, O.BETAS[0], O.BETAS[1], eps
    d.max_norm = max_norm or 0.0
    step_dev = None
    if on_device:
        step_dev = torch.full((3,), -77, dtype=torch.int64, device="cuda")    # the counter between two canary words
        step_dev[1] = t - 1
        d.step, d.step_dev = 0, step_dev[1:].data_ptr()
    else:
        d.step = t
    need = lib.d2d_adam_workspace(ctypes.byref(d))
    assert need >= 0 and (need > 0) == bool(max_norm)
    ws = torch.full((256 + need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    norm = Guarded(torch.full((N,), -1.0)) if max_norm else None
    rc = lib.d2d_adam_step(ctypes.byref(d), ws[256:].data_ptr() if need else None, need - short_ws,
                           norm.t.data_ptr() if norm else None, _lib.stream_ptr())
    if short_ws:
        return rc, lib.d2d_last_error()
    _lib.check(rc, "d2d_adam_step")
    torch.cuda.synchronize()
    for xs in G:
        for x in xs:
            assert x.intact(), "a write outside a tensor"
    assert bool((ws[:256] == 0x5A).all()) and bool((ws[256 + need:] == 0x5A).all()), "a write outside the workspace"
    if norm is not None:
        assert norm.intact()
    if on_device:
        assert step_dev.tolist() == [-77, t, -77], "the device counter must read t afterwards"
    out = {k: [x.t.cpu().clone() for x in G[j]] for j, k in enumerate("pgmv")}
    out["norm"] = norm.t.cpu().clone() if norm is not None else None
    return out


def make_state(name, N, clip, seed):
    shapes = O.tensor_shapes(name, N)
    p, g, m, v = O.random_state(shapes, seed, zero_grad=clip == "zero_grad")
    if clip in ("inactive", "one_over"):      # every agent at no more than half the norm
        s = float(0.5 * MAX_NORM / O.agent_norms64(g, N).max())
        g = [x * s for x in g]
    if clip == "one_over":          # the last agent at 1,000x the others: far over the norm, the others under it
        for x in g:
            x.view(N, -1)[N - 1] *= 1000.0
    return p, g, m, v


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("name,N", SETS, ids=[f"{n}-N{N}" for n, N in SETS])
def test_one_step_matches_float64(name, N, clip):
    max_norm = None if clip == "off" else MAX_NORM
    worst = {}
    for ci, (t, on_device, eps, shifts) in enumerate(COMBOS):
        state = make_state(name, N, clip, 11 + ci)
        ref = O.clip_adam64(*state, N, t, lr=LR, eps=eps, max_norm=max_norm)
        got = run_step(state, N, t, on_device, eps, max_norm, shifts)
        ratios = O.one_step_ratios(got, ref, state[2], state[3])
        for k, r in ratios.items():
            worst[k] = max(worst.get(k, 0.0), r)
        print(f"  {name} N={N} {clip} t={t} dev={on_device} eps={eps} shifts={shifts}: " +
              ", ".join(f"{k} {r:.2f}" for k, r in ratios.items()) + " (bars = 1)")
        for k, r in ratios.items():
            assert r <= 1.0, (k, r, t, on_device, eps, shifts)
        for xs in (got["p"], got["m"], got["v"], got["g"]):
            assert all(bool(torch.isfinite(x).all()) for x in xs)
        if max_norm is None:
            assert all(torch.equal(a, b) for a, b in zip(got["g"], state[1])), "no clipping: the gradient is not touched"
        else:
            norm64 = ref["norm"]
            over = norm64 > max_norm
            if clip == "inactive":
                assert not over.any()
                assert all(torch.equal(a, b) for a, b in zip(got["g"], state[1])), "coef = 1 leaves the gradient"
            elif clip == "one_over":
                assert over[N - 1] and not over[:N - 1].any()
            elif clip == "zero_grad":  # coef = 1, no NaN
                assert torch.equal(got["norm"], torch.zeros(N))
                assert all(bool((x == 0).all()) for x in got["g"])
        if clip == "one_over" and N > 1:
            # the agents under the norm do not depend on the one over it: the same results, bit for bit, with that
            # agent's gradient replaced by zeros
            z = [x.clone() for x in state[1]]
            for x in z:
                x.view(N, -1)[N - 1] = 0.0
            alt = run_step((state[0], z, state[2], state[3]), N, t, on_device, eps, max_norm, shifts)
            for k in "pgmv":
                for a, b in zip(got[k], alt[k]):
                    assert torch.equal(a.view(N, -1)[:N - 1], b.view(N, -1)[:N - 1]), k
            assert torch.equal(got["norm"][:N - 1], alt["norm"][:N - 1])


def test_zero_state_and_zero_gradient_leave_the_parameters():
    """v = 0, g = 0 (and m = 0): the step is 0 / (0 + eps) = 0, p is unchanged, with and without clipping."""
    for N, name in ((5, "mlp_tiny"), (1, "critic")):
        shapes = O.tensor_shapes(name, N)
        p = O.random_state(shapes, 3)[0]
        zeros = [torch.zeros(s) for s in shapes]
        for max_norm in (None, MAX_NORM):
            for eps in (1e-8, 1.5e-4):
                got = run_step((p, zeros, zeros, zeros), N, 1, False, eps, max_norm)
                for k, want in (("p", p), ("m", zeros), ("v", zeros), ("g", zeros)):
                    assert all(torch.equal(a, b) for a, b in zip(got[k], want)), k


def test_workspace_one_byte_short_is_refused():
    state = make_state("mlp", 3, "inactive", 5)
    rc, msg = run_step(state, 3, 1, False, 1e-8, MAX_NORM, short_ws=1)
    assert rc == -1 and b"workspace" in msg and b"too small" in msg


@pytest.mark.parametrize("name,N", [("rnn", 5), ("critic", 1), ("mlp_tiny", 64)])
def test_two_calls_on_cloned_inputs_are_bitwise_equal(name, N):
    state = make_state(name, N, "one_over", 9)
    a = run_step(state, N, 8, True, 1e-8, MAX_NORM)
    b = run_step([[x.clone() for x in xs] for xs in state], N, 8, True, 1e-8, MAX_NORM)
    # and at another alignment of every buffer: the order of the norm's sum depends on the sizes alone
    c = run_step(state, N, 8, True, 1e-8, MAX_NORM, shifts=(1, 1, 1, 1))
    e = run_step(state, N, 8, True, 1e-8, MAX_NORM, shifts=(0, 3, 0, 0))
    for other in (b, c, e):
        for k in "pgmv":
            assert all(torch.equal(x, y) for x, y in zip(a[k], other[k])), k
        assert torch.equal(a["norm"], other["norm"])


def _stacked(name, N, seed, max_norm, lr=LR, eps=1e-8):
    from d2dhip.optim import StackedAdam
    shapes = O.tensor_shapes(name, N)
    p0 = O.random_state(shapes, seed)[0]
    params = [torch.nn.Parameter(x.cuda()) for x in p0]
    return params, StackedAdam(params, N, lr=lr, eps=eps, max_norm=max_norm), shapes


def test_graph_capture_and_replay():
    """One warm-up step run eagerly (on a side stream, as torch asks before a capture), then step() captured once --
    capturing records the launches and runs none -- and replayed 3 times: 1 + 0 + 3 = 4 steps, which equal 4 eager
    steps on a clone bit for bit; the device step reads 4 on both.  The graph is linear: norm partials, finalize,
    update on one stream."""
    _gpu()
    N = 5
    pa, oa, shapes = _stacked("mlp", N, 21, MAX_NORM)
    pb, ob, _ = _stacked("mlp", N, 21, MAX_NORM)
    g0 = [x.cuda() * 30 for x in O.random_state(shapes, 22)[1]]        # over the norm: the clip is active
    grads_a = [x.clone() for x in g0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step(grads=grads_a)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step(grads=grads_a)
    torch.cuda.synchronize()
    assert int(oa.step_count) == 1, "capturing must not run the step"
    for _ in range(3):
        for dst, src in zip(grads_a, g0):                               # the step clips the gradient in place:
            dst.copy_(src)                                              # refill the graph's static buffer
        graph.replay()
    for _ in range(4):
        ob.step(grads=[x.clone() for x in g0])
    torch.cuda.synchronize()
    assert int(oa.step_count) == 4 and int(ob.step_count) == 4
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    for a, b in zip(oa.exp_avg + oa.exp_avg_sq, ob.exp_avg + ob.exp_avg_sq):
        assert torch.equal(a, b)
    assert torch.equal(oa.grad_norm, ob.grad_norm)


def test_five_steps_against_torch_fp32():
    """K = 5 steps with fresh random gradients on the (64, 31, 8) set, per element:
    |p_hip - p64| <= 4 max|p_torch - p64| + u max|p| -- four times the torch path's own distance from the float64
    trajectory (grad_norm_clip_ + torch.optim.Adam in fp32 on the GPU), the rule of DESIGN §1 round 4.  The share of
    elements bit-equal to torch's is printed: information, not a bar."""
    _gpu()
    from algorithms._core import StackedNets
    N, K = 5, 5
    ph, oh, shapes = _stacked("mlp", N, 31, MAX_NORM)
    pt = [torch.nn.Parameter(p.detach().clone()) for p in ph]
    ot = torch.optim.Adam(pt, lr=LR)
    stack = types.SimpleNamespace(N=N, params={str(i): p for i, p in enumerate(pt)})
    p64 = [p.detach().cpu().double() for p in ph]
    m64 = [torch.zeros_like(x) for x in p64]
    v64 = [torch.zeros_like(x) for x in p64]
    for t in range(1, K + 1):
        g = [x * (40.0 if t % 2 else 1.0) for x in O.random_state(shapes, 40 + t)[1]]   # odd steps over the norm
        oh.step(grads=[x.cuda() for x in g])
        for p, x in zip(pt, g):
            p.grad = x.cuda()
        StackedNets.grad_norm_clip_(stack, MAX_NORM)
        ot.step()
        r = O.clip_adam64(p64, g, m64, v64, N, t, lr=LR, max_norm=MAX_NORM)
        p64, m64, v64 = r["p"], r["m"], r["v"]
    worst, equal, total = 0.0, 0, 0
    for a, b, c in zip(ph, pt, p64):
        a, b = a.detach().cpu(), b.detach().cpu()
        d_t = float((b.double() - c).abs().max())
        bar = 4 * d_t + O.U * float(c.abs().max())
        d_h = float((a.double() - c).abs().max())
        worst = max(worst, d_h / bar)
        equal += int((a == b).sum())
        total += a.numel()
        assert d_h <= bar, (d_h, d_t, bar)
    print(f"  5 steps: worst |p_hip - p64| / (4 max|p_torch - p64| + u max|p|) = {worst:.3f}; "
          f"{equal / total:.4f} of the elements bit-equal to torch's")


def test_state_dict_round_trip_through_torch_adam():
    """2 steps on StackedAdam A; A's state loads into a torch.optim.Adam T over a clone, T's state into a fresh
    StackedAdam B over another clone.  The third step: B equals A bit for bit, T and A are each within the one-step
    bars of the float64 step from that state, and all three are at step 3."""
    _gpu()
    from d2dhip.optim import StackedAdam
    N = 3
    pa, oa, shapes = _stacked("rnn", N, 51, None, eps=1.5e-4)
    for t in (1, 2):
        oa.step(grads=[x.cuda() for x in O.random_state(shapes, 60 + t)[1]])
    sd = oa.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    assert float(sd["state"][0]["step"]) == 2.0 and sd["param_groups"][0]["params"] == list(range(len(pa)))
    pt = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ot = torch.optim.Adam(pt, lr=1.0)                                    # (lr, eps come with the state dict)
    ot.load_state_dict(sd)
    assert ot.param_groups[0]["lr"] == LR and ot.param_groups[0]["eps"] == 1.5e-4
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = StackedAdam(pb, N, lr=1.0)
    ob.load_state_dict(ot.state_dict())
    assert int(ob.step_count) == 2 and ob.param_groups[0]["lr"] == LR and ob.param_groups[0]["eps"] == 1.5e-4
    state = ([p.detach().cpu() for p in pa], O.random_state(shapes, 63)[1], [x.cpu() for x in oa.exp_avg],
             [x.cpu() for x in oa.exp_avg_sq])
    ref = O.clip_adam64(*state, N, 3, lr=LR, eps=1.5e-4)
    g3 = [x.cuda() for x in state[1]]
    oa.step(grads=g3)
    ob.step(grads=[x.clone() for x in g3])
    for p, x in zip(pt, g3):
        p.grad = x.clone()
    ot.step()
    assert int(oa.step_count) == 3 and int(ob.step_count) == 3 and float(ot.state[pt[0]]["step"]) == 3.0
    for a, b in zip(pa + oa.exp_avg + oa.exp_avg_sq, pb + ob.exp_avg + ob.exp_avg_sq):
        assert torch.equal(a, b)
    for who, params, ms, vs in (("hip", pa, oa.exp_avg, oa.exp_avg_sq),
                                ("torch", pt, [ot.state[p]["exp_avg"] for p in pt],
                                 [ot.state[p]["exp_avg_sq"] for p in pt])):
        got = dict(p=[p.detach().cpu() for p in params], m=[x.cpu() for x in ms], v=[x.cpu() for x in vs],
                   g=state[1], norm=None)
        ratios = O.one_step_ratios(got, ref, state[2], state[3])
        print(f"  third step, {who}: " + ", ".join(f"{k} {r:.2f}" for k, r in ratios.items()))
        assert all(r <= 1.0 for r in ratios.values()), (who, ratios)
    # a torch Adam that has not stepped yet has no state: it loads as zeros at step 0
    fresh = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in pa], lr=LR)
    ob.load_state_dict(fresh.state_dict())
    assert int(ob.step_count) == 0 and all(bool((x == 0).all()) for x in ob.exp_avg + ob.exp_avg_sq)


def test_nan_norm_propagates_as_torch_clamp_does():
    """A NaN in one agent's gradient: its norm and coefficient are NaN and go into all of that agent's gradient, as
    torch.clamp(max_norm / (norm + 1e-6), max=1) * grad does; the other agents are untouched by it."""
    N = 3
    state = make_state("mlp_tiny", N, "inactive", 4)
    state[1][0].view(N, -1)[1, 0] = float("nan")
    got = run_step(state, N, 1, False, 1e-8, MAX_NORM)
    assert bool(torch.isnan(got["norm"][1])) and bool(torch.isfinite(got["norm"][[0, 2]]).all())
    for k in "gpmv":
        for x in got[k]:
            assert bool(torch.isnan(x.view(N, -1)[1]).all()) and bool(torch.isfinite(x.view(N, -1)[[0, 2]]).all()), k
