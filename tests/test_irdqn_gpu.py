"""GPU parity of the iRDQN kernels (csrc/rdqn_kernels.hip, d2dhip/rdqn.py) against plain torch of the same ops in
float64: the reference's RNN Q-network (GRU from h0 = 0 -> Linear -> ReLU -> Linear -> ReLU -> Linear,
algorithms/irdqn.py:58-86), DQN.act's epsilon-greedy choice (irdqn.py:150-160) and the gradients of DQN.train_step's TD
loss (irdqn.py:133-148) through the window.

Tolerances (the rules tests/test_gru_gpu.py states): Q-values 1e-5 absolute, or twice torch fp32's own distance to
float64; gradients within 2e-5 * max|g| of float64 autograd where torch fp32 itself lands in that band, else within 4x
torch fp32's distance; loss 1e-5 relative."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from irdqn_oracle import net_q  # noqa: E402  (the float64 oracle, pinned to the reference by test_irdqn_cpu.py)

SHAPES = [(12, 100, 4), (30, 100, 8), (5, 16, 2), (46, 128, 16)]  # F, H, A
N = 3


def make_params(F, H, A, seed, n=N):
    """Agent-stacked parameters with torch's default init ranges (the GRU's spread so the gates leave their linear
    regime) and unequal in_dims: agent k uses the first dims[k] inputs (zero weight columns past them)."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) / H ** 0.5  # noqa: E731
    p = {"w_ih": 2 * u(n, 3 * H, F), "w_hh": 2 * u(n, 3 * H, H), "b_ih": u(n, 3 * H), "b_hh": u(n, 3 * H),
         "w1": u(n, H, H), "b1": u(n, H), "w2": u(n, H, H), "b2": u(n, H), "w3": u(n, A, H), "b3": u(n, A)}
    dims = [max(1, F - 2 * k) for k in range(n)]
    for k, d in enumerate(dims):
        p["w_ih"][k, :, d:] = 0
    return p, dims


def make_ring(rows, E, F, dims, seed):
    g = torch.Generator().manual_seed(seed)
    ring = torch.randint(-1, 4, (rows, E, len(dims), F), generator=g).float()
    ring += torch.rand(ring.shape, generator=g) * 0.3
    for k, d in enumerate(dims):
        ring[:, :, k, d:] = 0
    return ring


def gather(ring, samples, rows_of):
    """Windows of the samples grouped by length: {S: (sample indices, win [N][n][S][F])}."""
    out = {}
    for b, (e, last, S) in enumerate(samples):
        out.setdefault(S, ([], []))
        out[S][0].append(b)
        out[S][1].append(ring[rows_of(last, S), e])                       # [S][N][F]
    return {S: (idx, torch.stack(w).permute(2, 0, 1, 3)) for S, (idx, w) in out.items()}


def ref_q(p, ring, samples, dtype, rows_of=None):
    rows = ring.shape[0]
    rows_of = rows_of or (lambda last, S: [(last - S + 1 + j) % rows for j in range(S)])
    q = {k: v.to(dtype) for k, v in p.items()}
    n, A = p["w3"].shape[:2]
    out = torch.zeros(n, len(samples), A, dtype=dtype)
    for S, (idx, win) in gather(ring.to(dtype), samples, rows_of).items():
        out[:, idx] = net_q(q, win)
    return out


def dev(p):
    return {k: v.cuda().contiguous() for k, v in p.items()}


def mixed_samples(B, L, E, rows, seed):
    rng = np.random.default_rng(seed)
    lens = [(1, 2, L)[b % 3] for b in range(B)]
    if B >= 3:
        rng.shuffle(lens)
    return [(int(rng.integers(E)), int(rng.integers(S - 1, rows)), int(S)) for S in lens]


def masks_to_idx(act):
    a = act.cpu().to(torch.int64) & 0xFFFF
    idx = torch.log2(a.double()).round().long()
    assert torch.equal(torch.ones_like(a) << idx, a), "not one-hot"
    return idx


Q_CASES = [(s, L, B) for s in SHAPES for L in (5, 16) for B in (1, 17, 32)] + [(SHAPES[1], 256, 3)]


@pytest.mark.parametrize("case", Q_CASES, ids=lambda c: f"F{c[0][0]}-H{c[0][1]}-A{c[0][2]}-L{c[1]}-B{c[2]}")
def test_q_matches_float64(case):
    from d2dhip import rdqn
    (F, H, A), L, B = case
    E, rows = 5, L + 7
    p, dims = make_params(F, H, A, seed=H + F)
    ring = make_ring(rows, E, F, dims, seed=L)
    samples = mixed_samples(B, L, E, rows, seed=B)
    q64, q32 = ref_q(p, ring, samples, torch.float64), ref_q(p, ring, samples, torch.float32)
    q, qmax, act = rdqn.q_values(dev(p), ring.cuda(), torch.tensor(samples, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    assert q.shape == (N, B, A) and qmax.shape == (N, B) and act.shape == (B, N)
    assert act.dtype == (torch.uint8 if A <= 8 else torch.int16)
    err = (q.cpu().double() - q64).abs()
    tol = torch.clamp(2 * (q32.double() - q64).abs(), min=1e-5)
    print(f"  max |kernel - f64| {err.max().item():.2e}  max |torch f32 - f64| {(q32.double() - q64).abs().max().item():.2e}")
    assert torch.all(err <= tol), (err - tol).max().item()
    # qmax and the greedy action are the max / lowest-index argmax of the kernel's own q, bitwise
    qc = q.cpu()
    assert torch.equal(qmax.cpu(), qc.max(-1).values)
    first = (qc == qc.max(-1, keepdim=True).values).int().argmax(-1)     # lowest index among ties
    assert torch.equal(masks_to_idx(act), first.t())


def test_greedy_ties_take_the_lowest_index():
    from d2dhip import rdqn
    F, H, A = 5, 16, 8
    p, dims = make_params(F, H, A, seed=1)
    p["w3"].zero_()
    p["b3"][:] = torch.tensor([0., 1., 3., 3., 2., 3., 0., 1.])
    ring = make_ring(4, 2, F, dims, seed=0)
    s = torch.tensor([(0, 3, 2), (1, 2, 1)], dtype=torch.int32).cuda()
    q, qmax, act = rdqn.q_values(dev(p), ring.cuda(), s)
    assert torch.all(masks_to_idx(act) == 2) and torch.all(qmax == 3)


def _eps_setup(E, n, A=4):
    """A net whose greedy action is always A - 1 (a large output bias), so explore actions (0 / 1) are visible."""
    F, H = 5, 16
    p, dims = make_params(F, H, A, seed=2, n=n)
    p["b3"][:, A - 1] = 100.0
    ring = make_ring(3, E, F, dims, seed=3)
    samples = torch.tensor([(e, 2, 2) for e in range(E)], dtype=torch.int32).cuda()
    return dev(p), ring.cuda(), samples


def test_epsilon_greedy():
    from d2dhip import rdqn
    E, n, A = 512, 8, 4
    p, ring, s = _eps_setup(E, n, A)
    g = torch.Generator().manual_seed(0)
    em = (torch.rand(E, n, generator=g) < 0.3).to(torch.uint8)
    ea = torch.randint(0, A, (E, n), generator=g).to(torch.uint8)
    act = rdqn.q_values(p, ring, s, mode="forced", explore_mask=em.cuda(), explore_action=ea.cuda())[2]
    want = torch.where(em.bool(), ea.long(), torch.full((E, n), A - 1))
    assert torch.equal(masks_to_idx(act), want)
    run = lambda **kw: masks_to_idx(rdqn.q_values(p, ring, s, mode="eps", seed=7, **kw)[2])  # noqa: E731
    assert torch.all(run(eps=0.0, ready=True) == A - 1)
    for kw in (dict(eps=0.0, ready=False), dict(eps=1.0, ready=True)):
        a = run(**kw)
        assert torch.all(a <= 1) and 0 < int(a.sum()) < a.numel()          # both explore actions occur
    a = run(eps=0.5, ready=True, rng_step=5)
    n_explore = int((a <= 1).sum())
    print(f"  explore count {n_explore} of {a.numel()}")
    assert a.numel() == 4096 and abs(n_explore - 2048) <= 160                # 5 sigma of Binomial(4096, 1/2)
    assert torch.all((a <= 1) | (a == A - 1))
    assert torch.equal(a, run(eps=0.5, ready=True, rng_step=5))
    assert not torch.equal(a, run(eps=0.5, ready=True, rng_step=6))
    # the draw belongs to (env_base + env, agent, rng_step), not to the sample's position in the batch
    half = masks_to_idx(rdqn.q_values(p, ring, s[E // 2:].contiguous(), mode="eps", seed=7, eps=0.5, rng_step=5)[2])
    assert torch.equal(half, a[E // 2:])


def ref_td(p, ring, samples, L, act, reward, done, qt, gamma, loss, dtype, rows_of=None):
    q = {k: v.to(dtype).requires_grad_() for k, v in p.items()}
    rows = ring.shape[0]
    rows_of = rows_of or (lambda last, S: [(last - S + 1 + j) % rows for j in range(S)])
    (idx, win), = gather(ring.to(dtype), [(e, last, L) for e, last, _ in samples], rows_of).values()
    Q = net_q(q, win)                                                      # [N][B][A]
    qa = Q.gather(2, act.t().unsqueeze(-1)).squeeze(-1)                    # [N][B]
    td = reward.t().to(dtype) + (1 - done.to(dtype)).unsqueeze(0) * gamma * qt.to(dtype)
    if loss == "huber":
        ls = torch.nn.functional.smooth_l1_loss(qa, td, reduction="none").mean(1)
    else:
        ls = ((qa - td) ** 2).mean(1)
    ls.sum().backward()
    return {k: v.grad for k, v in q.items()}, ls.detach(), (qa - td).detach()


def td_inputs(B, A, seed):
    g = torch.Generator().manual_seed(seed)
    act = torch.randint(0, A, (B, N), generator=g)
    reward = torch.randn(B, N, generator=g) * 1.5                          # delta on both sides of +-1
    done = (torch.arange(B) % 2 == 1) if B > 1 else torch.zeros(1, dtype=torch.bool)
    qt = torch.randn(N, B, generator=g)
    return act, reward, done, qt


def run_grads(p, ring, samples, L, act, reward, done, qt, gamma, loss, A, ring_episode=0):
    from d2dhip import rdqn
    masks = (torch.ones_like(act) << act).to(rdqn.mask_dtype(A))
    g, ls = rdqn.grads(dev(p), ring.cuda(), torch.tensor(samples, dtype=torch.int32).cuda(), L, masks.cuda(),
                       reward.cuda(), done.cuda(), qt.cuda(), gamma, loss, ring_episode=ring_episode)
    torch.cuda.synchronize()
    return g, ls


def check_grads(got, ls, r64, l64, r32, p):
    for name in r64:
        assert got[name].shape == p[name].shape
        gk = got[name].cpu().double()
        scale = r64[name].abs().max().item()
        err64 = (gk - r64[name]).abs().max().item()
        band = (r32[name].double() - r64[name]).abs().max().item()
        print(f"  {name}: max|g| {scale:.3e}  |kernel-f64| {err64:.2e}  |torchf32-f64| {band:.2e}")
        tol = 2e-5 * scale + 1e-7
        assert err64 <= (tol if band <= tol else 4 * band), (name, err64, tol, band)
    torch.testing.assert_close(ls.cpu().double(), l64, rtol=1e-5, atol=1e-7)


GRAD_CASES = [(s, L, B) for s in SHAPES for L in (1, 5, 16) for B in (1, 32, 33)] + [(SHAPES[0], 256, 2)]


@pytest.mark.parametrize("loss", ["huber", "mse"])
@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: f"F{c[0][0]}-H{c[0][1]}-A{c[0][2]}-L{c[1]}-B{c[2]}")
def test_grads_match_autograd(case, loss):
    (F, H, A), L, B = case
    E, rows, gamma = 4, L + 6, 0.4
    p, dims = make_params(F, H, A, seed=3 + H + F)
    ring = make_ring(rows, E, F, dims, seed=L + 1)
    rng = np.random.default_rng(B + L)
    samples = [(int(rng.integers(E)), int(rng.integers(rows)), L) for _ in range(B)]  # some windows wrap the ring
    act, reward, done, qt = td_inputs(B, A, seed=B)
    r64, l64, d64 = ref_td(p, ring, samples, L, act, reward, done, qt, gamma, loss, torch.float64)
    r32, _, _ = ref_td(p, ring, samples, L, act, reward, done, qt, gamma, loss, torch.float32)
    if B >= 32:
        assert (d64.abs() < 1).any() and (d64.abs() > 1).any() and done.any() and not done.all()
    got, ls = run_grads(p, ring, samples, L, act, reward, done, qt, gamma, loss, A)
    check_grads(got, ls, r64, l64, r32, p)
    for k, d in enumerate(dims):  # unused input columns get exactly zero gradient
        assert torch.all(got["w_ih"][k, :, d:] == 0)
    again, ls2 = run_grads(p, ring, samples, L, act, reward, done, qt, gamma, loss, A)
    for name in got:
        assert torch.equal(got[name], again[name]), name
    assert torch.equal(ls, ls2)


def test_unsupported_shapes_raise_before_any_launch():
    from d2dhip import _lib, rdqn
    import ctypes
    p, dims = make_params(12, 144, 4, seed=0)
    ring = make_ring(4, 2, 12, dims, seed=0).cuda()
    s = torch.tensor([(0, 3, 2)], dtype=torch.int32).cuda()
    with pytest.raises(NotImplementedError, match="hidden <= 128"):
        rdqn.q_values(dev(p), ring, s)
    # the library itself refuses as well (D2D_EUNSUPPORTED)
    lib = _lib.require_gpu()
    w = ctypes.c_void_p(16)
    d = _lib.RdqnDesc(2, 2, 12, 144, 4, 4, 0, 0, *([w] * 10), 0, 0, None)
    assert lib.d2d_rdqn_q(ctypes.byref(d), w, w, 1, 0, 0, 0.0, None, 1, None, None, 0, w, None, None, None) == -2
    assert lib.d2d_rdqn_grad_workspace(ctypes.byref(d), 8, 4) == -1
    p, dims = make_params(12, 16, 4, seed=0)
    act, reward, done, qt = td_inputs(1, 4, seed=0)
    with pytest.raises(NotImplementedError, match="window length <= 256"):
        run_grads(p, make_ring(4, 2, 12, dims, seed=0), [(0, 3, 257)], 257, act, reward, done, qt, 0.4, "huber", 4)


def test_episode_ring_windows():
    """ring_episode = T: the ring holds episodes of T + 1 rows and window indices are transitions; transition m reads
    row m + m // T (+ 1 for its successor state).  Chunks across an episode boundary and across the ring's wrap-around
    equal the per-timeline sequences."""
    from d2dhip import rdqn
    F, H, A = 12, 100, 4
    T, n_ep, E, L = 6, 3, 4, 5
    rows, ntrans = n_ep * (T + 1), n_ep * T
    p, dims = make_params(F, H, A, seed=11)
    ring = make_ring(rows, E, F, dims, seed=12)
    lasts = [4, 7, 9, 17, 2, 0]       # inside an episode, across boundaries, the ring's last, wrapping to the end
    samples = [(b % E, last, L) for b, last in enumerate(lasts)]
    pd, rd, sd = dev(p), ring.cuda(), torch.tensor(samples, dtype=torch.int32).cuda()
    for shift in (0, 1):
        def rows_of(last, S, shift=shift):
            ms = [(last - S + 1 + j) % ntrans for j in range(S)]
            return [m + m // T + shift for m in ms]
        q64, q32 = ref_q(p, ring, samples, torch.float64, rows_of), ref_q(p, ring, samples, torch.float32, rows_of)
        q = rdqn.q_values(pd, rd, sd, ring_episode=T, row_shift=shift)[0]
        err = (q.cpu().double() - q64).abs()
        assert torch.all(err <= torch.clamp(2 * (q32.double() - q64).abs(), min=1e-5)), shift
    rows_of = lambda last, S: [m + m // T for m in [(last - S + 1 + j) % ntrans for j in range(S)]]  # noqa: E731
    act, reward, done, qt = td_inputs(len(samples), A, seed=5)
    r64, l64, _ = ref_td(p, ring, samples, L, act, reward, done, qt, 0.4, "huber", torch.float64, rows_of)
    r32, _, _ = ref_td(p, ring, samples, L, act, reward, done, qt, 0.4, "huber", torch.float32, rows_of)
    got, ls = run_grads(p, ring, samples, L, act, reward, done, qt, 0.4, "huber", A, ring_episode=T)
    check_grads(got, ls, r64, l64, r32, p)


# ------------------------------------------------------------------------------------------------ the learner
def make_env(E, N=2, C=2, T=6, seed=3):
    from envs.combinatorial_env import CombinatorialEnv
    return CombinatorialEnv(N, C, np.array([3] * N), np.ones(N) * 0.7, episode_length=T, n_envs=E, device="cuda:0",
                            seed=seed)


def make_learner(E, **kw):
    from algorithms.irdqn import iRDQN
    torch.manual_seed(0)
    args = dict(history_len=3, replay_start_size=2, replay_buffer_size=10 ** 4, gamma=0.4, update_target_frequency=2,
                minibatch_size=8, learning_rate=1e-3)
    args.update(kw)
    return iRDQN(make_env(E), **args)


def test_learner_refuses_unsupported_shapes():
    from algorithms.irdqn import iRDQN
    with pytest.raises(NotImplementedError, match="window length <= 256"):
        iRDQN(make_env(1), history_len=300)
    with pytest.raises(NotImplementedError, match="callable"):
        iRDQN(make_env(1), loss=lambda a, b, reduction: 0)


@pytest.mark.parametrize("E", [1, 4])
def test_replay_ring_windows(E):
    """With obs rows that encode (env, episode, t), the states / states_next windows the update gathers equal the
    per-timeline sequences: across an episode boundary, after wrap-around, and never mixing envs."""
    from d2dhip import rdqn
    T, L, B = 6, 3, 8
    ln = make_learner(E, replay_buffer_size=3 * T * E, minibatch_size=B)
    b = ln._bind_env()
    n_waves = 7
    ln._alloc_ring(b, n_waves)
    assert ln._ring_ep == 4 and ln._cap == 3 * T                       # capacity 3 episodes per env + 1 being written
    s = b.spec
    timeline = []                                                        # per wave: rows [T + 1][E][N][F]
    for w in range(n_waves):
        slot = (ln._added // T) % ln._ring_ep
        code = torch.zeros(T + 1, E, s.N, s.F)
        for t in range(T + 1):
            for e in range(E):
                code[t, e] = e + 0.1 * w + 0.01 * t + torch.arange(s.N).view(-1, 1) * 0.003
        ln._ring[slot * (T + 1):(slot + 1) * (T + 1)] = code.cuda()
        timeline.append(code)
        ln._added += T
    states = torch.cat([c[:T] for c in timeline])                       # transition m of the timeline: [n_waves * T][E]..
    nexts = torch.cat([c[1:] for c in timeline])
    # the kernel does not expose its windows: compare the Q-values of the gathered windows with the oracle's
    p = {k: v.detach().cpu() for k, v in ln.network.data().items()}
    length, first = ln._cap, ln._added - ln._cap
    starts = np.array([0, T - 2, T - 1, length - L - 1, 5, 2 * T - 1, 3, 9])   # boundary-straddling and the newest allowed
    envs = np.arange(B) % E
    ln._sample_chunks = lambda n_envs, length_, bs, cs: (envs, starts)
    samples, done = ln._chunk_samples(E)
    last_abs = first + starts + L - 1
    assert np.array_equal(done.cpu().numpy(), (last_abs % T == T - 1).astype(np.uint8))
    for shift, src in ((0, states), (1, nexts)):
        win = torch.stack([src[m - L + 1:m + 1, e] for m, e in zip(last_abs, envs)])   # [B][L][N][F]
        assert all(torch.all(win[i, ..., 0, 0].floor().long() == envs[i]) for i in range(B))  # one env per chunk
        want64 = net_q({k: v.double() for k, v in p.items()}, win.permute(2, 0, 1, 3).double())
        want32 = net_q(p, win.permute(2, 0, 1, 3))
        q = rdqn.q_values(ln.network.data(), ln._ring, samples, ring_episode=T, row_shift=shift)[0]
        err = (q.cpu().double() - want64).abs()
        assert torch.all(err <= torch.clamp(2 * (want32.double() - want64).abs(), min=1e-5)), shift
    # neighbouring rows differ by 0.01: a window shifted by one row is far outside the tolerance
    wrong = net_q({k: v.double() for k, v in p.items()}, (win + 0.01).permute(2, 0, 1, 3).double())
    assert (wrong - want64).abs().max() > 1e-4


@pytest.mark.parametrize("E", [1, 4])
def test_train_and_test_end_to_end(E):
    ln = make_learner(E)
    snaps = []
    orig_wave, orig_update, orig_sync = ln._train_wave, ln._update, ln._sync_target

    def wave(b, ep0):
        snaps.append(("wave", ep0, {k: v.clone() for k, v in ln.network.data().items()}))
        return orig_wave(b, ep0)

    def update(n):
        out = orig_update(n)
        snaps.append(("update", None, {k: v.clone() for k, v in ln.network.data().items()}))
        return out

    def sync():
        orig_sync()
        for k, v in ln.network.data().items():
            assert torch.equal(v, ln.target_network.data()[k])            # target == network right after a sync
        snaps.append(("sync", None, None))

    ln._train_wave, ln._update, ln._sync_target = wave, update, sync
    w0 = {k: v.clone() for k, v in ln.network.data().items()}
    t0 = {k: v.clone() for k, v in ln.target_network.data().items()}
    for k in w0:
        assert torch.equal(w0[k], t0[k])                                  # the target starts as a copy
    scores, tests, rewards = ln.train(6, early_stopping=False)
    assert len(scores) == 6 and len(tests) == 1 and len(rewards) == 1
    assert all(0 <= s <= 1 for s in scores)
    assert ln.n_updates == 4 and ln.n_syncs == 2                          # episodes 2..5; syncs at 2 and 4
    losses = torch.stack(ln.losses).cpu()
    assert losses.shape == (4, 2) and torch.isfinite(losses).all()
    # weights unchanged until the first ready episode's update, changed by every update
    first_update = next(i for i, s in enumerate(snaps) if s[0] == "update")
    for kind, _, w in snaps[:first_update]:
        if kind == "wave":
            assert all(torch.equal(w[k], w0[k]) for k in w0)
    prev = w0
    for kind, _, w in snaps:
        if kind == "update":
            assert all(not torch.equal(w[k], prev[k]) for k in ("w_hh", "w1", "w3", "b3"))
            prev = w
    # one update after a sync the target differs from the network again
    kinds = [s[0] for s in snaps]
    assert "sync" in kinds and kinds[-1] == "update"
    assert any(not torch.equal(ln.network.data()[k], ln.target_network.data()[k]) for k in w0)
    # the per-agent modules are views of the stacked storage
    for k, a in enumerate(ln.agents):
        assert a.network.layers[4].weight.data_ptr() == ln.network.params["w3"][k].data_ptr()
        assert torch.equal(a.target_network.lstm.weight_hh_l0, ln.target_network.params["w_hh"][k])
    score, reward = ln.test(2)
    assert 0 <= score <= 1 and np.isfinite(reward) and reward >= 0
    assert ln.test(2) != () and isinstance(score, float)


# ------------------------------------------------------------------------- the reference's recorded runs
def ref_adam_tolerance(steps, name, lr_, shape, rel_err=2e-5, base=1e-5):
    """Per-element bound on |w_got - w_ref| after the recorded Adam steps, from the reference's gradients (the helper of
    tests/test_learner_gpu.py): 2 lr min(1, rel_err max|g| / |g|) per step; an exactly-zero gradient adds nothing."""
    tol = np.full(shape, base, dtype=np.float64)
    for st in steps:
        g = np.abs(st[name].astype(np.float64))
        err = rel_err * g.max()
        tol += np.where(g == 0, 0.0, 2 * lr_ * np.minimum(err / np.maximum(g, 1e-30), 1.0))
    return tol


def fixture_learner(loss, E=1):
    import irdqn_oracle as O
    from algorithms.irdqn import iRDQN
    from envs.combinatorial_env import CombinatorialEnv
    zc, z, cfg = O.load_case(loss)
    env = CombinatorialEnv(**O.env_kwargs(cfg), n_envs=E, device="cuda:0", seed=0)
    ln = iRDQN(env, loss=loss, **cfg["learner"])
    for i, a in enumerate(ln.agents):
        sd = {k: torch.from_numpy(zc[f"weights/agent{i}/network/{k}"].copy()) for k in O.SD_NAMES.values()}
        a.network.load_state_dict(sd)                                   # views: fills the stacked storage
        a.target_network.load_state_dict(sd)
    return ln, zc, z, cfg, O


@pytest.mark.parametrize("loss", ["huber", "mse"])
def test_reference_updates(loss):
    """The K = 3 recorded updates (the reference's DQN.train_step on ReplayBuffer.sample_chunk's minibatches) on the
    learner: the recorded transitions in the device ring, the recorded chunk starts injected."""
    ln, zc, z, cfg, O = fixture_learner(loss)
    lk = cfg["learner"]
    b = ln._bind_env()
    obs = torch.from_numpy(zc["buffer/obs"])                             # [episodes][T + 1][N][F]
    n_ep, T = obs.shape[0], obs.shape[1] - 1
    acts, rews = zc["buffer/actions"], zc["buffer/rewards"]
    assert np.all(rews == rews[:, :1]) and T == ln.env.episode_length   # one reward per env, broadcast to the agents
    ln._alloc_ring(b, n_ep)
    assert ln._cap == lk["replay_buffer_size"] and ln._ring_ep == 5
    for ep in range(n_ep):                                               # what _train_wave writes, episode by episode
        slot = (ln._added // T) % ln._ring_ep
        ln._ring[slot * (T + 1):(slot + 1) * (T + 1), 0] = obs[ep].cuda()
        ln._act_ring[slot * T:(slot + 1) * T, 0] = torch.from_numpy(1 << acts[ep * T:(ep + 1) * T]).to(torch.uint8).cuda()
        ln._rew_ring[slot * T:(slot + 1) * T, 0] = torch.from_numpy(rews[ep * T:(ep + 1) * T, 0]).int().cuda()
        ln._added += T
    grads_seen = []
    step = ln.optimizer.step
    ln.optimizer.step = lambda: (grads_seen.append({k: v.grad.clone() for k, v in ln.network.params.items()}), step())[1]
    for u in range(int(z["K"])):
        ln._sample_chunks = lambda n_envs, length, B, L, u=u: (np.zeros(B, dtype=np.int64), z[f"upd/{u}/starts"])
        ln._update(1)
    torch.cuda.synchronize()
    s64, final64 = O.trajectory(zc, z, cfg, loss)                        # pinned to the fixtures by test_irdqn_cpu.py
    s32, _ = O.trajectory(zc, z, cfg, loss, torch.float32)
    N = ln.n_agents
    # first update: losses and gradients against the reference's recorded ones
    for i in range(N):
        want = float(z[f"upd/0/agent{i}/loss"])
        assert abs(ln.losses[0][i].item() - want) <= 1e-5 * abs(want)
    for k, sd in O.SD_NAMES.items():
        got = grads_seen[0][k].cpu().double()
        ref = s64[0]["grads"][k]
        assert np.abs(ref[0].numpy() - z[f"upd/0/agent0/grad/{sd}"]).max() <= 1e-9 * np.abs(ref[0].numpy()).max()
        scale = ref.abs().max().item()
        err64 = (got - ref).abs().max().item()
        band = (s32[0]["grads"][k].double() - ref).abs().max().item()
        print(f"  {k}: max|g| {scale:.3e}  |kernel-ref| {err64:.2e}  |torchf32-ref| {band:.2e}")
        tol = 2e-5 * scale + 1e-7
        assert err64 <= (tol if band <= tol else 4 * band), (k, err64, tol, band)
    # weights after K updates: the Adam-aware bound from the reference trajectory's gradients
    for k, sd in O.SD_NAMES.items():
        for i in range(N):
            want = z[f"weights_after/agent{i}/{sd}"].astype(np.float64)
            steps = [{k: s["grads"][k][i].numpy()} for s in s64]
            tol = ref_adam_tolerance(steps, k, lk["learning_rate"], want.shape)
            d = np.abs(ln.network.params[k][i].detach().cpu().numpy().astype(np.float64) - want)
            assert (d <= tol).all(), (k, i, d.max(), tol[d > tol].min())
            assert np.median(tol) <= 0.05 * 2 * lk["learning_rate"] * len(s64) + 1e-5, k
            moved = np.abs(want - zc[f"weights/agent{i}/network/{sd}"])
            assert moved.max() > 10 * np.median(tol) or k in ("w_ih",)    # the check is not vacuous


@pytest.mark.parametrize("E", [1, 2, 4])
def test_reference_test_episodes(E):
    """iRDQN.test on the reference's recorded env draws: bit-equal greedy actions and the recorded return tuple, the 4
    recorded episodes on 1 env (4 waves), 2 envs (2 waves) and 4 envs side by side."""
    ln, zc, z, cfg, O = fixture_learner("huber", E)
    n_ep, T = 4, ln.env.episode_length
    teacher = dict(actions=None, reset_arrivals=zc["test/draws/reset_arrivals"], flips=zc["test/draws/flips"],
                   arrivals=zc["test/draws/arrivals"])
    res = ln._test(n_ep, teacher=teacher)
    np.testing.assert_allclose(np.array(res, dtype=np.float64), zc["test/result"], rtol=0, atol=1e-12)
    waves = n_ep // E
    got = masks_to_idx(ln._last_test_actions.view(waves, T, E, -1))      # [waves][T][E][N]
    want = torch.from_numpy(zc["test/draws/actions"]).argmax(-1).view(n_ep, T, -1)   # episode q = e * waves + w
    for e in range(E):
        for w in range(waves):
            assert torch.equal(got[w, :, e], want[e * waves + w]), (e, w)


def test_drivers_irdqn_block_runs_as_written():
    """The commented iRDQN block of xp_load.py:112-128 / xp_n_agents.py:116-132, uncommented, on the drivers' env shape
    (8 channels, homogeneous obs of 14 + 2 * 8 = 30 inputs, history_len = n_agents), a short run."""
    from algorithms.irdqn import iRDQN
    from envs.combinatorial_env import CombinatorialEnv
    n_agents = 6
    env = CombinatorialEnv(n_agents=n_agents, n_channels=8, deadlines=np.array([7, 14] * 3), lbdas=np.array([0.5] * 6),
                           period=np.array([2] * 6), arrival_probs=np.array([.2, .4, .8, 1, 1, 1]), offsets=np.zeros(6),
                           episode_length=12, traffic_model="heterogeneous", homogeneous_size=True,
                           periodic_devices=[0, 1, 2], channel_switch=np.full((6, 8), 0.3))
    idqn = iRDQN(
                env,
                history_len = n_agents,
                replay_start_size=100,
                replay_buffer_size=100000,
                gamma=0.4,
                update_target_frequency=100,
                minibatch_size=64,
                learning_rate=1e-4,
                update_frequency=1,
                initial_exploration_rate=1,
                final_exploration_rate=0.1,
                adam_epsilon=1e-8,
                loss='huber'
            )
    res = idqn.train(3)
    assert len(res) == 3 and len(res[0]) == 3 and len(res[1]) == 1 and idqn.n_updates == 0
    assert idqn.network.H == 100 and idqn.network.F == 30 and idqn.network.A == 8
    acts = idqn._act_ring[: 3 * 12].cpu().long()
    assert torch.all((acts == 1) | (acts == 2))                            # not training-ready: explore actions in {0, 1}
