"""Host-side checks of iRDQN (algorithms/irdqn.py, d2dhip/rdqn.py) that need no GPU: the C ABI's argument checks,
the reference-compatible ReplayBuffer, the epsilon / update / target-sync / test schedule of the train loop
(/root/reference/algorithms/irdqn.py:230-300) with the kernels stubbed, and the loud no-GPU error."""
import ctypes
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_abi_argument_checks():
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    assert ctypes.sizeof(_lib.RdqnDesc) == 8 * 4 + 10 * 8 + 2 * 8 + 8
    w = ctypes.c_void_p(16)
    q = lambda d, B=1, shift=0, mode=0, eps=0.0, em=None: lib.d2d_rdqn_q(  # noqa: E731
        None if d is None else ctypes.byref(d), w, w, B, shift, mode, eps, None, 1, em, em, 0, w, None, w, None)
    mk = lambda F=12, H=100, A=4, rows=14, ep=0: _lib.RdqnDesc(2, 3, F, H, A, rows, ep, 0, *([w] * 10), 0, 0, None)  # noqa
    assert q(None) == -1 and b"NULL desc" in lib.d2d_last_error()
    for bad in (mk(H=144), mk(F=64), mk(A=17)):
        assert q(bad) == -2 and b"hidden <= 128, obs_dim + 1 <= 64, n_out <= 16" in lib.d2d_last_error()
    assert q(mk(rows=15, ep=6)) == -1 and b"whole episodes" in lib.d2d_last_error()
    assert q(mk(), shift=2) == -1
    assert q(mk(), mode=3) == -1 and b"mode" in lib.d2d_last_error()
    assert q(mk(), mode=_lib.D2D_RDQN_FORCED) == -1 and b"explore_mask" in lib.d2d_last_error()
    assert q(mk(), mode=_lib.D2D_RDQN_EPS, eps=1.5) == -1 and b"eps" in lib.d2d_last_error()
    assert q(mk(), B=0) == 0                                             # nothing to do: no launch
    # workspace: x [L][Bp][IW] + h [L + 1][Bp][HW] + gates [L][Bp][4 HW] + four head images + dq + tile losses
    d, N, L, Bp, HW, IW = mk(), 2, 5, 48, 112, 16
    want = N * (L * Bp * IW + (L + 1) * Bp * HW + L * Bp * 4 * HW + 4 * Bp * HW + Bp * 16 + Bp // 16)
    assert lib.d2d_rdqn_grad_workspace(ctypes.byref(d), 33, L) == want
    assert lib.d2d_rdqn_grad_workspace(ctypes.byref(d), 33, 257) == -1
    g = lambda d, L, ws: lib.d2d_rdqn_grad(ctypes.byref(d), w, w, 33, L, w, w, w, w, 0.4, 0, *([w] * 12), ws, None)  # noqa
    assert g(d, 257, want) == -2 and b"window lengths" in lib.d2d_last_error()
    assert g(d, L, want - 1) == -1 and b"d2d_rdqn_grad_workspace" in lib.d2d_last_error()
    assert g(mk(H=129), L, want) == -2


def test_python_envelope_and_loss_checks():
    from d2dhip import rdqn
    rdqn.check_envelope(63, 128, 16, 256)
    for bad in ((64, 100, 4, 5), (12, 144, 4, 5), (12, 100, 17, 5), (12, 100, 4, 257)):
        with pytest.raises(NotImplementedError, match="hidden <= 128"):
            rdqn.check_envelope(*bad)
    assert rdqn.mask_dtype(8) == torch.uint8 and rdqn.mask_dtype(9) == torch.int16


def test_replay_buffer_matches_the_reference_semantics():
    from algorithms.irdqn import ReplayBuffer
    N, F, B, L = 3, 4, 5, 3
    rb = ReplayBuffer(10, "cpu")
    rng = np.random.default_rng(0)
    rows = []
    for t in range(14):                                                   # 14 adds into a 10-deep deque
        tr = (torch.full((N, F), float(t)), rng.integers(0, 2, N), rng.normal(size=N), torch.full((N, F), t + 1.0),
              t % 7 == 6)
        rows.append(tr)
        rb.add(tr)
    assert len(rb) == 10 and rb.buffer_limit == 10
    kept = rows[4:]
    np.random.seed(3)
    s, a, r, sn, d = rb.sample_chunk(B, L)
    np.random.seed(3)
    starts = np.random.randint(0, 10 - L, B)                              # irdqn.py:25: never the newest as a last
    assert starts.max() + L - 1 < 9 + 1 and s.shape == (B, L, N, F) and sn.shape == (B, L, N, F)
    assert (a.shape, r.shape, d.shape) == ((B, L, N), (B, L, N), (B, L, 1))
    assert (s.dtype, a.dtype, r.dtype, d.dtype) == (torch.float32, torch.int64, torch.float32, torch.float32)
    for i, st in enumerate(starts):
        for j in range(L):
            tr = kept[st + j]
            assert torch.equal(s[i, j], tr[0]) and torch.equal(sn[i, j], tr[3])
            assert np.array_equal(a[i, j].numpy(), tr[1]) and float(d[i, j, 0]) == float(tr[4])
            assert np.allclose(r[i, j].numpy(), tr[2].astype(np.float32))
    rb.reset()
    assert len(rb) == 0


def reference_schedule(n_episodes, replay_start_size, update_frequency, update_target_frequency, initial, final):
    """The reference's train loop (irdqn.py:230-300) reduced to its schedule: per episode the epsilon each slot's
    act() sees, and the end-of-episode events in order."""
    eps_attr, out = None, []
    for ep in range(n_episodes):
        ready = ep >= replay_start_size
        seen = []
        for t in range(3):                                                # slots of the episode
            seen.append(eps_attr)                                         # act() reads self.epsilon ...
            e = initial - (initial - final) * (ep / 1000)                 # ... then update_epsilon(ep)
            eps_attr = max(e, final)
        ev = []
        if ep % 100 == 0:
            ev.append(("test", ep))
        if ready and ep % update_frequency == 0:
            ev.append(("update", ep))
            if ep % update_target_frequency == 0:
                ev.append(("sync", ep))
        out.append((ready, seen, ev))
    return out


def test_epsilon_and_event_schedule():
    from algorithms.irdqn import episode_plan, wave_events
    kw = dict(replay_start_size=2, update_frequency=1, update_target_frequency=2, initial=1.0, final=0.1)
    ref = reference_schedule(6, **kw)
    for ep, (ready, seen, ev) in enumerate(ref):
        p = episode_plan(ep, **kw)
        assert p["ready"] == ready
        if ep > 0:
            assert p["eps_first"] == seen[0]
        else:
            assert seen[0] is None and p["eps_first"] == 1.0              # the reference has no epsilon yet (documented)
        assert p["eps"] == seen[1] == seen[2]
        assert wave_events(ep, 1, 6, **kw) == ev
    assert [e for _, _, ev in ref for e in ev] == [("test", 0), ("update", 2), ("sync", 2), ("update", 3),
                                                   ("update", 4), ("sync", 4), ("update", 5)]
    # E = 4: a wave runs the events of its episodes in order; episodes past n_episodes have none
    assert wave_events(0, 4, 6, **kw) == [("test", 0), ("update", 2), ("sync", 2), ("update", 3)]
    assert wave_events(4, 4, 6, **kw) == [("update", 4), ("sync", 4), ("update", 5)]
    # epsilon: linear over 1000 episodes, then flat; update_frequency thins the updates
    assert episode_plan(500, **kw)["eps"] == pytest.approx(0.55) and episode_plan(5000, **kw)["eps"] == 0.1
    kw["update_frequency"] = 3
    assert [e for ep in range(8) for e in wave_events(ep, 1, 8, **kw)] == [
        ("test", 0), ("update", 3), ("update", 6), ("sync", 6)]


@pytest.mark.parametrize("E", [1, 4])
def test_train_loop_order_with_stubbed_kernels(E):
    """iRDQN.train's host logic on stubs: waves of E episodes, then the reference's events in order."""
    from algorithms.irdqn import iRDQN
    L = iRDQN.__new__(iRDQN)
    L.replay_start_size, L.update_frequency, L.update_target_frequency = 2, 1, 2
    L.initial_exploration_rate, L.final_exploration_rate = 1.0, 0.1
    log = []
    batch = types.SimpleNamespace(E=E, spec=types.SimpleNamespace(arrival_kinds=lambda: None))
    L._bind_env = lambda: batch
    L._alloc_ring = lambda b, n_waves: log.append(("alloc", n_waves))
    L._train_wave = lambda b, ep0: (log.append(("wave", ep0)) or ([0.5 + e for e in range(E)], [1.0] * E))
    L._update = lambda n: log.append(("update",))
    L._sync_target = lambda: log.append(("sync",))
    L.test = lambda n: (log.append(("test", n)) or (0.25, 3.0))
    scores, tests, rewards = L.train(6)
    assert len(scores) == 6 and tests == [0.25] and rewards == [3.0]
    if E == 1:
        assert log == [("alloc", 6), ("wave", 0), ("test", 50), ("wave", 1), ("wave", 2), ("update",), ("sync",),
                       ("wave", 3), ("update",), ("wave", 4), ("update",), ("sync",), ("wave", 5), ("update",)]
    else:
        assert log == [("alloc", 2), ("wave", 0), ("test", 50), ("update",), ("sync",), ("update",),
                       ("wave", 4), ("update",), ("sync",), ("update",)]
        assert scores == [0.5, 1.5, 2.5, 3.5, 0.5, 1.5]
    # early stopping: a test score of 1 ends training after that episode, before its update
    log.clear()
    L.replay_start_size = 0
    L.test = lambda n: (1, 9.0)
    scores, tests, _ = L.train(6)
    assert tests == [1] and len(scores) == 1 and ("update",) not in log


def test_constructing_without_a_gpu_raises_the_require_gpu_error():
    import d2dhip
    from algorithms.irdqn import iRDQN, DQN, RNN, ReplayBuffer, Transition  # noqa: F401  (the reference's names)
    from envs.combinatorial_env import CombinatorialEnv
    env = CombinatorialEnv(2, 2, np.array([3, 3]), np.ones(2), episode_length=6)
    if torch.cuda.is_available():
        assert iRDQN(env, history_len=3).n_agents == 2
        return
    with pytest.raises(d2dhip.D2DHipError, match="no CPU fallback"):
        iRDQN(env)
    with pytest.raises(NotImplementedError, match="callable"):
        DQN(env, loss=lambda a, b, reduction: 0)


def test_rnn_module_matches_torch_gru():
    """The per-agent RNN (irdqn.py:58-86) computes what torch.nn.GRU + the Sequential head compute, for (L, in) and
    (B, L, in) inputs."""
    from algorithms.irdqn import RNN
    torch.manual_seed(0)
    m = RNN(7, 4)
    assert m.hidden_size == 100 and [type(x).__name__ for x in m.layers] == ["Linear", "ReLU"] * 2 + ["Linear"]
    x = torch.randn(3, 5, 7)
    with torch.no_grad():
        want = m.layers(m.lstm(x.permute(1, 0, 2))[0][-1])
        torch.testing.assert_close(m(x), want, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(m(x[0]), want[:1], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("loss", ["huber", "mse"])
def test_float64_oracle_reproduces_the_reference_fixtures(loss):
    """The float64 oracle the GPU tests use (tests/irdqn_oracle.py) against the reference's recorded updates
    (tools/gen_irdqn_fixtures.py: DQN.train_step in float64 on ReplayBuffer.sample_chunk's minibatches): losses, deltas
    and gradients to 1e-9 relative, the weights after K Adam steps to the fixtures' float32 rounding."""
    import irdqn_oracle as O
    zc, z, cfg = O.load_case(loss)
    N = cfg["env"]["n_agents"]
    # the oracle's GRU is torch.nn.GRU's: agent 0's hidden state through the module itself
    p = O.stacked(zc, "weights/agent{}/network", N)
    st = O.chunk_batch(zc, z["upd/0/starts"], cfg["learner"]["history_len"], cfg["learner"]["replay_buffer_size"])[0]
    gru = torch.nn.GRU(st.shape[-1], 100).double()
    with torch.no_grad():
        for n, k in (("weight_ih_l0", "w_ih"), ("weight_hh_l0", "w_hh"), ("bias_ih_l0", "b_ih"), ("bias_hh_l0", "b_hh")):
            getattr(gru, n).copy_(p[k][0])
        h = gru(st[0].permute(1, 0, 2))[0][-1]
        y = torch.relu(h @ p["w1"][0].t() + p["b1"][0])
        y = torch.relu(y @ p["w2"][0].t() + p["b2"][0])
        torch.testing.assert_close(O.net_q(p, st)[0], y @ p["w3"][0].t() + p["b3"][0], rtol=1e-12, atol=1e-12)
    steps, final = O.trajectory(zc, z, cfg, loss)
    assert len(steps) == 3
    for u, s in enumerate(steps):
        for i in range(N):
            want = float(z[f"upd/{u}/agent{i}/loss"])
            assert abs(s["loss"][i].item() - want) <= 1e-9 * abs(want), (u, i)
            np.testing.assert_allclose(s["delta"][i].numpy(), z[f"upd/{u}/agent{i}/delta"], rtol=1e-9, atol=1e-12)
            for k, sd in O.SD_NAMES.items():
                g = s["grads"][k][i].numpy()
                cs = np.array([g.sum(), np.abs(g).sum(), np.abs(g).max()])
                np.testing.assert_allclose(cs, z[f"upd/{u}/agent{i}/gradsum/{sd}"], rtol=1e-9,
                                           atol=1e-9 * np.abs(g).sum())
        if loss == "huber":                                               # both branches of the loss in every minibatch
            assert (s["delta"].abs() < 1).any(1).all() and (s["delta"].abs() > 1).any(1).all()
    for k, sd in O.SD_NAMES.items():                                      # the first update's gradients, element-wise
        want = z[f"upd/0/agent0/grad/{sd}"]
        got = steps[0]["grads"][k][0].numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), k
        for i in range(N):
            np.testing.assert_allclose(final[k][i].numpy(), z[f"weights_after/agent{i}/{sd}"], rtol=0, atol=2e-7)
    assert zc["test/gaps"].min() >= 1e-3                                  # every recorded greedy decision is clear


def test_fixture_files_are_data_only():
    import irdqn_oracle as O
    import os
    from conftest import GOLDEN
    for name in ("common", "huber", "mse"):
        path = os.path.join(GOLDEN, f"irdqn_{name}.npz")
        assert os.path.getsize(path) < (1 << 20)
        z = np.load(path, allow_pickle=False)
        assert all(z[k].dtype.kind in "fiubU" for k in z.files)
    zc, _, cfg = O.load_case("huber")
    assert cfg["learner"]["history_len"] == 5 and cfg["learner"]["gamma"] == 0.4 and cfg["env"]["n_channels"] == 4
