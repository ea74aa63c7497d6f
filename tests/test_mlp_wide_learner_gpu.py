"""The learners at their default hidden_size 128 on the 16-channel combinatorial env of run_ippo_combinatorial.py
(6 agents, deadlines 7 / 14: 39 / 46 inputs): the shape that ran on the torch agent-stacked path until the wide MLP
kernels (csrc/mlp_wide_kernels.hip).  iPPO(env) as a user gets it must take the compact record (64-byte rows), the
wide policy and update kernels, capture its rollout in a HIP graph and replay it with the eager loop's bits, train
with finite losses, and agree to 1e-5 in its log-probs and values with the same learner built under
D2D_FUSED_POLICY=0 D2D_FUSED_UPDATE=0.  The reference traces learner_*_mlp_comb16_h128 / _h100 / _cat15_h80 of
tests/test_learner_gpu.py hold the same path to the reference's numbers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, C, E = 6, 16, 10


def make_env(seed=3):
    from envs.combinatorial_env import CombinatorialEnv
    # run_ippo_combinatorial.py:29-76 at load 1 on 10 parallel envs
    return CombinatorialEnv(N, C, np.array([7, 14] * 3), np.full(N, 1.0), period=np.full(N, 1.0),
                            arrival_probs=np.array([0.4, 0.8] * 3), offsets=np.zeros(N), episode_length=20,
                            traffic_model="heterogeneous", periodic_devices=[0, 1],
                            channel_switch=np.full(C, 0.8), n_envs=E, device="cuda", seed=seed)


def make_learner(algo="ippo"):
    from algorithms.d2d_ppo import D2DPPO
    from algorithms.ippo import iPPO
    torch.manual_seed(0)
    env = make_env()
    cls = iPPO if algo == "ippo" else D2DPPO
    return cls(env, device="cuda", combinatorial=True, early_stopping=False)      # hidden_size: the default


@pytest.mark.parametrize("algo", ["ippo", "d2d"])
def test_default_learner_takes_the_wide_kernels(algo):
    from d2dhip import _lib
    from d2dhip.record import ObsRecord
    lr = make_learner(algo)
    p = lr.policy
    assert (p.H, p.F, p.A) == (128, 46, 16) and _lib.mlp_wide(p.F, p.H)
    assert _lib.mlp_entry(_lib.load(), "policy", p.F, p.H)[1] == "d2d_policy_mlp_wide_step"
    assert lr._fused_ok() and lr._fused_update_ok() and lr._record_ok()
    if algo == "ippo":
        assert lr._defer_values_ok()
    ro = lr._rollout(2 * E)
    assert isinstance(ro.obs, ObsRecord) and ro.obs.data.shape[-1] == 64, "the 64-byte record"


def test_rollout_graph_replays_the_eager_bits():
    outs = []
    for graph in (False, True):
        lr = make_learner()
        lr.graph_rollout = graph
        res = []
        for _ in range(3):      # 2 waves each; capture on the first, replay after
            ro = lr._rollout(2 * E)
            res.append((ro.obs_f32.clone(), ro.actions.clone(), ro.logp.clone(), ro.rewards.clone(), ro.values.clone(),
                        list(ro.scores)))
        outs.append(res)
        assert bool(getattr(lr, "_rollout_graphs", None)) == graph, "graph path taken exactly when asked"
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert x == y if isinstance(x, list) else torch.equal(x, y)
    assert not torch.equal(outs[1][1][1], outs[1][2][1]), "consecutive rollouts draw fresh actions"


def test_train_iteration_and_torch_path_parity(monkeypatch):
    from algorithms._core import unpack_actions
    lr = make_learner()
    ro = lr._rollout(2 * E)
    assert ro.logp.shape == (ro.T, N, E) and ro.values.shape == (ro.T, N, E)
    assert bool(torch.isfinite(ro.logp).all()) and bool(torch.isfinite(ro.values).all())
    # the same learner on the torch agent-stacked path (what these shapes ran on before), same weights
    monkeypatch.setenv("D2D_FUSED_POLICY", "0")
    monkeypatch.setenv("D2D_FUSED_UPDATE", "0")
    lt = make_learner()
    assert not lt._fused_ok() and not lt._fused_update_ok() and not lt._record_ok()
    for a, b in zip(lr.agents, lt.agents):
        b.policy_network.load_state_dict(a.policy_network.state_dict())
        b.value_network.load_state_dict(a.value_network.state_dict())
    worst_lp = worst_v = 0.0
    with torch.no_grad():
        for i in range(ro.T):
            x = ro.obs_f32[i].transpose(0, 1)                                   # [N][E][F]
            acts = unpack_actions(ro.actions[i], C).transpose(0, 1)             # [N][E][C]
            _, lp, v = lt._act(x, True, True, forced=acts)
            worst_lp = max(worst_lp, (lp - ro.logp[i]).abs().max().item())
            worst_v = max(worst_v, (v - ro.values[i]).abs().max().item())
    print(f"wide kernels against the torch path over {ro.T} slots: log-prob {worst_lp:.2e}, value {worst_v:.2e}")
    assert worst_lp <= 1e-5 and worst_v <= 1e-5
    monkeypatch.delenv("D2D_FUSED_POLICY")
    monkeypatch.delenv("D2D_FUSED_UPDATE")
    # one training iteration as the user runs it (graph rollout, deferred values, the wide update kernels)
    scores, tests, pl, vl = lr.train(1, n_epoch=2, num_episodes=2 * E, test_freq=10 ** 9)
    assert len(pl) == 2 and len(vl) == 2
    assert all(np.isfinite(pl)) and all(np.isfinite(vl))
    for ag in lr.agents:
        for t in list(ag.policy_network.state_dict().values()) + list(ag.value_network.state_dict().values()):
            assert bool(torch.isfinite(t).all())
