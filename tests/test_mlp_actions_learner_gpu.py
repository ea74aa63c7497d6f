"""iPPO(env) and D2DPPO(env) with default arguments (useRNN=False, hidden_size 128) on xp_gamma.py's env -- 5 agents
x 16 channels, 17 ids, 24 inputs --: the shape whose default learner ran on the torch agent-stacked path until
csrc/mlp_actions_kernels.hip.  As a user gets them they must take the new policy and update kernels (fp32 rows: no
record for this head), capture the rollout in a HIP graph and replay it with the eager loop's bits, train one
iteration with finite losses, agree to 1e-5 in their log-probs (iPPO: and values) with the same weights under
D2D_FUSED_POLICY=0 D2D_FUSED_UPDATE=0, and run test().  The reference traces learner_ippo_mlp_cat16_h64 /
learner_d2d_mlp_cat16_h128 of tests/test_learner_gpu.py hold the same path to the reference's numbers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, C, E = 5, 16, 10


def make_env(seed=3):
    from envs.channel_selection_env import ChannelSelectionEnv
    # xp_gamma.py:33-54 on 10 parallel envs, episodes of 20 slots
    return ChannelSelectionEnv(n_agents=N, n_channels=C, deadlines=np.array([7] * N), period=np.array([7] * N),
                               lbdas=np.array([1 / 3.5] * N), episode_length=20, traffic_model="aperiodic",
                               arrival_probs=np.array([1] * N), periodic_devices=np.array([2, 4]),
                               offsets=np.array([0, 2, 4, 0, 2]), channel_switch=np.array([0.8] * (C + 1)),
                               verbose=False, n_envs=E, device="cuda", seed=seed)


def make_learner(algo="ippo"):
    from algorithms.d2d_ppo import D2DPPO
    from algorithms.ippo import iPPO
    torch.manual_seed(0)
    cls = iPPO if algo == "ippo" else D2DPPO
    return cls(make_env(), device="cuda", early_stopping=False)      # useRNN, hidden_size: the defaults


@pytest.mark.parametrize("algo", ["ippo", "d2d"])
def test_default_learner_takes_the_new_kernels(algo):
    from d2dhip import _lib
    lr = make_learner(algo)
    p = lr.policy
    assert not lr.useRNN and (p.H, p.F, p.A) == (128, 24, 17) and _lib.mlp_actions(p.F, p.H, p.A, 1)
    names = [_lib.mlp_entry(_lib.load(), w, p.F, p.H, True, p.A, 1)[1] for w in ("policy", "workspace", "actor_grad")]
    assert names == ["d2d_policy_mlp_actions_step", "d2d_ppo_actions_workspace", "d2d_ppo_actor_grad_actions"]
    assert lr._fused_ok() and lr._fused_update_ok() and not lr._record_ok()
    if algo == "ippo":
        assert lr._defer_values_ok()
    ro = lr._rollout(2 * E)
    assert torch.is_tensor(ro.obs) and ro.obs.dtype == torch.float32, "fp32 rows"
    assert ro.actions.dtype == torch.uint8 and int(ro.actions.max()) <= C
    assert int(ro.actions.max()) == C, "an id of the second tile is drawn in 2,000 draws"
    res = lr.test(4)
    assert len(res) == 4 and all(np.isfinite(float(v)) for v in res)


@pytest.mark.parametrize("algo", ["ippo", "d2d"])
def test_rollout_graph_replays_the_eager_bits(algo):
    outs = []
    for graph in (False, True):
        lr = make_learner(algo)
        lr.graph_rollout = graph
        res = []
        for _ in range(3):      # 2 waves each; capture on the first, replay after
            ro = lr._rollout(2 * E)
            out = [ro.obs_f32.clone(), ro.actions.clone(), ro.logp.clone(), ro.rewards.clone(), list(ro.scores)]
            if algo == "ippo":
                out.append(ro.values.clone())
            res.append(out)
        outs.append(res)
        assert bool(getattr(lr, "_rollout_graphs", None)) == graph, "graph path taken exactly when asked"
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            assert x == y if isinstance(x, list) else torch.equal(x, y)
    assert not torch.equal(outs[1][1][1], outs[1][2][1]), "consecutive rollouts draw fresh actions"


@pytest.mark.parametrize("algo", ["ippo", "d2d"])
def test_train_iteration_and_torch_path_parity(algo, monkeypatch):
    lr = make_learner(algo)
    ro = lr._rollout(2 * E)
    assert ro.logp.shape == (ro.T, N, E) and bool(torch.isfinite(ro.logp).all())
    # the same learner on the torch agent-stacked path (what this shape ran on before), same weights
    monkeypatch.setenv("D2D_FUSED_POLICY", "0")
    monkeypatch.setenv("D2D_FUSED_UPDATE", "0")
    lt = make_learner(algo)
    assert not lt._fused_ok() and not lt._fused_update_ok() and not lt._record_ok()
    for a, b in zip(lr.agents, lt.agents):
        b.policy_network.load_state_dict(a.policy_network.state_dict())
        if algo == "ippo":
            b.value_network.load_state_dict(a.value_network.state_dict())
    worst_lp = worst_v = 0.0
    with torch.no_grad():
        for i in range(ro.T):
            x = ro.obs_f32[i].transpose(0, 1)                                   # [N][E][F]
            acts = ro.actions[i].transpose(0, 1).long()                         # [N][E] ids
            _, lp, v = lt._act(x, True, algo == "ippo", forced=acts)
            worst_lp = max(worst_lp, (lp - ro.logp[i]).abs().max().item())
            if algo == "ippo":
                worst_v = max(worst_v, (v - ro.values[i]).abs().max().item())
    print(f"{algo}: kernels against the torch path over {ro.T} slots: log-prob {worst_lp:.2e}, value {worst_v:.2e}")
    assert worst_lp <= 1e-5 and worst_v <= 1e-5
    monkeypatch.delenv("D2D_FUSED_POLICY")
    monkeypatch.delenv("D2D_FUSED_UPDATE")
    # one training iteration as the user runs it (graph rollout, deferred values / the forced pass and the chain)
    scores, tests, pl, vl = lr.train(1, n_epoch=2, num_episodes=2 * E, test_freq=10 ** 9)
    def flat(v):        # the losses come as floats, device scalars or per-agent lists of them
        if torch.is_tensor(v):
            return [float(x) for x in v.detach().cpu().reshape(-1)]
        if isinstance(v, (list, tuple, np.ndarray)):
            return [x for q in v for x in flat(q)]
        return [float(v)]
    assert len(flat(pl)) >= 2 and len(flat(vl)) == 2
    assert np.isfinite(flat(pl)).all() and np.isfinite(flat(vl)).all()
    for ag in lr.agents:
        for t in ag.policy_network.state_dict().values():
            assert bool(torch.isfinite(t).all())
