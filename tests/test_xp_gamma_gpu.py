"""xp_gamma.py:33-81's construction and call sequence, end to end on the GPU, as tests/test_drivers_gpu.py does for
the other drivers: not a copy of the driver -- the calls it makes, in its order, with its keyword arguments and
input types, at a tiny iteration count.

  xp_gamma.py:33-54   ChannelSelectionEnv(5 agents, 16 channels, deadlines 7, lbdas 1 / 3.5, an ndarray
                      periodic_devices, channel_switch 0.8 x 17, 200-slot episodes)
  xp_gamma.py:69-81   iPPO(hidden_size=64, gamma, useRNN=True, history_len=10, early_stopping=True) ->
                      train(num_iter, n_epoch, num_episodes, test_freq) -> test(n)

24 inputs and 17 action ids: the GRU kernels' second action tile (csrc/gru_kernels.hip, AT = 2), not the torch
agent-stacked path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

n_agents, n_channels, load = 5, 16, 1 / 3.5


def xp_gamma_env(**kw):
    from envs.channel_selection_env import ChannelSelectionEnv
    deadlines = np.array([7] * n_agents)
    channel_switch = np.array([0.8 for _ in range(n_channels + 1)])
    lbdas = np.array([load for _ in range(n_agents)])
    period = np.array([7 for _ in range(n_agents)])
    arrival_probs = np.array([1 for _ in range(n_agents)])
    offsets = np.array([0, 2, 4, 0, 2])
    periodic_devices = np.array([2, 4])
    return ChannelSelectionEnv(n_agents=n_agents, n_channels=n_channels, deadlines=deadlines, period=period,
                               lbdas=lbdas, episode_length=200, traffic_model="aperiodic",
                               arrival_probs=arrival_probs, periodic_devices=periodic_devices, offsets=offsets,
                               channel_switch=channel_switch, verbose=False, **kw)


def xp_gamma_learner(env):
    from algorithms.ippo import iPPO
    return iPPO(env, hidden_size=64, gamma=0.4, policy_lr=3e-4, value_lr=1e-2, device=None, useRNN=True,
                history_len=10, early_stopping=True)


def test_xp_gamma_sequence():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    np.random.seed(42)
    env = xp_gamma_env()
    assert env.observation_space[0].shape[0] == 24
    ippo = xp_gamma_learner(env)
    assert ippo.policy.A == 17 and ippo.policy.F == 24
    assert ippo._gru_ok() and ippo._fused_update_ok()
    assert not ippo._record_ok()
    res = ippo.train(num_iter=1, n_epoch=2, num_episodes=2, test_freq=1)
    assert all(np.isfinite(np.asarray(res[2], dtype=np.float64)).reshape(-1))
    assert all(np.isfinite(np.asarray(res[3], dtype=np.float64)).reshape(-1))
    score_ppo, jains_ppo, channel_error_ppo, rewards_ppo = ippo.test(5)
    assert 0.0 <= score_ppo <= 1.0 and channel_error_ppo == 0
    assert len(res[0]) == 2 and 1 <= len(res[1]) <= 2 and len(res[2]) == len(res[3]) == len(res[1])
    for s in list(res[0]) + list(res[1]):
        assert 0.0 <= float(s) <= 1.0


def test_xp_gamma_graph_rollout_equals_eager():
    """the HIP-graph rollout of this learner at 40 envs (captured once, replayed) reproduces the eager slot loop bit
    for bit over consecutive rollouts: obs, ids in 0..16, log-probs, values, rewards, episode statistics"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    outs = []
    for graph in (False, True):
        torch.manual_seed(0)
        lr = xp_gamma_learner(xp_gamma_env(n_envs=40, device="cuda", seed=3))
        assert lr._gru_ok() and lr._fused_update_ok()
        lr.graph_rollout = graph
        res = []
        for _ in range(2):     # capture on the first, replay after (buffers are reused)
            ro = lr._rollout(40)
            res.append((ro.obs_f32.clone(), ro.actions.clone(), ro.logp.clone(), ro.rewards.clone(),
                        None if ro.values is None else ro.values.clone(), list(ro.scores), list(ro.ep_rewards)))
        outs.append(res)
        if graph:
            assert getattr(lr, "_rollout_graphs", None), "graph path not taken"
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            if x is None:
                assert y is None
            elif isinstance(x, list):
                assert x == y
            else:
                assert torch.equal(x, y)
    acts = outs[1][0][1]
    assert int(acts.max()) <= 16 and int(acts.max()) >= 16, "no id of the second tile in 16,000 draws"
    assert not torch.equal(outs[1][0][1], outs[1][1][1])
