"""The learners on the fused optimizer (fused_optimizer=True: d2dhip.optim.StackedAdam / d2d_adam_step) against the
same learners on torch's Adam, and one reference trace replayed on it (pytest -m gpu).

Two learners are built from one seed and trained on the same random streams.  Until the first optimizer step nothing
differs, so the first rollout and (on the HIP gradient kernels) the first step's gradients are bit-equal.

The optimizer's arithmetic over the whole run -- 2 iterations of 2 epochs, iRDQN: 3 updates -- is held to the K-step
rule of tests/test_optim_gpu.py with each learner replayed in float64 on ITS OWN recorded gradients (the fused learner's
with its clip at 20 inside the replay, the torch learner's as they enter torch's Adam):
    |p_hip - p64_own| <= 4 max|p_torch - p64_torch| + u max|p|      per element, after the first step and after the last.
After the first step the two learners compute their gradients at weights one rounding apart, and Adam divides every
element by its own gradient history, so a replay of the OTHER learner's gradients bounds a learner only for the step they
share: that ratio is printed (1.7-2.0 for policy stacks), and the two learners' weights are compared with the existing
Adam-aware bound -- test_learner_gpu's ref_adam_tolerance and assert_weights_close, imported, the torch learner's
recorded gradients as the reference.

The D2D setups start from a central critic whose output layer is scaled by 30, so that its gradient norm is over the
clip at 20 (asserted): .grad after the step must then hold a gradient that the clip changed.  Two setups run the torch
epoch (the learners' path when the HIP update kernels do not apply): zero_grad, backward into freshly allocated .grad
tensors, step."""
import os

import numpy as np
import pytest

import optim_oracle as O
from conftest import GOLDEN
from test_learner_gpu import _nets, _sd, assert_weights_close, build, ref_adam_tolerance, ref_grads

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class StepLog:
    """Per optimizer.step: the gradients going in, the gradients left in .grad and the parameters coming out."""

    def __init__(self, opt, params, names):
        self.params, self.names = list(params), list(names)
        self.init = [p.detach().clone() for p in self.params]
        self.g_in, self.g_out, self.p_out = [], [], []
        step = opt.step

        def rec(*a, **kw):
            self.g_in.append([p.grad.detach().clone() for p in self.params])
            out = step(*a, **kw)
            self.g_out.append([p.grad.detach().clone() for p in self.params])
            self.p_out.append([p.detach().clone() for p in self.params])
            return out
        opt.step = rec


def _optimizers(ln, algo):
    """[(label, optimizer, params, names, n_agents, lr, eps)]"""
    if algo == "irdqn":
        pp = ln.network.params
        return [("q", ln.optimizer, pp.values(), pp.keys(), ln.n_agents, ln.learning_rate, ln.adam_epsilon)]
    pp = ln.policy.params
    out = [("policy", ln.policy_optimizer, pp.values(), pp.keys(), ln.n_agents, 3e-3, 1e-8)]
    if algo == "ippo":
        vp = ln.value.params
        out.append(("value", ln.value_optimizer, vp.values(), vp.keys(), ln.n_agents, 1e-2, 1e-8))
    else:
        named = list(ln.value_network.named_parameters())
        out.append(("critic", ln.value_optimizer, [p for _, p in named], [n for n, _ in named], 1, 1e-2, 1e-8))
    return out


def _make(setup, fused):
    """A learner of `setup` from seed 0 at n_envs = 2."""
    torch.manual_seed(0)
    np.random.seed(0)
    kw = {} if fused is None else {"fused_optimizer": fused}
    if setup == "irdqn":
        from algorithms.irdqn import iRDQN
        from envs.combinatorial_env import CombinatorialEnv
        env = CombinatorialEnv(4, 2, np.array([3] * 4), np.ones(4) * 0.7, episode_length=6, n_envs=2, device="cuda:0",
                               seed=3)
        return iRDQN(env, history_len=3, replay_start_size=2, replay_buffer_size=10 ** 4, gamma=0.4,
                     update_target_frequency=2, minibatch_size=8, learning_rate=1e-3, **kw), "irdqn"
    torch_epoch = setup.endswith("_torch")
    fixture, hidden = {"ippo_mlp": ("ippo_mlp_comb", None), "d2d_mlp": ("d2d_mlp_comb", None),
                       "d2d_gru": ("d2d_rnn_comb", 16)}[setup[:-len("_torch")] if torch_epoch else setup]
    z = np.load(os.path.join(GOLDEN, f"learner_{fixture}.npz"))
    env, kind, common, iPPO, D2DPPO = build(z, n_envs=2)
    assert env.n_agents == 6 and kind == "comb"
    if hidden is not None:
        common["hidden_size"] = hidden
    algo = fixture.split("_")[0]
    ln = iPPO(env, **common, **kw) if algo == "ippo" else D2DPPO(env, beta_entropy=0.02, **common, **kw)
    if torch_epoch:
        ln._fused_upd = False              # the torch epoch, as D2D_FUSED_UPDATE=0 selects it
    if algo == "d2d":
        with torch.no_grad():              # a critic far from its targets: its gradient norm is over the clip at 20
            ln.value_network.linear2.weight.mul_(30.0)
            ln.value_network.linear2.bias.mul_(30.0)
    return ln, algo


def _train(ln, algo):
    np.random.seed(21)
    torch.manual_seed(21)
    if algo == "irdqn":
        ln.test = lambda n_episodes, verbose=False: (0.5, 1.0)
        ln.train(5, early_stopping=False)
        assert ln.n_updates == 3
    else:
        ln.test = lambda num_episodes: (0.5, 1.0, 0, 0.0)
        ln.train(2, n_epoch=2, num_episodes=2, test_freq=10 ** 9)


SETUPS = ["ippo_mlp", "d2d_mlp", "d2d_gru", "irdqn", "ippo_mlp_torch", "d2d_mlp_torch"]


@pytest.mark.parametrize("setup", SETUPS)
def test_fused_optimizer_learner_follows_the_torch_learner(setup):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    from d2dhip.optim import StackedAdam
    lt, algo = _make(setup, False)
    lh, _ = _make(setup, True)
    opts_t, opts_h = _optimizers(lt, algo), _optimizers(lh, algo)
    for (_, ot, *_), (_, oh, *_) in zip(opts_t, opts_h):
        assert isinstance(ot, torch.optim.Adam) and isinstance(oh, StackedAdam)
    for (_, _, pt, *_), (_, _, ph, *_) in zip(opts_t, opts_h):
        assert all(torch.equal(a, b) for a, b in zip(pt, ph)), "one seed, one initialisation"
    if algo != "irdqn":
        # the first rollout, before any optimizer step: bit-equal
        env_t, env_h = lt.env, lh.env
        np.random.seed(20)
        torch.manual_seed(20)
        ro_t = lt._rollout(2)
        np.random.seed(20)
        torch.manual_seed(20)
        ro_h = lh._rollout(2)
        for name in ("actions", "logp", "rewards"):
            assert torch.equal(getattr(ro_t, name), getattr(ro_h, name)), name
        assert ro_t.scores == ro_h.scores and env_t is not env_h
    logs_t = [StepLog(o, p, n) for _, o, p, n, *_ in opts_t]
    logs_h = [StepLog(o, p, n) for _, o, p, n, *_ in opts_h]
    pre_clip = []
    if algo == "d2d":   # the torch learner's policy gradients before grad_norm_clip_(20)
        clip = lt.policy.grad_norm_clip_
        lt.policy.grad_norm_clip_ = lambda mx: (pre_clip.append([p.grad.detach().clone() for p in logs_t[0].params]),
                                                clip(mx))[1]
    _train(lt, algo)
    _train(lh, algo)
    torch_epoch = setup.endswith("_torch")
    if algo != "irdqn":    # which epoch ran: the HIP update kernels, or the torch epoch of the *_torch setups
        assert bool(lt._fused_update_ok()) is not torch_epoch and bool(lh._fused_update_ok()) is not torch_epoch

    def replay(lg, N, lr_, eps, max_norm, K):
        p64, m64 = [x.double() for x in lg.init], [torch.zeros_like(x).double() for x in lg.init]
        v64 = [x.clone() for x in m64]
        for t in range(1, K + 1):
            r = O.clip_adam64(p64, lg.g_in[t - 1], m64, v64, N, t, lr=lr_, eps=eps, max_norm=max_norm)
            p64, m64, v64 = r["p"], r["m"], r["v"]
        return p64

    for (label, _, _, names, N, lr_, eps), lg_t, lg_h in zip(opts_t, logs_t, logs_h):
        K = len(lg_t.g_in)
        assert K == len(lg_h.g_in) and K >= (3 if algo == "irdqn" else 4), (label, K)
        clipped = algo == "d2d"
        max_norm = 20.0 if clipped else None
        # the first step: the same gradients going in (the first rollout and the gradient kernels are bit-equal) ...
        g_first = pre_clip[0] if (clipped and label == "policy") else lg_t.g_in[0]
        if not torch_epoch and not (clipped and label == "critic"):   # (the torch critic's is logged after its clip)
            assert all(torch.equal(a, b) for a, b in zip(g_first, lg_h.g_in[0])), (label, "first-step gradients")
        # ... .grad afterwards holds the clipped gradient, within 8u of the float64 clip of what went in
        if clipped:
            norms = O.agent_norms64(lg_h.g_in[0], N)
            print(f"  {setup} {label}: first-step gradient norms {[round(float(x), 2) for x in norms]} (clip at 20)")
            if label == "critic":
                assert bool((norms > 20.0).all()), "the critic's gradient must be over the clip"
                assert not any(torch.equal(a, b) for a, b in zip(lg_h.g_in[0], lg_h.g_out[0])), "the clip wrote nothing"
            g64 = O.clip_adam64(lg_h.init, lg_h.g_in[0], lg_h.init, lg_h.init, N, 1, max_norm=20.0)["g"]
            for i, name in enumerate(names):
                for who, lg in (("hip", lg_h),) + (() if torch_epoch else (("torch", lg_t),)):
                    err = (lg.g_out[0][i].double() - g64[i]).abs()
                    assert bool((err <= 8 * O.U * g64[i].abs()).all()), (label, name, who)
        # the K-step rule, each learner against the float64 replay of its own gradients: after step 1 and after step K
        for k_steps, p_t, p_h in ((1, lg_t.p_out[0], lg_h.p_out[0]),
                                  (K, [p.detach() for p in lg_t.params], [p.detach() for p in lg_h.params])):
            p64_t = replay(lg_t, N, lr_, eps, None, k_steps)
            p64_h = replay(lg_h, N, lr_, eps, max_norm, k_steps)
            worst = 0.0
            for i, name in enumerate(names):
                d_t = float((p_t[i].double() - p64_t[i]).abs().max())
                d_h = float((p_h[i].double() - p64_h[i]).abs().max())
                bar = 4 * d_t + O.U * float(p64_h[i].abs().max())
                worst = max(worst, d_h / bar)
                assert d_h <= bar, (label, name, k_steps, d_h, d_t, bar)
            print(f"  {setup} {label}: {k_steps} step(s), own-gradient K-step ratio {worst:.3g} (bar = 1)")
        # the other learner's gradients (information: the gradients differ after step 1) ...
        p64 = replay(lg_t, N, lr_, eps, None, K)
        ratio = 0.0
        for i in range(len(p64)):
            d_t = float((lg_t.params[i].detach().double() - p64[i]).abs().max())
            d_h = float((lg_h.params[i].detach().double() - p64[i]).abs().max())
            ratio = max(ratio, d_h / (4 * d_t + O.U * float(p64[i].abs().max())))
        print(f"  {setup} {label}: {K} steps, K-step ratio against the TORCH learner's float64 replay {ratio:.3g}")
        # ... and the Adam-aware bound between the two learners' weights
        for i, name in enumerate(names):
            steps = [{name: g[i].cpu().numpy()} for g in lg_t.g_in]
            shape = tuple(lg_t.params[i].shape)
            assert_weights_close(lg_h.params[i].detach().cpu().numpy(), lg_t.params[i].detach().double().cpu().numpy(),
                                 ref_adam_tolerance(steps, name, lr_, shape), f"{setup} {label} {name}", 2 * lr_ * K)


@pytest.mark.parametrize("setup", SETUPS)
def test_default_optimizer_is_torch_adam(setup):
    """A learner built without the kwarg (and without D2D_FUSED_OPTIM=1 in the environment) keeps torch.optim.Adam."""
    from algorithms._learner import BatchedLearnerBase
    assert os.environ.get("D2D_FUSED_OPTIM", "0") != "1", "run the suite without D2D_FUSED_OPTIM=1"
    assert BatchedLearnerBase.fused_optimizer is False
    ln, algo = _make(setup, None)
    assert ln.fused_optimizer is False
    for _, opt, *_ in _optimizers(ln, algo):
        assert type(opt) is torch.optim.Adam


def test_reference_trace_on_the_fused_optimizer():
    """The reference trace learner_d2d_mlp_comb_h128 (teacher-forced rollout, one iteration of 2 epochs) with
    fused_optimizer=True: the final weights of every agent and of the critic stay within the trace's
    reference-gradient bound (ref_adam_tolerance over the reference's recorded gradients).  The loss deviations are
    printed for DESIGN §4.11 and not asserted: the 1e-5 loss bar is what a differently rounded Adam moved before."""
    from d2dhip.optim import StackedAdam
    z = np.load(os.path.join(GOLDEN, "learner_d2d_mlp_comb_h128.npz"))
    n_ep = int(z["episodes"]) if "episodes" in z.files else 2
    env, kind, common, iPPO, D2DPPO = build(z, n_envs=1)
    ln = D2DPPO(env, beta_entropy=0.02, **common, fused_optimizer=True)
    assert isinstance(ln.policy_optimizer, StackedAdam) and isinstance(ln.value_optimizer, StackedAdam)
    for i, ag in enumerate(ln.agents):
        ag.policy_network.load_state_dict(_sd(z, f"init/agent{i}/policy"))
    ln.value_network.load_state_dict(_sd(z, "init/critic"))
    teacher = dict(actions=z["ro/actions"], reset_arrivals=z["draws/reset_arrivals"], flips=z["draws/flips"],
                   arrivals=z["draws/arrivals"])
    ro = ln._rollout(n_ep, teacher=teacher)
    ln._rollout = lambda num_episodes, teacher=None, defer_values=False, _ro=ro: _ro
    ln.test = lambda num_episodes: (0.5, 1.0, 0, 0.0)
    np.random.seed(21)
    res = ln.train(1, num_episodes=n_ep, n_epoch=2, test_freq=10 ** 9)
    dp = np.abs(np.array(res[2]) - z["train/policy_loss"]).max()
    dv = np.abs(np.array([float(v) for v in res[3]]) - z["train/value_loss"]).max()
    print(f"  learner_d2d_mlp_comb_h128 on the fused optimizer: max |policy loss - ref| {dp:.3g}, "
          f"max |value loss - ref| {dv:.3g} (torch's Adam is held to 1e-5)")
    assert int(ln.policy_optimizer.step_count) == 2 and int(ln.value_optimizer.step_count) == 2
    for msg, pre, net in _nets(ln, "d2d"):
        tag = pre[len("final/"):]
        steps = ref_grads(z, tag)
        lr_ = common["value_lr"] if tag == "critic" else common["policy_lr"]
        assert len(steps) == 2
        for k, v in net.named_parameters():
            vd = v.detach()
            assert_weights_close(vd.cpu().numpy(), z[f"{pre}/{k}"], ref_adam_tolerance(steps, k, lr_, tuple(vd.shape)),
                                 f"{msg} {k}", 2 * lr_ * len(steps))
