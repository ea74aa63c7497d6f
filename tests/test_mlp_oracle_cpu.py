"""Pins tests/mlp_oracle.py (the float64 reference of tests/test_policy_edges_gpu.py) without a GPU:
1. its float32 instance equals algorithms._core.Policy / Value modules loaded with the same parameters plus
   torch.distributions.Bernoulli / Categorical, to 1e-6;
2. the inputs of every GPU run are well conditioned on the reference alone: for A >= 2 every probability lies in
   [1e-3, 1 - 1e-3], and each tie mask (sampled and deterministic actions) excludes at most 1 % of its cells.
   A seed that breaks a condition is changed (mlp_oracle.shape_seed); the caps are not."""
import numpy as np
import pytest
import torch

import mlp_oracle as O

TIE_CAP = 0.01
IDS = [f"{k}-F{F}-H{H}-A{A}" for k, F, H, A in O.SHAPES]


@pytest.mark.parametrize("frac", [False, True], ids=["int", "frac"])
@pytest.mark.parametrize("shape", O.SHAPES, ids=IDS)
def test_fp32_oracle_equals_the_modules(shape, frac):
    from algorithms._core import Policy, Value
    from torch.distributions import Bernoulli, Categorical
    kind, F, H, A = shape
    N, E = 5, 33
    dims = O.HET.get(shape)
    actor, critic, obs = O.case_inputs(shape, N, E, dims, frac)
    p32, v32 = O.probs(actor, obs, torch.float32), O.values(critic, obs, torch.float32)
    g = torch.Generator().manual_seed(1)
    for k in range(N):
        d = (dims or [F] * N)[k]
        pol, val = Policy(d, A, H), Value(d, H)
        with torch.no_grad():
            for m, net in ((pol, actor), (val, critic)):
                m.linear1.weight.copy_(net["w1"][k, :, :d])
                m.linear1.bias.copy_(net["b1"][k])
                m.linear2.weight.copy_(net["w2"][k])
                m.linear2.bias.copy_(net["b2"][k])
            pm, vm = pol(obs[:, k, :d]), val(obs[:, k, :d])[:, 0]
        assert (pm - p32[k]).abs().max().item() <= 1e-6
        assert (vm - v32[k]).abs().max().item() <= 1e-6
        if kind == "comb":
            bits = torch.rand((E, A), generator=g) < 0.4
            want = Bernoulli(probs=pm, validate_args=False).log_prob(bits.float()).mean(-1)
            got = O.bernoulli_logp(p32[k], bits)
        else:
            ids = torch.randint(0, A, (E,), generator=g)
            want = Categorical(probs=pm, validate_args=False).log_prob(ids)
            got = O.categorical_logp(p32[k], ids)
        assert (got - want).abs().max().item() <= 1e-6


def test_action_rules_on_hand_made_probabilities():
    p = torch.tensor([[[0.2, 0.5, 0.3], [0.4, 0.4, 0.2], [0.500001, 0.25, 0.249999]]], dtype=torch.float64)
    a, tie = O.deterministic_actions(p, "comb")
    assert a.tolist() == [[[False, False, False], [False, False, False], [True, False, False]]]
    assert tie.tolist() == [[[False, True, False], [False, False, False], [True, False, False]]]
    a, tie = O.deterministic_actions(p, "chsel")
    assert a.tolist() == [[1, 0, 0]] and tie.tolist() == [[False, True, False]]       # lowest index of a tie
    # the clamp: eps = 2^-23, not float64's
    q = torch.tensor([[[1.0, 0.0]]], dtype=torch.float64)
    want = (np.log(1 - 2.0 ** -23) + np.log(2.0 ** -23)) / 2
    assert abs(O.bernoulli_logp(q, torch.tensor([[[1, 1]]])).item() - want) < 1e-12
    assert abs(O.categorical_logp(q, torch.tensor([[1]])).item() - np.log(2.0 ** -23)) < 1e-12
    # the sampler against a scalar restatement of the kernel's rule
    from oracle import philox
    envs, agents, step, seed = 77 + np.arange(4), np.arange(3), 5, 1234
    g = torch.Generator().manual_seed(0)
    p = torch.softmax(torch.randn((3, 4, 6), generator=g, dtype=torch.float64), -1)
    bits, _ = O.sampled_actions(p, "comb", envs, agents, step, seed)
    ids, _ = O.sampled_actions(p, "chsel", envs, agents, step, seed)
    for k in range(3):
        for e in range(4):
            for a in range(6):
                w = int(philox.philox4x32_10(envs[e], k, step, (3 << 24) | (a // 4), seed)[a % 4])
                assert bool(bits[k, e, a]) == ((w >> 8) / 2.0 ** 24 < p[k, e, a].item())
            u = (int(philox.philox4x32_10(envs[e], k, step, 3 << 24, seed)[0]) >> 8) / 2.0 ** 24 * p[k, e].sum().item()
            c, pick = 0.0, 5
            for a in range(6):
                c += p[k, e, a].item()
                if u < c:
                    pick = a
                    break
            assert int(ids[k, e]) == pick


@pytest.mark.parametrize("frac", [False, True], ids=["int", "frac"])
@pytest.mark.parametrize("shape", O.SHAPES, ids=IDS)
def test_gpu_inputs_are_well_conditioned(shape, frac):
    kind, F, H, A = shape
    worst, lo, hi = 0.0, 1.0, 0.0
    for N, E, dims in O.batches(shape):
        actor, critic, obs = O.case_inputs(shape, N, E, dims, frac)
        p = O.probs(actor, obs)
        lo, hi = min(lo, p.min().item()), max(hi, p.max().item())
        if A >= 2:
            assert p.min().item() >= 1e-3 and p.max().item() <= 1 - 1e-3, (N, E, p.min().item(), p.max().item())
        _, t_det = O.deterministic_actions(p, kind)
        _, t_smp = O.sampled_actions(p, kind, O.RNG["env_base"] + np.arange(E), np.arange(N), O.RNG["rng_step"],
                                     O.RNG["seed"])
        for name, t in (("deterministic", t_det), ("sampled", t_smp)):
            share = t.double().mean().item()
            worst = max(worst, share)
            assert share <= TIE_CAP, (name, N, E, share)
        # torch fp32 against float64: the scale of the GPU test's "twice torch fp32" escape
        v32, v64 = O.values(critic, obs, torch.float32), O.values(critic, obs)
        assert (v32.double() - v64).abs().max().item() < 1e-5
    print(f"{shape} frac {frac}: p in [{lo:.3g}, {hi:.3g}], largest tie share {worst:.5f}")
