"""Pins the gradient oracle of tests/mlp_oracle.py (the float64 reference of tests/test_update_edges_gpu.py) without a
GPU:
1. its float32 instance equals, to 1e-6 of max|g| per tensor, autograd through algorithms._core.Policy / Value plus
   torch.distributions and the reference's loss expressions (ref_actor / ref_critic of tests/test_update_gpu.py), for
   both kinds, A in {1, 3, 8, 9, 16} and the saturated case (b2[:, 0] += 40: every sample at the clamp);
2. every input set the GPU file runs (mlp_oracle.update_input_sets: generated on the CPU from a per-case seed) is well
   conditioned on the reference alone: every probability in [1e-3, 1 - 1e-3] (A >= 2, saturated case excepted); torch
   fp32's own excess over the relu-flip envelope at most 2e-5 of max|g64[k]|, so that the GPU criterion's "4 x torch
   fp32" escape never widens the bar (saturated case excepted: there it may act); ambiguous (agent, sample, unit)
   pairs at most 1e-3 of a case's pairs; units (agent, hidden) with a nonzero envelope at most 10 % of its units; no
   ratio within 5e-4 of a clip edge (0.8, 0.9, 1.1, 1.2), where the surrogate's gradient jumps.
   A seed that breaks a cap is changed (mlp_oracle.update_inputs); the caps are not."""
import pytest
import torch

import mlp_oracle as O

AMB_CAP = 1e-3
UNIT_CAP = 0.10
EXCESS_CAP = 2e-5
CLIP, BETA = 0.1, 0.05

PIN = [(kind, F, H, A) for kind in ("comb", "chsel") for F, H, A in ((12, 33, 1), (30, 64, 3), (46, 32, 8), (31, 128, 9),
                                                                     (10, 16, 16))]


def _modules(inp, k, critic):
    """agent k's Policy / Value module loaded with the oracle's parameters"""
    from algorithms._core import Policy, Value
    kind, F, H, A = inp["shape"]
    d = (inp["dims"] or [F] * inp["N"])[k]
    m = Value(d, H) if critic else Policy(d, A, H)
    net = inp["critic" if critic else "actor"]
    with torch.no_grad():
        m.linear1.weight.copy_(net["w1"][k, :, :d])
        m.linear1.bias.copy_(net["b1"][k])
        m.linear2.weight.copy_(net["w2"][k])
        m.linear2.bias.copy_(net["b2"][k])
    return m, d


def _module_grads(m, d, F):
    g = {"w1": torch.zeros(m.linear1.weight.shape[0], F), "b1": m.linear1.bias.grad, "w2": m.linear2.weight.grad,
         "b2": m.linear2.bias.grad}
    g["w1"][:, :d] = m.linear1.weight.grad
    return g


def _pin(inp):
    from torch.distributions import Bernoulli, Categorical
    kind, F, H, A = inp["shape"]
    N, B = inp["N"], inp["T"] * inp["E"]
    obs = inp["obs"].view(B, N, F)
    scale = 1.0 / B
    a32 = O.actor_grad_oracle(inp["actor"], obs, kind, inp["acts"], inp["logp_old"], inp["W"], CLIP, BETA, scale,
                              torch.float32)
    c32 = O.critic_grad_oracle(inp["critic"], obs, inp["R"], scale, torch.float32)
    want_a, want_c = [], []
    for k in range(N):
        # the reference's expressions (ref_actor of tests/test_update_gpu.py) on the module
        pol, d = _modules(inp, k, False)
        pr = pol(obs[:, k, :d])
        if kind == "comb":
            dist = Bernoulli(probs=pr, validate_args=False)
            lp, ent = dist.log_prob(inp["acts"][k].float()).mean(-1), dist.entropy().mean(-1)
        else:
            dist = Categorical(probs=pr, validate_args=False)
            lp, ent = dist.log_prob(inp["acts"][k]), dist.entropy()
        ratio = torch.exp(lp - inp["logp_old"][k])
        s = torch.min(ratio * inp["W"][k], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * inp["W"][k])
        (-s.mean() - BETA * ent.mean()).backward()
        want_a.append(_module_grads(pol, d, F))
        assert abs(a32["surr"][k].item() - s.sum().item()) <= 1e-5 * max(1.0, abs(s.sum().item()))
        assert abs(a32["ent"][k].item() - ent.sum().item()) <= 1e-5 * max(1.0, abs(ent.sum().item()))
        # ref_critic
        val, d = _modules(inp, k, True)
        v = val(obs[:, k, :d])[:, 0]
        ((v - inp["R"][k]) ** 2).mean().backward()
        want_c.append(_module_grads(val, d, F))
        assert (c32["v"][k] - v.detach()).abs().max().item() <= 1e-6
    # 1e-6 of max|g| per (agent-stacked) tensor
    for net, got, want in (("actor", a32, want_a), ("critic", c32, want_c)):
        for name in want[0]:
            w = torch.stack([q[name] for q in want])
            top, err = w.abs().max().item(), (got["grads"][name] - w).abs().max().item()
            print(f"{inp['shape']} {inp['mode']} {net} {name}: max|g| {top:.3e}, |oracle32 - modules| {err:.2e}")
            assert err <= 1e-6 * top, (net, name, err, top)


@pytest.mark.parametrize("shape", PIN, ids=[f"{k}-F{F}-H{H}-A{A}" for k, F, H, A in PIN])
def test_fp32_oracle_equals_module_autograd(shape):
    for mode in ("int", "frac"):
        _pin(O.update_inputs(shape, 5, 2, 20, dims=O.upd_dims(shape[1]), mode=mode))


@pytest.mark.parametrize("kind", ["comb", "chsel"])
def test_fp32_oracle_equals_module_autograd_saturated(kind):
    inp = O.update_inputs((kind, 12, 33, 4), 5, 2, 20, saturated=True)
    p = O.probs(inp["actor"], inp["obs"].view(40, 5, 12))
    assert p[..., 1:].max().item() < O.EPS, "every sample at the clamp"
    _pin(inp)


def test_oracle_on_a_hand_made_sample():
    """One agent, one sample, H = 1, A = 2, w1 = b1 = 0 -> the logits are b2: every formula by hand."""
    import math
    z = torch.tensor([0.3, -0.2], dtype=torch.float64)
    net = {"w1": torch.zeros(1, 1, 1), "b1": torch.ones(1, 1), "w2": torch.zeros(1, 2, 1), "b2": z.float().view(1, 2)}
    z = net["b2"][0].double()
    p = torch.softmax(z, -1)
    obs = torch.zeros(1, 1, 1)
    for W, lo_shift, gate in ((1.5, 0.0, 1.0), (1.5, -0.5, 0.0), (-1.5, -0.5, 1.0), (1.5, 0.5, 1.0), (-1.5, 0.5, 0.0)):
        # chsel, action 1: logp = log p1; ratio = exp(-lo_shift)
        lo = torch.tensor([[math.log(p[1].item()) + lo_shift]])
        r = math.exp(math.log(p[1].item()) - lo.double().item())
        out = O.actor_grad_oracle(net, obs, "chsel", torch.tensor([[1]]), lo, torch.tensor([[W]]), 0.1, 0.0, 2.0)
        # d(-min(r W, clamp(r) W)) / dz = -gate r W (e_1 - p); ratio 1 is inside the clip range, 1.65 is clipped for
        # W > 0 (the min takes the clamped side: no gradient), kept for W < 0; 0.61 the other way round
        want = -2.0 * gate * r * W * (torch.tensor([0.0, 1.0], dtype=torch.float64) - p)
        assert (out["grads"]["b2"][0] - want).abs().max().item() < 1e-12, (W, lo_shift)
        assert abs(out["surr"].item() - min(r * W, min(max(r, 0.9), 1.1) * W)) < 1e-12
    # entropy: d(-beta H) / dz_j = beta p_j (log p_j + H)
    out = O.actor_grad_oracle(net, obs, "chsel", torch.tensor([[1]]), torch.zeros(1, 1), torch.zeros(1, 1), 0.1, 0.5, 1.0)
    Hh = -(p * p.log()).sum()
    assert (out["grads"]["b2"][0] - 0.5 * p * (p.log() + Hh)).abs().max().item() < 1e-12
    assert abs(out["ent"].item() - Hh.item()) < 1e-12
    # critic: v = w2 relu(b1) + b2 = 0.3; loss 2 (v - R)^2; and the envelope of an ambiguous unit
    cnet = {"w1": torch.zeros(1, 1, 1), "b1": torch.ones(1, 1), "w2": torch.ones(1, 1, 1), "b2": torch.full((1, 1), -0.7)}
    out = O.critic_grad_oracle(cnet, obs, torch.tensor([[1.3]]), 2.0)
    assert abs(out["v"].item() - cnet["b2"].double().item() - 1.0) < 1e-12
    d = out["v"].item() - torch.tensor(1.3).double().item()
    assert abs(out["grads"]["b2"].item() - 4.0 * d) < 1e-12 and abs(out["grads"]["b1"].item() - 4.0 * d) < 1e-12
    assert abs(out["loss"].item() - d * d) < 1e-12 and int(out["n_amb"]) == 0 and float(out["env"]["b1"].abs().max()) == 0.0
    cnet["w1"] = torch.full((1, 1, 1), 1.0)
    x = torch.full((1, 1, 1), 1.0)
    cnet["b1"] = torch.full((1, 1), -1.0) + 1e-7        # pre = 1e-7 * ~1.19: within 2 (F + 2) 2^-24 (|b| + |w x|) = 7e-7
    out = O.critic_grad_oracle(cnet, x, torch.tensor([[1.3]]), 2.0)
    assert int(out["n_amb"]) == 1
    dA = abs(4.0 * (out["v"].item() - torch.tensor(1.3).double().item()))   # |dL/dh| = |dL/dv| w2
    assert abs(out["env"]["b1"].item() - dA) < 1e-12 and abs(out["env"]["w1"].item() - dA) < 1e-12
    assert float(out["env"]["w2"].abs().max()) == 0.0 and float(out["env"]["b2"].abs().max()) == 0.0


SETS = O.update_input_sets()
WORST = {"amb": 0.0, "units": 0.0, "excess32": 0.0}


@pytest.mark.parametrize("label,kw", SETS, ids=[s[0].replace(" ", "").replace("'", "") for s in SETS])
def test_gpu_inputs_are_well_conditioned(label, kw):
    inp = O.update_inputs(**kw)
    kind, F, H, A = inp["shape"]
    N, B = inp["N"], inp["T"] * inp["E"]
    obs = inp["obs"].view(B, N, F)
    sat = kw.get("saturated", False)
    if inp["mode"] == "mixed":
        share = O.fractional_tiles(inp["T"], inp["E"], N).double().mean().item()
        assert 0.4 <= share <= 0.6, share
    args = (inp["actor"], obs, kind, inp["acts"], inp["logp_old"], inp["W"], CLIP, BETA, 1.0 / B)
    a64, a32 = O.actor_grad_oracle(*args), O.actor_grad_oracle(*args, torch.float32)
    c64 = O.critic_grad_oracle(inp["critic"], obs, inp["R"], 1.0 / B)
    c32 = O.critic_grad_oracle(inp["critic"], obs, inp["R"], 1.0 / B, torch.float32)
    p = a64["probs"]
    ratio = torch.exp(a64["logp"] - inp["logp_old"].double())
    assert min((ratio - edge).abs().min().item() for edge in O.CLIP_EDGES) >= 5e-4, "a ratio at a clip edge"
    assert N * B < 300 or (ratio.min().item() < 0.8 and ratio.max().item() > 1.2), "ratios beyond both clip ranges"
    if A >= 2 and not sat:
        assert p.min().item() >= 1e-3 and p.max().item() <= 1 - 1e-3, (p.min().item(), p.max().item())
    line = []
    for net, r64, r32 in (("actor", a64, a32), ("critic", c64, c32)):
        amb = r64["n_amb"].sum().item() / (N * B * H)
        units = ((r64["env"]["b1"] > 0) | (r64["env"]["w1"] > 0).any(-1)).double().mean().item()
        exc = max(O.grad_excess(r32["grads"][n], r64["grads"][n], r64["env"][n]).max().item() for n in r64["grads"])
        line.append(f"{net}: ambiguous pairs {amb:.2e}, units with an envelope {units:.3f}, torch fp32 excess {exc:.2e}")
        assert amb <= AMB_CAP, (net, amb)
        assert units <= UNIT_CAP, (net, units)
        if not (sat and net == "actor"):
            assert exc <= EXCESS_CAP, (net, exc)
            WORST["excess32"] = max(WORST["excess32"], exc)
        WORST["amb"], WORST["units"] = max(WORST["amb"], amb), max(WORST["units"], units)
    print(f"{label}: p in [{p.min().item():.3g}, {p.max().item():.3g}]; " + "; ".join(line))
    print(f"WORST so far: ambiguous-pair share {WORST['amb']:.2e}, unit share {WORST['units']:.3f}, "
          f"torch fp32 excess {WORST['excess32']:.2e}")
