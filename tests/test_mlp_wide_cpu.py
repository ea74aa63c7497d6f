"""The wide MLP entry points (d2d_policy_mlp_wide_step, d2d_ppo_actor_grad_wide, d2d_ppo_critic_grad_wide,
d2d_ppo_wide_workspace; csrc/mlp_wide_kernels.hip) without a GPU: their argument checks and envelope refusals, the one
Python rule that routes a shape to them, and -- on the float64 oracle alone -- the conditioning of every input set the
GPU files run (tests/mlp_wide_cases.py), with the caps of tests/test_mlp_oracle_cpu.py and
tests/test_update_oracle_cpu.py: probabilities in [1e-3, 1 - 1e-3] for A >= 2, tie masks <= 1 % of their cells,
ambiguous (sample, unit) pairs <= 1e-3, units with a relu-flip envelope <= 10 %, torch fp32's excess <= 2e-5, no ratio
within 5e-4 of a clip edge.  A seed that breaks a cap is changed, never the cap."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_oracle as O
import mlp_wide_cases as C

TIE_CAP, AMB_CAP, UNIT_CAP, EXCESS_CAP = 0.01, 1e-3, 0.10, 2e-5
CLIP, BETA = 0.1, 0.05


def test_one_rule_routes_shapes():
    from d2dhip import _lib
    wide = [(F, H) for F in (1, 30, 31, 32, 46, 63, 64) for H in (1, 64, 65, 100, 128, 129) if _lib.mlp_wide(F, H)]
    assert wide == [(F, H) for F in (32, 46, 63) for H in (65, 100, 128)]
    lib = _lib.load()
    names = {w: (_lib.mlp_entry(lib, w, 30, 128)[1], _lib.mlp_entry(lib, w, 46, 128)[1])
             for w in ("policy", "workspace", "actor_grad", "critic_grad")}
    assert names == {"policy": ("d2d_policy_mlp_step", "d2d_policy_mlp_wide_step"),
                     "workspace": ("d2d_ppo_workspace", "d2d_ppo_wide_workspace"),
                     "actor_grad": ("d2d_ppo_actor_grad", "d2d_ppo_actor_grad_wide"),
                     "critic_grad": ("d2d_ppo_critic_grad_values", "d2d_ppo_critic_grad_wide")}
    # d2dhip.update's default (allow_wide=False): the narrow entry whatever the shape
    assert [_lib.mlp_entry(lib, w, 46, 128, False)[1] for w in ("workspace", "actor_grad", "critic_grad")] == \
        ["d2d_ppo_workspace", "d2d_ppo_actor_grad", "d2d_ppo_critic_grad_values"]
    for name in ("d2d_policy_mlp_wide_step", "d2d_ppo_wide_workspace", "d2d_ppo_actor_grad_wide",
                 "d2d_ppo_critic_grad_wide"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.d2d_abi_version() == 15                       # additions on top of ABI v15


def test_wide_entry_points_validate_arguments_without_gpu():
    """Every check runs before any HIP call, so it works on a GPU-less host; nothing here passes all of them."""
    from d2dhip import _lib
    lib = _lib.load()
    w = ctypes.c_void_p(16)
    st = (ctypes.c_int64 * 3)(1, 1, 1)
    neg = (ctypes.c_int64 * 3)(1, -1, 1)
    err = lambda: lib.d2d_last_error()  # noqa: E731

    def desc(F=46, H=128, A=16, kind=0, critic=(None, None, None, None), fmt=_lib.D2D_OBS_F32, sgn=None, N=4, E=32):
        return _lib.MlpDesc(N, E, F, H, A, kind, w, w, w, w, *critic, 0, 0, None, fmt, 0, sgn)

    def policy(d, obs=w, forced=None, actions=w, logp=w):
        return lib.d2d_policy_mlp_wide_step(ctypes.byref(d), obs, forced, 0, 0, actions, logp, None, None)

    def actor(d, obs=w, T=3, lo_st=st, w_st=st, ws=w, ws_floats=1 << 40, gw1=w, acts=w):
        return lib.d2d_ppo_actor_grad_wide(ctypes.byref(d), T, obs, acts, w, lo_st, w, w_st, 0.1, 0.05, 1.0, gw1, w, w,
                                           w, w, ws, ws_floats, None)

    def critic(d, obs=w, T=3, r_st=st, ws=w, ws_floats=1 << 40, values=None, v_st=None, gw1=w):
        return lib.d2d_ppo_critic_grad_wide(ctypes.byref(d), T, obs, w, r_st, 1.0, gw1, w, w, w, w, ws, ws_floats,
                                            values, v_st, None)

    # the envelope: 64 < hidden <= 128, 32 < obs_dim + 1 <= 64, n_out in [1, 16]
    for bad in (dict(F=31), dict(F=64), dict(H=64), dict(H=129), dict(F=30, H=64), dict(F=31, H=128), dict(F=1, H=1)):
        for call in (policy, actor, critic):
            assert call(desc(**bad)) == -2, (bad, call.__name__)
            assert b"64 < hidden <= 128" in err() and b"32 < obs_dim + 1 <= 64" in err(), err()
    for bad in (dict(A=0), dict(A=17)):
        assert policy(desc(**bad)) == -2 and b"n_out <= 16" in err(), bad
        assert actor(desc(**bad)) == -2 and b"n_out <= 16" in err(), bad
        assert critic(desc(**bad), ws_floats=0) == -1 and b"workspace" in err()   # n_out is ignored: the next check
    # NULLs
    assert lib.d2d_policy_mlp_wide_step(None, w, None, 0, 0, w, w, None, None) == -1 and b"NULL" in err()
    assert policy(desc(), obs=None) == -1 and b"NULL" in err()
    assert policy(desc(), logp=None) == -1 and b"NULL" in err()
    assert policy(desc(), actions=None) == -1 and b"NULL" in err()        # actions = NULL in forced mode only
    assert actor(desc(), acts=None) == -1 and b"NULL" in err()
    assert actor(desc(), gw1=None) == -1 and b"NULL" in err()
    assert actor(desc(), obs=None) == -1 and b"NULL" in err()
    assert critic(desc(), gw1=None) == -1 and b"NULL" in err()
    assert critic(desc(), r_st=None) == -1 and b"NULL" in err()
    assert critic(desc(), values=w) == -1 and b"values without strides" in err()
    # kind, critic tensors, sizes
    assert policy(desc(kind=2)) == -1 and b"kind" in err()
    assert actor(desc(kind=2)) == -1 and b"kind" in err()
    for missing in range(1, 4):
        crit = [w, w, w, w]
        crit[missing] = None
        assert policy(desc(critic=crit)) == -1 and b"critic" in err(), missing
    assert policy(desc(E=-1)) == -1 and b"negative" in err()
    assert actor(desc(), T=-1) == -1 and b"negative" in err()
    assert critic(desc(N=-1)) == -1 and b"negative" in err()
    # obs_format / obs_signed / alignment of the record
    for call in (policy, actor, critic):
        assert call(desc(fmt=7)) == -1 and b"obs_format" in err()
        assert call(desc(fmt=_lib.D2D_OBS_U8)) == -1 and b"obs_signed" in err()
        assert call(desc(fmt=_lib.D2D_OBS_U8, sgn=w), obs=ctypes.c_void_p(24)) == -1 and b"aligned" in err()
    # strides
    assert actor(desc(), lo_st=neg) == -1 and b"strides" in err()
    assert actor(desc(), w_st=neg) == -1 and b"strides" in err()
    assert critic(desc(), r_st=neg) == -1 and b"strides" in err()
    assert critic(desc(), values=w, v_st=neg) == -1 and b"strides" in err()
    # the workspace: one float short, or NULL where one is needed
    need = lib.d2d_ppo_wide_workspace(4, 3, 32, 46, 128, 16)
    assert actor(desc(), ws_floats=need - 1) == -1 and b"workspace" in err()
    assert actor(desc(), ws=None) == -1 and b"workspace" in err()
    need = lib.d2d_ppo_wide_workspace(4, 3, 32, 46, 128, 1)
    assert critic(desc(), ws_floats=need - 1) == -1 and b"workspace" in err()
    # the narrow entry points still refuse the wide corner (tests/test_abi_cpu.py pins one point of it)
    d = desc()
    assert lib.d2d_policy_mlp_step(ctypes.byref(d), w, None, 0, 0, w, w, None, None) == -2


def test_workspace_is_the_grid_rule():
    """d2d_ppo_wide_workspace = 4 G N P floats with G from wide_blocks (one partial per wave); 0 with no sample."""
    from d2dhip import _lib
    lib = _lib.load()
    for N, T, E, F, H, A in [(5, 3, 45, 46, 128, 16), (256, 25, 70, 32, 65, 5), (256, 75, 9, 46, 128, 1),
                             (1, 1, 1, 63, 100, 1), (6, 12, 4096, 46, 128, 16), (3, 40, 65536, 32, 128, 8)]:
        P = H * F + H + A * H + A + 2
        G = C.wide_blocks(N, T * ((E + 15) // 16))
        assert lib.d2d_ppo_wide_workspace(N, T, E, F, H, A) == 4 * G * N * P, (N, T, E)
    for N, T, E in [(0, 3, 45), (5, 0, 45), (5, 3, 0)]:
        assert lib.d2d_ppo_wide_workspace(N, T, E, 46, 128, 16) == 0
    # at N = 256 one workgroup serves an agent: every wave of the tile cases takes several tiles
    for shape, T, E, _ in C.TILE_CASES:
        n_tiles = T * ((E + 15) // 16)
        assert n_tiles >= 8 * C.wide_blocks(C.TILE_N, n_tiles)


@pytest.mark.parametrize("frac", [False, True], ids=["int", "frac"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_policy_inputs_are_well_conditioned(shape, frac):
    kind, F, H, A = shape
    worst, lo, hi = 0.0, 1.0, 0.0
    for N, E, dims in C.batches(shape):
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
        v32, v64 = O.values(critic, obs, torch.float32), O.values(critic, obs)
        assert (v32.double() - v64).abs().max().item() < 1e-5
        if not frac:
            assert torch.equal(obs, obs.round()) and obs.abs().max().item() <= 127, "record inputs are small integers"
    print(f"{shape} frac {frac}: p in [{lo:.3g}, {hi:.3g}], largest tie share {worst:.5f}")


SETS = C.update_input_sets()


@pytest.mark.parametrize("label,kw", SETS, ids=[s[0].replace(" ", "_") for s in SETS])
def test_update_inputs_are_well_conditioned(label, kw):
    inp = O.update_inputs(**kw)
    kind, F, H, A = inp["shape"]
    N, B = inp["N"], inp["T"] * inp["E"]
    obs = inp["obs"].view(B, N, F)
    sat = kw.get("saturated", False)
    args = (inp["actor"], obs, kind, inp["acts"], inp["logp_old"], inp["W"], CLIP, BETA, 1.0 / B)
    a64, a32 = O.actor_grad_oracle(*args), O.actor_grad_oracle(*args, torch.float32)
    c64 = O.critic_grad_oracle(inp["critic"], obs, inp["R"], 1.0 / B)
    c32 = O.critic_grad_oracle(inp["critic"], obs, inp["R"], 1.0 / B, torch.float32)
    p = a64["probs"]
    ratio = torch.exp(a64["logp"] - inp["logp_old"].double())
    edge = min((ratio - e).abs().min().item() for e in O.CLIP_EDGES)
    assert edge >= 5e-4, "a ratio at a clip edge"
    if A >= 2 and not sat:
        assert p.min().item() >= 1e-3 and p.max().item() <= 1 - 1e-3, (p.min().item(), p.max().item())
    if sat:
        assert p[..., 1:].max().item() < O.EPS, "every sample at the clamp"
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
    print(f"{label}: p in [{p.min().item():.3g}, {p.max().item():.3g}]; nearest clip edge {edge:.1e}; " + "; ".join(line))
