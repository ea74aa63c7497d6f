"""The MLP entry points for 17..32 action ids (d2d_policy_mlp_actions_step, d2d_ppo_actor_grad_actions,
d2d_ppo_actions_workspace; csrc/mlp_actions_kernels.hip) without a GPU: their argument checks and envelope refusals
(every check runs before any HIP call), the unchanged refusals of the older entry points at n_out = 17, the one Python
rule d2dhip._lib.mlp_actions against the C envelope, the learners' gates on a stub learner, the workspace against the
restated grid rule, and -- on the float64 oracle alone -- the conditioning of every input set the GPU files run
(tests/mlp_actions_cases.py), with the caps of DESIGN §6.1 / §6.2: probabilities in [1e-3, 1 - 1e-3], tie masks <= 1 %
of their cells, no ratio within 5e-4 of a clip edge, ambiguous (sample, unit) pairs <= 1e-3, units with a relu-flip
envelope <= 10 %, torch fp32's excess <= 2e-5.  A seed that breaks a cap is changed, never the cap."""
import ctypes
import types

import numpy as np
import pytest
import torch

import mlp_actions_cases as C
import mlp_oracle as O

TIE_CAP, AMB_CAP, UNIT_CAP, EXCESS_CAP = 0.01, 1e-3, 0.10, 2e-5
CLIP, BETA = 0.1, 0.05
NEW = ("d2d_policy_mlp_actions_step", "d2d_ppo_actions_workspace", "d2d_ppo_actor_grad_actions")


def _calls():
    from d2dhip import _lib
    lib = _lib.load()
    w = ctypes.c_void_p(16)
    st = (ctypes.c_int64 * 3)(1, 1, 1)

    def desc(F=24, H=64, A=17, kind=1, critic=(None, None, None, None), fmt=_lib.D2D_OBS_F32, sgn=None, N=4, E=32):
        return _lib.MlpDesc(N, E, F, H, A, kind, w, w, w, w, *critic, 0, 0, None, fmt, 0, sgn)

    def policy(d, obs=w, forced=None, actions=w, logp=w, fn="d2d_policy_mlp_actions_step"):
        return getattr(lib, fn)(ctypes.byref(d), obs, forced, 0, 0, actions, logp, None, None)

    def actor(d, obs=w, T=3, lo_st=st, w_st=st, ws=w, ws_floats=1 << 40, gw1=w, acts=w,
              fn="d2d_ppo_actor_grad_actions"):
        return getattr(lib, fn)(ctypes.byref(d), T, obs, acts, w, lo_st, w, w_st, 0.1, 0.05, 1.0, gw1, w, w, w, w, ws,
                                ws_floats, None)

    return _lib, lib, w, st, desc, policy, actor


def test_exports_and_routing():
    _lib, lib, *_ = _calls()
    for name in NEW:
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.d2d_abi_version() == 15                       # additions on top of ABI v15
    names = lambda F, H, A, kind, wide=True: [_lib.mlp_entry(lib, w, F, H, wide, A, kind)[1]      # noqa: E731
                                              for w in ("policy", "workspace", "actor_grad", "critic_grad")]
    assert names(24, 64, 17, 1) == list(NEW[:1] + NEW[1:2] + NEW[2:]) + ["d2d_ppo_critic_grad_values"]
    assert names(46, 128, 32, "chsel")[3] == "d2d_ppo_critic_grad_wide"            # the critic: by (F, H) alone
    assert names(46, 128, 32, "chsel", False)[:3] == list(NEW)                     # no opt-in needed: nothing older takes it
    assert names(24, 64, 16, 1)[:3] == ["d2d_policy_mlp_step", "d2d_ppo_workspace", "d2d_ppo_actor_grad"]
    assert names(24, 64, 17, 0)[:3] == ["d2d_policy_mlp_step", "d2d_ppo_workspace", "d2d_ppo_actor_grad"]
    assert names(46, 128, 16, 1)[0] == "d2d_policy_mlp_wide_step"
    # existing callers (no action count) keep their results
    assert _lib.mlp_entry(lib, "policy", 30, 128)[1] == "d2d_policy_mlp_step"
    assert _lib.mlp_entry(lib, "actor_grad", 46, 128)[1] == "d2d_ppo_actor_grad_wide"
    assert _lib.mlp_entry(lib, "actor_grad", 46, 128, False)[1] == "d2d_ppo_actor_grad"


GRID = [(F, H, A, kind) for F in (0, 1, 24, 63, 64) for H in (0, 1, 64, 65, 128, 129) for A in (1, 16, 17, 32, 33)
        for kind in (0, 1)]


def test_python_rule_agrees_with_the_c_envelope():
    _lib, lib, w, st, desc, policy, actor = _calls()
    err = lambda: lib.d2d_last_error().decode()  # noqa: E731
    for F, H, A, kind in GRID:
        want = kind == 1 and 17 <= A <= 32 and 1 <= H <= 128 and 1 <= F <= 63
        assert _lib.mlp_actions(F, H, A, kind) is want, (F, H, A, kind)
        assert _lib.mlp_actions(F, H, A, "chsel" if kind else "comb") is want
        d = desc(F=F, H=H, A=A, kind=kind, N=0, E=0)      # empty: the checks run, nothing is launched
        for call in (policy, actor):
            rc = call(d)
            assert (rc == 0) is want, (F, H, A, kind, rc, err())
            if not want:
                assert rc == -2, (rc, err())                    # D2D_EUNSUPPORTED, the envelope in the message
                for word in ("kind 1", "17 <= n_out <= 32", "1 <= hidden <= 128", "obs_dim + 1 <= 64", "fp32 rows"):
                    assert word in err(), err()
    for s in C.SHAPES:
        assert _lib.mlp_actions(s[1], s[2], s[3], 1)


def test_entry_points_validate_arguments_without_gpu():
    _lib, lib, w, st, desc, policy, actor = _calls()
    neg = (ctypes.c_int64 * 3)(1, -1, 1)
    err = lambda: lib.d2d_last_error()  # noqa: E731
    # the record input: refused, with the envelope
    sgn = ctypes.c_void_p(32)
    for call in (policy, actor):
        assert call(desc(fmt=_lib.D2D_OBS_U8, sgn=sgn)) == -2 and b"record" in err() and b"17 <= n_out <= 32" in err()
        assert call(desc(fmt=7)) == -1 and b"obs_format" in err()
    # NULLs
    assert lib.d2d_policy_mlp_actions_step(None, w, None, 0, 0, w, w, None, None) == -1 and b"NULL" in err()
    assert policy(desc(), obs=None) == -1 and b"NULL" in err()
    assert policy(desc(), logp=None) == -1 and b"NULL" in err()
    assert policy(desc(), actions=None) == -1 and b"NULL" in err()        # actions = NULL in forced mode only
    assert actor(desc(), acts=None) == -1 and b"NULL" in err()
    assert actor(desc(), gw1=None) == -1 and b"NULL" in err()
    assert actor(desc(), obs=None) == -1 and b"NULL" in err()
    assert actor(desc(), lo_st=None) == -1 and b"NULL" in err()
    # kind, critic tensors, sizes, strides
    assert policy(desc(kind=2)) == -1 and b"kind" in err()
    assert actor(desc(kind=2)) == -1 and b"kind" in err()
    for missing in range(1, 4):
        crit = [w, w, w, w]
        crit[missing] = None
        assert policy(desc(critic=crit)) == -1 and b"critic" in err(), missing
    assert policy(desc(E=-1)) == -1 and b"negative" in err()
    assert actor(desc(), T=-1) == -1 and b"negative" in err()
    assert actor(desc(N=-1)) == -1 and b"negative" in err()
    assert actor(desc(), lo_st=neg) == -1 and b"strides" in err()
    assert actor(desc(), w_st=neg) == -1 and b"strides" in err()
    # the workspace: one float short, or NULL where one is needed
    need = lib.d2d_ppo_actions_workspace(4, 3, 32, 24, 64, 17)
    assert need > 0
    assert actor(desc(), ws_floats=need - 1) == -1 and b"workspace" in err()
    assert actor(desc(), ws=None) == -1 and b"workspace" in err()


def test_older_entry_points_still_refuse_17_ids():
    _lib, lib, w, st, desc, policy, actor = _calls()
    err = lambda: lib.d2d_last_error()  # noqa: E731
    assert policy(desc(), fn="d2d_policy_mlp_step") == -2
    assert actor(desc(), fn="d2d_ppo_actor_grad") == -2
    assert policy(desc(F=46, H=128), fn="d2d_policy_mlp_wide_step") == -2 and b"n_out <= 16" in err()
    assert actor(desc(F=46, H=128), fn="d2d_ppo_actor_grad_wide") == -2 and b"n_out <= 16" in err()


def test_workspace_is_the_grid_rule():
    """d2d_ppo_actions_workspace = 4 G N P floats with G from actions_blocks (one partial per wave and agent)"""
    _lib, lib, *_ = _calls()
    for N, T, E, F, H, A in [(5, 3, 45, 24, 64, 17), (256, 25, 70, 24, 64, 17), (256, 75, 9, 63, 128, 32),
                             (1, 1, 1, 1, 1, 17), (6, 12, 4096, 24, 128, 17), (3, 40, 65536, 31, 128, 32)]:
        want = C.workspace_floats(N, T, E, F, H, A)
        assert want > 0 and lib.d2d_ppo_actions_workspace(N, T, E, F, H, A) == want, (N, T, E)
    for N, T, E in [(0, 3, 45), (5, 0, 45), (5, 3, 0)]:
        assert lib.d2d_ppo_actions_workspace(N, T, E, 24, 64, 17) == 0 == C.workspace_floats(N, T, E, 24, 64, 17)
    shape, T, E, _ = C.TILE_CASE
    n_tiles = T * ((E + 15) // 16)
    assert C.actions_blocks(C.TILE_N, n_tiles) == 1 and n_tiles >= 8     # each of the 4 waves sums >= 31 tiles


# ------------------------------------------------------------------------------------------ the learners' gates

class _Stub:
    """What _fused_ok / _fused_update_ok / _record_ok read of a learner (a learner itself needs the GPU to be built):
    a ChannelSelectionEnv learner's policy shape, F = deadline 7 + n_channels + 1 inputs, A = n_channels + 1 ids."""

    def __init__(self, n_channels, hidden, useRNN=False):
        from algorithms._learner import BatchedLearnerBase as B
        self.useRNN, self.combinatorial, self.kind, self.history_len = useRNN, False, "chsel", 10
        self.policy = types.SimpleNamespace(kind="rnn" if useRNN else "mlp", F=7 + n_channels + 1, H=hidden,
                                            A=n_channels + 1, N=5)
        self.obs_record = True
        for name in ("_gru_ok", "_fused_ok", "_fused_update_ok", "_record_ok", "_gru_kind"):
            setattr(self, name, getattr(B, name).__get__(self))


@pytest.mark.parametrize("n_channels,hidden,want", [(16, 64, True), (16, 128, True), (31, 128, True), (32, 128, False),
                                                    (32, 64, False), (16, 129, False), (15, 64, True)])
def test_learner_gates_follow_the_rule(n_channels, hidden, want, monkeypatch):
    from d2dhip import _lib
    monkeypatch.delenv("D2D_FUSED_POLICY", raising=False)
    monkeypatch.delenv("D2D_FUSED_UPDATE", raising=False)
    lr = _Stub(n_channels, hidden)
    assert bool(lr._fused_ok()) is want and bool(lr._fused_update_ok()) is want
    if n_channels >= 16:
        assert _lib.mlp_actions(lr.policy.F, hidden, n_channels + 1, 1) is want
    assert not lr._record_ok()
    assert not _Stub(n_channels, hidden)._gru_ok()


@pytest.mark.parametrize("var", ["D2D_FUSED_POLICY", "D2D_FUSED_UPDATE"])
def test_environment_switches_force_the_torch_path(var, monkeypatch):
    monkeypatch.delenv("D2D_FUSED_POLICY", raising=False)
    monkeypatch.delenv("D2D_FUSED_UPDATE", raising=False)
    monkeypatch.setenv(var, "0")
    lr = _Stub(16, 64)
    assert bool(lr._fused_ok()) is (var != "D2D_FUSED_POLICY")
    assert not lr._fused_update_ok() and not lr._record_ok()


# ------------------------------------------------------------------------------------------ input conditioning

MEASURED = {"p_min": 1.0, "p_max": 0.0, "tie": 0.0, "amb": 0.0, "units": 0.0, "excess": 0.0, "edge": 1.0}


def test_case_table():
    assert len(set(C.SHAPES)) == 9 and all(k == "chsel" and 17 <= A <= 32 for k, F, H, A in C.SHAPES)
    assert {(H + 15) // 16 for _, F, H, A in C.SHAPES} >= {1, 4, 5, 7, 8}
    assert {A for _, F, H, A in C.SHAPES} >= {17, 20, 25, 32} and {F for _, F, H, A in C.SHAPES} >= {1, 31, 32, 63}
    assert C.HET[("chsel", 24, 64, 17)] == [24, 20, 24, 17, 24]


@pytest.mark.parametrize("frac", [False, True], ids=["int", "frac"])
@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_policy_inputs_are_well_conditioned(shape, frac):
    kind, F, H, A = shape
    worst, lo, hi = 0.0, 1.0, 0.0
    for N, E, dims in C.batches(shape):
        r = C.policy_ref(shape, N, E, None if dims is None else tuple(dims), frac)
        p = r.p64
        lo, hi = min(lo, p.min().item()), max(hi, p.max().item())
        assert p.min().item() >= 1e-3 and p.max().item() <= 1 - 1e-3, (N, E, p.min().item(), p.max().item())
        for name, t in (("deterministic", r.det_tie), ("sampled", r.smp_tie)):
            share = t.double().mean().item()
            worst = max(worst, share)
            assert share <= TIE_CAP, (name, N, E, share)
        assert (r.v32.double() - r.v64).abs().max().item() < 1e-5
        assert set(r.forced.reshape(-1).tolist()) == set(range(A)), "every id is forced"
        if not frac:
            assert torch.equal(r.obs, r.obs.round())
        else:
            assert float((r.obs != r.obs.round()).float().mean()) > 0.3
        if N == 5 and dims is None and shape in C.TILE1_SHAPES:
            seen = set(r.smp[~r.smp_tie].tolist())
            assert set(range(16, A)) <= seen, sorted(set(range(16, A)) - seen)
    MEASURED.update(p_min=min(MEASURED["p_min"], lo), p_max=max(MEASURED["p_max"], hi), tie=max(MEASURED["tie"], worst))
    print(f"{shape} frac {frac}: p in [{lo:.3g}, {hi:.3g}], largest tie share {worst:.5f}")


SETS = C.update_input_sets()


@pytest.mark.parametrize("label,kw", SETS, ids=[s[0].replace(" ", "_") for s in SETS])
def test_update_inputs_are_well_conditioned(label, kw):
    inp = C.update_inputs(**kw)
    kind, F, H, A = inp["shape"]
    N, B = inp["N"], inp["T"] * inp["E"]
    obs = inp["obs"].view(B, N, F)
    args = (inp["actor"], obs, kind, inp["acts"], inp["logp_old"], inp["W"], CLIP, BETA, 1.0 / B)
    a64, a32 = O.actor_grad_oracle(*args), O.actor_grad_oracle(*args, torch.float32)
    p = a64["probs"]
    ratio = torch.exp(a64["logp"] - inp["logp_old"].double())
    edge = min((ratio - e).abs().min().item() for e in O.CLIP_EDGES)
    assert edge >= 5e-4, "a ratio at a clip edge"
    assert p.min().item() >= 1e-3 and p.max().item() <= 1 - 1e-3, (p.min().item(), p.max().item())
    if N * B >= A:
        assert set(inp["acts"].reshape(-1).tolist()) == set(range(A)), "every id is used (16 and A - 1 included)"
    amb = a64["n_amb"].sum().item() / (N * B * H)
    units = ((a64["env"]["b1"] > 0) | (a64["env"]["w1"] > 0).any(-1)).double().mean().item()
    exc = max(O.grad_excess(a32["grads"][n], a64["grads"][n], a64["env"][n]).max().item() for n in a64["grads"])
    assert amb <= AMB_CAP, amb
    assert units <= UNIT_CAP, units
    assert exc <= EXCESS_CAP, exc
    for key, v in (("p_min", -p.min().item()), ("p_max", p.max().item()), ("amb", amb), ("units", units),
                   ("excess", exc), ("edge", -edge)):
        MEASURED[key] = -max(-MEASURED[key], v) if key in ("p_min", "edge") else max(MEASURED[key], v)
    print(f"{label}: p in [{p.min().item():.3g}, {p.max().item():.3g}]; nearest clip edge {edge:.1e}; ambiguous pairs "
          f"{amb:.2e}, units with an envelope {units:.3f}, torch fp32 excess {exc:.2e}")


def test_report_measured():
    """(after the sets above, in file order) the extremes over all sets, for DESIGN.md"""
    print("  " + ", ".join(f"{k} {v:.3g}" for k, v in MEASURED.items()))
