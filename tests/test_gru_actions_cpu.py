"""The categorical GRU head with 17..32 ids, without a GPU:

- every input set of tests/test_gru_actions_gpu.py (tests/gru_actions_cases.py) meets the conditions that
  tests/test_gru_oracle_cpu.py::test_input_set_conditions asserts for the one-tile sets -- conditions on the float64 /
  float32 torch references alone, not measurements of a kernel;
- the sampler sets' reference ids cover every id of the second tile;
- the C envelope (check_gru_desc) through the empty-batch early return: n_envs = 0 reaches no kernel, so the library
  answers without a device -- kind 1 with n_out in 17..32 at hidden <= 64 on fp32 rows is accepted, and n_out = 33, the
  sigmoid head, hidden > 64 and the record input with n_out = 17 are refused with a message naming the rule;
- d2d_gru_grad_workspace grows by the second tile's head sums and head-image rows;
- the Python rule d2dhip.gru.supported and the learners' _gru_ok() agree with the C envelope."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gru_actions_cases as C  # noqa: E402
import gru_oracle as O  # noqa: E402

CASES = C.all_cases()


def test_case_table():
    ids = [O.cid(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    ht = lambda H: 1 if H <= 16 else 2 if H <= 32 else 4                           # noqa: E731
    it = lambda F: 1 if F + 1 <= 16 else 2 if F + 1 <= 32 else 3 if F + 1 <= 48 else 4   # noqa: E731
    for c in CASES:
        assert c.kind == "softmax" and 17 <= c.A <= 32 and c.H <= 64 and c.F <= 63 and c.T % c.ep == 0
    assert {ht(c.H) for c in C.MATRIX} == {1, 2, 4} and {it(c.F) for c in C.MATRIX} == {1, 2, 3, 4}
    assert {c.A for c in C.MATRIX} == {17, 25, 32}
    assert (C.A17.H, C.A17.F, C.A17.A) == (50, 30, 17) and (C.A32.H, C.A32.F, C.A32.A) == (50, 30, 32)


MEASURED = {"p_min": 1.0, "p_max": 0.0, "band": 0.0, "skipped": 0.0}


@pytest.mark.parametrize("c", CASES, ids=O.cid)
def test_input_set_conditions(c):
    r = C.ref(c)
    exact = O.bf16_exact(r.obs)
    if c.frac == "none":
        assert bool(exact.all())
    elif c.frac == "column":
        assert int((~exact).sum()) == c.T * c.E * c.N and int((~exact).any(0).any(0).any(0).sum()) == 1
    else:
        assert float((~exact).float().mean()) > 0.3
    for padded in (False, True):
        assert r.ambiguous(padded) == 0, f"{r.ambiguous(padded)} ambiguous head-relu pairs: take the next seed"
    for padded in (False, True):
        o = r.out(padded)
        assert bool(torch.isfinite(o).all())
        MEASURED["p_min"] = min(MEASURED["p_min"], o.min().item())
        MEASURED["p_max"] = max(MEASURED["p_max"], o.max().item())
        assert O.P_LO <= o.min().item() and o.max().item() <= 1 - O.P_LO, (padded, o.min().item(), o.max().item())
        skipped = (r.margin(padded) <= O.TIE).float().mean().item()
        MEASURED["skipped"] = max(MEASURED["skipped"], skipped)
        assert skipped <= 0.01, (padded, skipped)
    r64, s64, r32, s32 = r.grads()
    worst = 0.0
    for name in O.NAMES:
        tol = O.GRAD_RTOL * r64[name].abs().max().item() + O.GRAD_ATOL
        band = (r32[name] - r64[name]).abs().max().item()
        worst = max(worst, band / tol)
        assert band <= tol, (name, band, tol)
    MEASURED["band"] = max(MEASURED["band"], worst)
    print(f"  torch fp32 at {worst:.3f} of the gradient tolerance")
    if c.L == 1:
        assert bool((r64["w_hh"] == 0).all())
    acts, lo, W = r.train()
    assert int(acts.max()) >= 16, "no forced id in the second tile"
    ratio = torch.exp(r.logp(r.out(True), acts) - lo.double())
    assert ratio.min().item() < 0.9 and ratio.max().item() > 1.1 or c.T * c.E * c.N < 40
    for edge in O.CLIP_EDGES:
        assert (ratio - edge).abs().min().item() > 5e-4


def test_report_measured():
    """(after the sets above, in file order) the extremes over all sets, for DESIGN.md"""
    print(f"  probabilities in [{MEASURED['p_min']:.4f}, {MEASURED['p_max']:.4f}]; torch fp32 autograd at most "
          f"{MEASURED['band']:.3f} of the gradient tolerance; at most {MEASURED['skipped']:.4f} of a set's "
          f"deterministic decisions within {O.TIE} of a tie")


@pytest.mark.parametrize("c", C.SAMPLER, ids=O.cid)
def test_sampler_sets_cover_the_second_tile(c):
    ids, near = C.sampler_reference(C.ref(c))
    seen = set(ids[~near].tolist())
    assert set(range(16, c.A)) <= seen, sorted(set(range(16, c.A)) - seen)
    assert near.mean() < 0.01


# --------------------------------------------------------------------------------------------- the C envelope

def _lib_and_desc(H, A, kind, F=24, L=3, ep=5, N=2, E=0):
    from d2dhip import _lib
    lib = _lib.load()
    buf = np.zeros(16, dtype=np.float32)
    ptr = buf.ctypes.data
    d = _lib.GruDesc(N, E, F, H, A, kind, L, ep, *([ptr] * 8), 0, 0, None)
    return _lib, lib, d, buf


def _policy_rc(H, A, kind, record=False):
    """d2d_policy_gru with n_envs = 0, n_slots = 0: the checks run, nothing is launched, no pointer is read"""
    _lib, lib, d, buf = _lib_and_desc(H, A, kind)
    sgn = np.zeros(8, dtype=np.uint32)
    if record:
        d.obs_format = _lib.D2D_OBS_U8
        d.obs_signed = sgn.ctypes.data
    p = buf.ctypes.data
    rc = lib.d2d_policy_gru(ctypes.byref(d), 5, p, 0, 0, 0, None, 0, 0, p, p, None)
    return rc, lib.d2d_last_error().decode()


@pytest.mark.parametrize("H", [16, 64])
@pytest.mark.parametrize("A", [17, 32])
def test_envelope_accepts_the_second_tile(H, A):
    rc, msg = _policy_rc(H, A, 1)
    assert rc == 0, msg


@pytest.mark.parametrize("H,A,kind,record,word", [(64, 33, 1, False, "[1,32]"), (64, 17, 0, False, "softmax"),
                                                  (65, 17, 1, False, "hidden"), (64, 17, 1, True, "record")],
                         ids=["A33", "sigmoid-A17", "H65-A17", "record-A17"])
def test_envelope_refuses(H, A, kind, record, word):
    rc, msg = _policy_rc(H, A, kind, record)
    assert rc == -2, (rc, msg)                       # D2D_EUNSUPPORTED
    assert "n_out" in msg and word in msg, msg


def test_envelope_unchanged_up_to_16():
    for kind in (0, 1):
        assert _policy_rc(64, 16, kind)[0] == 0
        assert _policy_rc(100, 16, kind)[0] == 0
    assert _policy_rc(64, 16, 1, record=True)[0] == 0


@pytest.mark.parametrize("H", [16, 32, 64])
def test_grad_workspace_grows_by_the_head_sums(H):
    """n_out = 32 against n_out = 16: per wave 64 (4 HT + 4) more head sums, per agent 16 HW + 16 more head-image
    floats, and the partials' (A H + A) per (workgroup, agent)"""
    T, E, N = 10, 17, 2
    _lib, lib, d16, _b16 = _lib_and_desc(H, 16, 1, E=E, N=N)
    _lib, lib, d32, _b32 = _lib_and_desc(H, 32, 1, E=E, N=N)
    w16 = lib.d2d_gru_grad_workspace(ctypes.byref(d16), T)
    w32 = lib.d2d_gru_grad_workspace(ctypes.byref(d32), T)
    ht = 1 if H <= 16 else 2 if H <= 32 else 4
    tiles = T * ((E + 15) // 16)
    G = max(1, min((256 + N - 1) // N, (tiles + 3) // 4))
    added = G * N * 4 * 64 * (4 * ht + 4) + N * (16 * 16 * ht + 16)
    assert w16 > 0 and w32 >= w16 + added, (w16, w32, added)


# ------------------------------------------------------------------------------------- the Python rule, _gru_ok

SHAPES = [(24, 64, 17, "softmax", 10, False, True), (24, 16, 32, "softmax", 3, False, True),
          (24, 64, 33, "softmax", 3, False, False), (24, 64, 17, "sigmoid", 3, False, False),
          (24, 65, 17, "softmax", 3, False, False), (24, 64, 17, "softmax", 3, True, False),
          (24, 64, 16, "softmax", 3, True, True), (24, 100, 16, "sigmoid", 3, False, True),
          (24, 64, 16, "sigmoid", 3, False, True), (63, 64, 32, "softmax", 3, False, True),
          (64, 64, 17, "softmax", 3, False, False)]


@pytest.mark.parametrize("F,H,A,kind,L,record,want", SHAPES)
def test_supported_agrees_with_the_c_envelope(F, H, A, kind, L, record, want):
    from d2dhip import gru
    assert gru.supported(F, H, A, kind, L, record) is want
    assert gru.supported(F, H, A, gru.KIND[kind], L, record) is want
    if F + 1 <= 64:                                                     # (the helper's dummy desc has F = 24)
        rc, msg = _policy_rc(H, A, gru.KIND[kind], record)
        assert (rc == 0) is want, (rc, msg)
    assert gru.supported(F, H, 1, None, L, record) is (F + 1 <= 64)     # value networks: A does not enter


class _Stub:
    """What _gru_ok / _fused_update_ok / _record_ok read of a learner (a learner itself needs the GPU to be built):
    a ChannelSelectionEnv learner's policy shape, F = deadline 7 + n_channels + 1 inputs, A = n_channels + 1 ids."""

    def __init__(self, n_channels, hidden, useRNN, history_len=10):
        import types
        from algorithms._learner import BatchedLearnerBase as B
        self.useRNN, self.combinatorial, self.kind, self.history_len = useRNN, False, "chsel", history_len
        self.policy = types.SimpleNamespace(kind="rnn" if useRNN else "mlp", F=7 + n_channels + 1, H=hidden,
                                            A=n_channels + 1, N=5)
        self.obs_record = True
        for name in ("_gru_ok", "_fused_ok", "_fused_update_ok", "_record_ok", "_gru_kind"):
            setattr(self, name, getattr(B, name).__get__(self))


@pytest.mark.parametrize("n_channels,hidden,useRNN,want", [(16, 64, True, True), (31, 32, True, True),
                                                           (15, 64, True, True), (16, 80, True, False),
                                                           (32, 64, True, False), (16, 64, False, False)])
def test_gru_ok_follows_the_rule(n_channels, hidden, useRNN, want, monkeypatch):
    from d2dhip import gru
    monkeypatch.delenv("D2D_FUSED_POLICY", raising=False)
    monkeypatch.delenv("D2D_FUSED_UPDATE", raising=False)
    lr = _Stub(n_channels, hidden, useRNN)
    assert bool(lr._gru_ok()) is want
    if useRNN:
        assert want is gru.supported(lr.policy.F, hidden, n_channels + 1, "softmax", lr.history_len)
        assert bool(lr._fused_update_ok()) is want
        rc, msg = _policy_rc(hidden, n_channels + 1, 1)
        assert (rc == 0) is want, (rc, msg)
    assert not lr._record_ok()
