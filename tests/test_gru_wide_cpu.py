"""The input sets of tests/test_gru_wide_gpu.py (tests/gru_wide_cases.py: hidden sizes 65..128), checked on the CPU
against the oracle of tests/gru_oracle.py, and the C ABI's new hidden bound on a GPU-less host.

- Every set meets the conditions of tests/test_gru_oracle_cpu.py::test_input_set_conditions, under which the GPU file
  needs one strict branch: every action probability in [1e-3, 1 - 1e-3], torch float32 autograd within the gradient
  tolerance 2e-5 max|g| + 1e-7 of float64 for all eight tensors, no ambiguous head-relu pair by the 2 (H + 2) 2^-24
  rule, at most 1 % of the deterministic decisions within 1e-5 of a tie, the surrogate's ratios on both sides of the
  clip and none within 5e-4 of an edge.  These are conditions on the reference alone, not measurements of a kernel.
- The table reaches every hidden tile count HT = 5 .. 8 and every input tile count IT = 1 .. 4 of the wide kernels.
- d2d_gru_carry_floats answers for a hidden-128 desc, and a hidden-129 desc is refused as unsupported with a message
  that names the bound, before any HIP call."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

import gru_oracle as O  # noqa: E402
import gru_wide_cases as W  # noqa: E402

CASES = W.all_cases()


def test_case_table_is_consistent():
    ids = [O.cid(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert not set(ids) & {O.cid(c) for c in O.all_cases()}, "a set of the narrow file (its reference is cached by id)"
    for c in CASES:
        assert 65 <= c.H <= 128 and 1 <= c.F <= 63 and c.T % c.ep == 0 and c.frac in O.FRAC_MODES
        assert c.H < 96 or c.T == c.ep, "H >= 96: one episode (see gru_wide_cases)"
        assert c.L < 64 or (c.E <= 3 and c.T == c.ep), "long windows: E <= 3 and one episode (the reference's cost)"
    reached = {W.tiles(c) for c in CASES}
    assert {ht for ht, _ in reached} == {5, 6, 7, 8} and {it for _, it in reached} == {1, 2, 3, 4}
    assert {(8, it, c.kind) for c in W.MATRIX for it in [W.tiles(c)[1]]} == {(8, i, k) for i in (1, 2, 3, 4) for k in W.KINDS}
    assert {(5, it) for c in W.LOW for it in [W.tiles(c)[1]]} == {(5, i) for i in (1, 2, 3, 4)}
    # ragged tiles: a last hidden tile of 1, 4, 8 and 15 units; a last input tile of 14 and 15 columns
    assert {c.H % 16 for c in CASES} >= {1, 4, 8, 15, 0}
    assert {c.F % 16 for c in CASES} >= {12, 14, 15}


def conditions(c):
    """test_gru_oracle_cpu.py::test_input_set_conditions for one set; returns torch fp32's share of the gradient
    tolerance"""
    r = O.ref(c)
    exact = O.bf16_exact(r.obs)
    if c.frac == "none":
        assert bool(exact.all())
    elif c.frac == "one":
        assert int((~exact).sum()) == 1
    elif c.frac == "column":
        assert int((~exact).sum()) == c.T * c.E * c.N and int((~exact).any(0).any(0).any(0).sum()) == 1
    else:
        assert float((~exact).float().mean()) > 0.3
    for k, d in enumerate(r.dims):
        assert bool((r.obs[:, :, k, d:] == 0).all())
    for padded in (False, True):
        assert r.ambiguous(padded) == 0, f"{r.ambiguous(padded)} ambiguous head-relu pairs: take the next seed"
    for padded in (False, True):
        o = r.out(padded)
        assert bool(torch.isfinite(o).all())
        if c.kind is not None:
            assert O.P_LO <= o.min().item() and o.max().item() <= 1 - O.P_LO, (padded, o.min().item(), o.max().item())
            skipped = (r.margin(padded) <= O.TIE).float().mean().item()
            assert skipped <= 0.01, (padded, skipped)
    r64, s64, r32, s32 = r.grads()
    worst = 0.0
    for name in O.NAMES:
        tol = O.GRAD_RTOL * r64[name].abs().max().item() + O.GRAD_ATOL
        band = (r32[name] - r64[name]).abs().max().item()
        worst = max(worst, band / tol)
        assert band <= tol, (name, band, tol)
    if c.L == 1:
        assert bool((r64["w_hh"] == 0).all())
    if c.kind is not None:      # the ratios straddle the clip: both branches of the surrogate's min are taken
        acts, lo, Wt = r.train()
        ratio = torch.exp(r.logp(r.out(True), acts) - lo.double())
        assert ratio.min().item() < 0.9 and ratio.max().item() > 1.1 or c.T * c.E * c.N < 40
        for edge in O.CLIP_EDGES:
            assert (ratio - edge).abs().min().item() > 5e-4
    return worst


@pytest.mark.parametrize("c", CASES, ids=O.cid)
def test_input_set_conditions(c):
    worst = conditions(c)
    print(f"  torch fp32 at {worst:.3f} of the gradient tolerance")


def _gru_desc(lib_mod, hidden, n_agents=3, n_envs=17, obs_dim=30, n_out=8, kind=0, L=4, ep=20):
    w = ctypes.c_void_p(16)
    return lib_mod.GruDesc(n_agents, n_envs, obs_dim, hidden, n_out, kind, L, ep, w, w, w, w, w, w, w, w, 0, 0, None,
                           lib_mod.D2D_OBS_F32, 0, None)


def test_carry_floats_of_a_wide_desc():
    """(a GPU-less host) the h image of every (agent, 16-env tile): [N][tiles][HT][64] f32x4"""
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    for H, ht in ((128, 8), (100, 7), (65, 5)):
        n = lib.d2d_gru_carry_floats(ctypes.byref(_gru_desc(_lib, H)))
        assert n == 3 * 2 * ht * 64 * 4, (H, n)
    assert lib.d2d_gru_carry_floats(ctypes.byref(_gru_desc(_lib, 129))) == -1
    # the narrow layout is what it was: [N][env tiles][4 HT'][64]
    assert lib.d2d_gru_carry_floats(ctypes.byref(_gru_desc(_lib, 64))) == 3 * 2 * 4 * 4 * 64


def test_hidden_129_is_refused_before_any_hip_call():
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    w = ctypes.c_void_p(16)
    d = _gru_desc(_lib, 129)
    assert lib.d2d_policy_gru(ctypes.byref(d), 20, w, 0, 1, 0, None, 0, 0, w, w, None) == -2     # D2D_EUNSUPPORTED
    assert b"128" in lib.d2d_last_error() and b"129" in lib.d2d_last_error()
    st = (ctypes.c_int64 * 3)(1, 1, 1)
    rc = lib.d2d_gru_grad(ctypes.byref(d), 20, w, w, w, st, w, st, 0.1, 0.01, 1.0, w, w, w, w, w, w, w, w, w, w, 1 << 20,
                          None)
    assert rc == -2 and b"128" in lib.d2d_last_error()
    # inside the envelope the same calls get past the hidden check: a too-long window and a too-small workspace are
    # refused by the wide path's own checks, still before any HIP call
    d = _gru_desc(_lib, 128, L=257, ep=300)
    assert lib.d2d_policy_gru(ctypes.byref(d), 300, w, 0, 1, 0, None, 0, 0, w, w, None) == -2
    assert b"history_len" in lib.d2d_last_error()
    d = _gru_desc(_lib, 128)
    need = lib.d2d_gru_grad_workspace(ctypes.byref(d), 20)
    assert need > 0
    rc = lib.d2d_gru_grad(ctypes.byref(d), 20, w, w, w, st, w, st, 0.1, 0.01, 1.0, w, w, w, w, w, w, w, w, w, w, 16, None)
    assert rc == -1 and b"one tile of every agent" in lib.d2d_last_error()
