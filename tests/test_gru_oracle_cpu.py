"""The oracle of tests/test_gru_edges_gpu.py, checked on the CPU (tests/gru_oracle.py):

- algorithms._core.gru_window in float64 is torch.nn.GRU(batch_first=True) in float64 with the same weights, to 1e-12
  relative on the last hidden state -- until here the GRU tests' reference was the project's own torch code;
- every input set of the GPU file meets the conditions under which its tests need no fallback branch: every action
  probability in [1e-3, 1 - 1e-3] (the old `well` mask covers every sample), torch float32 autograd within the
  gradient tolerance 2e-5 max|g| + 1e-7 of float64 for all eight tensors (the strict branch is the only branch), no
  ambiguous head-relu pair by the 2 (H + 2) 2^-24 rule, at most 1 % of the deterministic decisions within 1e-5 of a
  tie.  These are conditions on the reference alone, not measurements of a kernel;
- the stride triples d2dhip.gru._strides3 derives for the [N][E*T] layout and for views of wider tensors address the
  elements of the contiguous [T][E][N] tensor.

Measured over the sets (float64 vs float32 torch): see DESIGN.md, "GRU kernels at every instance and edge"."""
import pytest

torch = pytest.importorskip("torch")

import gru_oracle as O  # noqa: E402

CASES = O.all_cases()


def test_case_table_is_consistent():
    ids = [O.cid(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        assert 1 <= c.H <= 64 and 1 <= c.F <= 63 and c.T % c.ep == 0 and c.frac in O.FRAC_MODES
        assert c.L < 65 or (c.E <= 3 and c.T == c.ep), "long windows: E <= 3 and one episode (the reference's cost)"
    # every (HT, IT) instance of both kernels is reached
    ht = lambda H: 1 if H <= 16 else 2 if H <= 32 else 4                           # noqa: E731
    it = lambda F: 1 if F + 1 <= 16 else 2 if F + 1 <= 32 else 3 if F + 1 <= 48 else 4   # noqa: E731
    reached = {(ht(c.H), it(c.F), c.kind) for c in O.MATRIX}
    assert reached == {(h, i, k) for h in (1, 2, 4) for i in (1, 2, 3, 4) for k in O.KINDS}


@pytest.mark.parametrize("c", [O.case("sigmoid", 30, 50), O.case("softmax", 31, 64), O.WINDOW_LONG[0]], ids=O.cid)
def test_gru_window_is_torch_nn_gru(c):
    """one ragged-H set, one H = 64 set, the L = 129 set: every slot's padded and unpadded window"""
    from algorithms._core import gru_window
    r = O.ref(c)
    q = {k: v.double() for k, v in r.p.items()}
    for padded in (False, True):
        for _, x in O.window_groups(r.obs.double(), c.ep, c.L, padded):          # [N][B][S][F]
            ours = gru_window(x, q["w_ih"], q["w_hh"], q["b_ih"], q["b_hh"])
            for k in range(c.N):
                m = torch.nn.GRU(c.F, c.H, 1, batch_first=True).double()
                with torch.no_grad():
                    m.weight_ih_l0.copy_(q["w_ih"][k])
                    m.weight_hh_l0.copy_(q["w_hh"][k])
                    m.bias_ih_l0.copy_(q["b_ih"][k])
                    m.bias_hh_l0.copy_(q["b_hh"][k])
                    _, hn = m(x[k])
                err = (ours[k] - hn[0]).abs().max().item()
                assert err <= 1e-12 * hn.abs().max().item(), (padded, k, err)


MEASURED = {"p_min": 1.0, "p_max": 0.0, "band": 0.0, "skipped": 0.0}


@pytest.mark.parametrize("c", CASES, ids=O.cid)
def test_input_set_conditions(c):
    r = O.ref(c)
    # the inputs are what the set's name says
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
    if c.kind is not None:      # the ratios straddle the clip: both branches of the surrogate's min are taken
        acts, lo, W = r.train()
        ratio = torch.exp(r.logp(r.out(True), acts) - lo.double())
        assert ratio.min().item() < 0.9 and ratio.max().item() > 1.1 or c.T * c.E * c.N < 40
        for edge in O.CLIP_EDGES:
            assert (ratio - edge).abs().min().item() > 5e-4


def test_report_measured():
    """(after the sets above, in file order) the extremes over all sets, for DESIGN.md"""
    print(f"  probabilities in [{MEASURED['p_min']:.4f}, {MEASURED['p_max']:.4f}]; torch fp32 autograd at most "
          f"{MEASURED['band']:.3f} of the gradient tolerance; at most {MEASURED['skipped']:.4f} of a set's "
          f"deterministic decisions within {O.TIE} of a tie")


def test_strides3_address_the_contiguous_elements():
    T, E, N = 6, 5, 3
    ref = torch.arange(T * E * N, dtype=torch.float32).view(T, E, N)
    assert O.strides_address_same(ref, ref)
    # [N][E*T], env-major (the learner's flattened batch)
    ne = ref.permute(2, 1, 0).reshape(N, E * T).contiguous()
    assert O.strides_address_same(ne, ref)
    # a permuted view of an [N][T][E] tensor
    nte = ref.permute(2, 0, 1).contiguous()
    assert O.strides_address_same(nte.permute(1, 2, 0), ref)
    # a view of a wider NaN-filled tensor, at an offset
    wide = torch.full((T, E + 3, N + 2), float("nan"))
    wide[:, 2:2 + E, 1:1 + N] = ref
    assert O.strides_address_same(wide[:, 2:2 + E, 1:1 + N], ref)
    wide2 = torch.full((N + 1, E * T + 7), float("nan"))
    wide2[1:, 3:3 + E * T] = ne
    assert O.strides_address_same(wide2[1:, 3:3 + E * T], ref)
