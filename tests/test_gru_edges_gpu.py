"""The GRU window kernels (csrc/gru_kernels.hip, gru_common.h) at every template instance, ragged size, input branch
and loop edge, against float64 torch (tests/gru_oracle.py; the input sets and their references are shared with
tests/test_gru_oracle_cpu.py, which asserts on the CPU the conditions that make every comparison here strict).

Shapes are the smallest at which each path exists: N = 2 agents, two 5-slot episodes, 17 envs (a full 16-env tile and
a tile of one), 3-step windows unless the case is about the window; H = 50 / F = 30 is the ragged base case around which
one size at a time varies.  Tolerances are those of tests/test_gru_gpu.py -- values 1e-5 absolute; log-probs 1e-5
absolute (plus two ulps of the fp32 Bernoulli probabilities through log p / log(1 - p)); deterministic actions exact
where the margin exceeds 1e-5 (at most 1 % of a case's decisions may be closer); gradients within 2e-5 max|g| + 1e-7
of float64 autograd; loss sums rtol 1e-5, atol 1e-4 -- with no fallback: no fp32-band branch and no mask that drops
samples.  Every output, and every input but the parameters, lives inside a 0xFF-filled (NaN) guarded buffer; every
guard must be intact and every output finite.  Each test prints max |kernel - f64| beside torch fp32's own distance.

What this file found (fixed with it): d2d_gru_grad with T = 0 or n_envs = 0 wrote its images and N * P zeros into a
workspace for which d2d_gru_grad_workspace asks 0 floats; it now zeroes the outputs themselves and returns, and
d2dhip.gru.grads no longer divides by T * E = 0.  With N = 0 it divided by N before its early return.  And
gru_grad_kernel<4, 3> / <4, 4> (H > 32, F >= 32, fp32 rows) returned garbage for any window holding a bf16-inexact
input: their generated code read an accumulator straight after the MFMA that writes it (test_grads_fractional_inputs;
DESIGN.md 6.3).  Every instance that keeps the per-step exact / inexact branch runs its inexact side here (FRAC_LOW)."""
import contextlib
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gru_oracle as O  # noqa: E402
from mlp_oracle import to_record  # noqa: E402

DEV = "cuda"
RNG = dict(seed=1234, env_base=77, rng_step=5)


@contextlib.contextmanager
def option(opt, value):
    from d2dhip import _lib
    lib = _lib.require_gpu()
    lib.d2d_set_option(opt, value)
    try:
        yield
    finally:
        lib.d2d_set_option(opt, 0)


def impl_option(impl):
    from d2dhip import _lib
    return option(_lib.D2D_OPT_POLICY_F32_MFMA, 1 if impl == "f32" else 0)


def impls(c):
    """the policy's split kernel exists for F + 1 <= 32 (IT <= 2); wider inputs run the fp32-MFMA kernel either way"""
    return ("split", "f32") if c.F + 1 <= 32 else ("f32",)


def with_impls(cases):
    return [pytest.param(c, i, id=f"{O.cid(c)}-{i}") for c in cases for i in impls(c)]


def params_dev(r):
    return {k: v.to(DEV).contiguous() for k, v in r.p.items()}


def obs_dev(r, fmt="f32", obs=None):
    """(obs argument, guard check): fp32 rows or the compact record, NaN / 0xFF rows before and after"""
    from d2dhip.record import ObsRecord
    obs = r.obs if obs is None else obs
    if fmt == "f32":
        return O.guarded(src=obs.contiguous())
    rec = to_record(obs)
    data, chk = O.guarded(src=rec.data)
    return ObsRecord(data, rec.obs_dim, rec.signed), chk


def act_dtype(c):
    return torch.uint8 if (c.kind == "softmax" or c.A <= 8) else torch.int16


def pack_actions(c, acts):
    """[N][T][E](A) reference actions -> the kernels' [T][E][N] masks / ids (CPU)"""
    from d2dhip.envbatch import pack_masks_torch
    if c.kind == "sigmoid":
        return pack_masks_torch(acts.permute(1, 2, 0, 3))
    return acts.permute(1, 2, 0).to(torch.uint8).contiguous()


def unpack_actions(c, a_te):
    """the kernels' [n][E][N] masks / ids -> [N][n][E](A) (CPU; double bits / int64 ids)"""
    a = a_te.cpu().to(torch.int64).permute(2, 0, 1)
    if c.kind == "sigmoid":
        return (((a & 0xFFFF).unsqueeze(-1) >> torch.arange(c.A)) & 1).double()
    return a


def run_policy(r, pd, od, slot0, n, padded=False, forced=None, deterministic=False, sample=False, hcarry=None,
               carry_in=False):
    """One d2d_policy_gru launch on guarded buffers -> (actions [n][E][N] or None, out [N][n * E]), both on the device"""
    from d2dhip import gru
    c = r.c
    out, chk_out = O.guarded(shape=(c.N, n * c.E), dtype=torch.float32)
    checks = [(chk_out, "out")]
    kw = {}
    if c.kind is not None:
        act, chk_act = O.guarded(shape=(n, c.E, c.N), dtype=act_dtype(c))
        checks.append((chk_act, "actions_out"))
        kw["actions_out"] = act
        if forced is not None:
            f, chk_f = O.guarded(src=forced.to(DEV))
            checks.append((chk_f, "forced"))
            kw["forced"] = f
        if sample:
            kw.update(RNG)
        kw["deterministic"] = deterministic
    if hcarry is not None:
        kw.update(hcarry=hcarry, carry_in=carry_in)
    res = gru.policy(pd, od, c.kind, c.L, c.ep, slot0, n, padded=padded, out=out, **kw)
    torch.cuda.synchronize()
    for chk, what in checks:
        chk(what)
    assert bool(torch.isfinite(out).all()), "an output was not written (NaN) or is not finite"
    if c.kind is None:
        return None, res
    acts = res[0]
    if c.kind == "softmax":
        assert int(acts.max()) < c.A, "an action id was not written"
    elif c.A < 8 * acts.element_size():
        assert int((acts.to(torch.int64) & 0xFFFF).max()) < (1 << c.A), "an action mask was not written"
    return acts, res[1]


def lp_tol(c, probs):
    """1e-5, and for Bernoulli two ulps of the fp32 probabilities through log p / log(1 - p) (test_gru_gpu.py)"""
    tol = torch.full(probs.shape[:3], 1e-5, dtype=torch.float64)
    if c.kind == "sigmoid":
        tol = torch.maximum(tol, (2 * 2.0 ** -23 * probs / torch.minimum(probs, 1 - probs)).mean(-1))
    return tol


def check_logp(r, lp_dev, acts, padded, slots, what):
    """lp_dev [N][n * E] of slots [s0, s1) against float64, for actions acts [N][n][E](A)"""
    c = r.c
    s0, s1 = slots
    probs = r.out(padded)[:, s0:s1]
    want = r.logp(probs, acts)
    lp32 = r.logp(r.out(padded, torch.float32)[:, s0:s1], acts)
    got = lp_dev.view(c.N, s1 - s0, c.E).cpu().double()
    err = (got - want).abs()
    print(f"  {what}: max |kernel - f64| {err.max().item():.2e}  |torch fp32 - f64| {(lp32 - want).abs().max().item():.2e}")
    tol = lp_tol(c, probs)
    assert bool((err <= tol).all()), (what, err.max().item(), (err / tol).max().item())


def check_values(r, v_dev, padded, slots, what):
    c = r.c
    s0, s1 = slots
    want = r.out(padded)[:, s0:s1]
    got = v_dev.view(c.N, s1 - s0, c.E).cpu().double()
    err = (got - want).abs().max().item()
    band = (r.out(padded, torch.float32)[:, s0:s1] - want).abs().max().item()
    print(f"  {what}: max |kernel - f64| {err:.2e}  |torch fp32 - f64| {band:.2e}")
    assert err <= 1e-5, (what, err)


def check_deterministic(r, acts_dev, padded, slots, what):
    from d2dhip.envbatch import pack_masks_torch
    c = r.c
    s0, s1 = slots
    probs = r.out(padded)[:, s0:s1]
    if c.kind == "sigmoid":
        want = pack_masks_torch((probs > 0.5).permute(1, 2, 0, 3))                     # [n][E][N]
    else:
        want = probs.argmax(-1).permute(1, 2, 0).to(torch.uint8)
    clear = (r.margin(padded)[:, s0:s1] > O.TIE).permute(1, 2, 0)
    assert (~clear).float().mean().item() <= 0.01
    assert torch.equal(acts_dev.cpu()[clear], want[clear]), what


def policy_all(r, fmt="f32"):
    """The three modes of one input set on the current policy kernel: the forced log-probs of the padded training
    windows; the rollout's sampled actions with their log-probs (bitwise those of the forced re-evaluation, and within
    tolerance of float64); the deterministic actions.  Value networks: the padded and the unpadded values."""
    c = r.c
    pd = params_dev(r)
    od, chk_obs = obs_dev(r, fmt)
    T = c.T
    if c.kind is None:
        for padded in (True, False):
            _, v = run_policy(r, pd, od, 0, T, padded=padded)
            check_values(r, v, padded, (0, T), "padded" if padded else "unpadded")
        chk_obs("obs")
        return
    forced = pack_actions(c, r.actions())
    acts, lp = run_policy(r, pd, od, 0, T, padded=True, forced=forced)
    assert torch.equal(acts.cpu(), forced)
    check_logp(r, lp, r.actions(), True, (0, T), "forced, padded")
    a_s, lp_s = run_policy(r, pd, od, 0, T, sample=True)
    a_f, lp_f = run_policy(r, pd, od, 0, T, forced=a_s)
    assert torch.equal(a_f, a_s) and torch.equal(lp_f, lp_s), "the forced re-evaluation of sampled actions"
    check_logp(r, lp_s, unpack_actions(c, a_s), False, (0, T), "sampled, unpadded")
    a_d, _ = run_policy(r, pd, od, 0, T, deterministic=True)
    check_deterministic(r, a_d, False, (0, T), "deterministic, unpadded")
    a_d, _ = run_policy(r, pd, od, 0, T, padded=True, deterministic=True)
    check_deterministic(r, a_d, True, (0, T), "deterministic, padded")
    chk_obs("obs")


# ---------------------------------------------------------------------------------------------------- policy

@pytest.mark.parametrize("c,impl", with_impls([c for c in O.MATRIX if c.F != 47]))
def test_policy_instance_matrix(c, impl):
    """(HT, IT) in {1, 2, 4}^2 x kind x mode, on tile boundaries: H = 16 / 32 / 64, F + 1 = 16 / 32 / 64"""
    with impl_option(impl):
        policy_all(O.ref(c))


@pytest.mark.parametrize("c,impl", with_impls(O.RAGGED))
def test_policy_ragged_sizes(c, impl):
    """H, F, per-agent in_dims, A, E, N = 1: one size at a time off the ragged base case (H = 50, F = 30, E = 17)"""
    with impl_option(impl):
        policy_all(O.ref(c))


@pytest.mark.parametrize("c,impl", with_impls(O.FRAC + O.FRAC_LOW))
def test_policy_input_branches(c, impl):
    """fp32 rows that are bf16-exact in every step, in no step, in all but one step of one tile, and in no step
    through one column (x_exact_step is a wave-wide ballot per window step)"""
    with impl_option(impl):
        policy_all(O.ref(c))


@pytest.mark.parametrize("c,impl", with_impls([c for c in O.FRAC + O.BASE_CASES if c.frac == "none"]))
def test_policy_record_input(c, impl):
    """the same integer data as the compact record"""
    with impl_option(impl):
        policy_all(O.ref(c), "record")


@pytest.mark.parametrize("c,impl", with_impls(O.WINDOW))
def test_policy_window_thresholds(c, impl):
    """L = 64 / 65 (the last window on the LDS padding table / the first on the global one), 129, L > episode, L = 1;
    padded and unpadded, at ragged H"""
    with impl_option(impl):
        policy_all(O.ref(c))


@pytest.mark.parametrize("kind", O.KINDS, ids=lambda k: k or "value")
def test_policy_long_padded_window_under_graph_capture(kind):
    """While a stream is capturing, a padded window past the LDS table runs its padding steps per tile instead of
    allocating the global table: the replay of the (single-kernel) graph equals the eager launch bit for bit."""
    from d2dhip import gru
    c = O.case(kind, 30, 50, L=65, ep=6, T=6, E=3)
    r = O.ref(c)
    pd = params_dev(r)
    od, chk_obs = obs_dev(r)
    forced = None if kind is None else pack_actions(c, r.actions())
    _, eager = run_policy(r, pd, od, 0, c.T, padded=True, forced=forced)
    eager = eager.clone()
    out, chk_out = O.guarded(shape=(c.N, c.T * c.E), dtype=torch.float32)
    kw = {} if kind is None else dict(forced=forced.to(DEV), want_actions=False)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gru.policy(pd, od, kind, c.L, c.ep, 0, c.T, padded=True, out=out, **kw)
    graph.replay()
    torch.cuda.synchronize()
    chk_out("out")
    chk_obs("obs")
    assert torch.equal(out, eager)


def slot_outputs(r, pd, od, slot0, n, padded):
    """(forced log-probs or values, deterministic actions) of one launch over slots [slot0, slot0 + n)"""
    c = r.c
    if c.kind is None:
        return run_policy(r, pd, od, slot0, n, padded=padded)[1], None
    forced = pack_actions(c, r.actions())[slot0:slot0 + n]
    _, lp = run_policy(r, pd, od, slot0, n, padded=padded, forced=forced)
    a_d, _ = run_policy(r, pd, od, slot0, n, padded=padded, deterministic=True)
    return lp, a_d


def per_slot_outputs(r, pd, od, slot0, n, padded):
    c = r.c
    outs = [slot_outputs(r, pd, od, t, 1, padded) for t in range(slot0, slot0 + n)]
    lp = torch.cat([o[0] for o in outs], 1)
    return lp, None if c.kind is None else torch.cat([o[1] for o in outs], 0)


def assert_same_launches(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: log-probs / values"
    if a[1] is not None:
        assert torch.equal(a[1], b[1]), f"{what}: actions"


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("c,impl", with_impls(O.BASE_CASES))
def test_policy_slot_ranges(c, impl, padded):
    """slot0 > 0 with n_slots > 1 across the episode boundary (slots 3 .. 6 of two 5-slot episodes) and all slots in
    one launch (20 tiles: 256-thread workgroups) equal one launch per slot (2 tiles: 512-thread) bit for bit, and
    float64 within tolerance"""
    r = O.ref(c)
    with impl_option(impl):
        pd = params_dev(r)
        od, chk_obs = obs_dev(r)
        each = per_slot_outputs(r, pd, od, 0, c.T, padded)
        assert_same_launches(slot_outputs(r, pd, od, 0, c.T, padded), each, "all slots")
        part = slot_outputs(r, pd, od, 3, 4, padded)
        sl = slice(3 * c.E, 7 * c.E)
        assert_same_launches(part, (each[0][:, sl], None if each[1] is None else each[1][3:7]), "slots 3 .. 6")
        if c.kind is None:
            check_values(r, part[0], padded, (3, 7), "slots 3 .. 6")
        else:
            check_logp(r, part[0], r.actions()[:, 3:7], padded, (3, 7), "slots 3 .. 6")
        chk_obs("obs")


@pytest.mark.parametrize("N,E,n", [(1, 15, 4), (1, 15, 5), (2, 80, 5)], ids=["N1-4tiles", "N1-5tiles", "N2-E80"])
@pytest.mark.parametrize("impl", ["split", "f32"])
def test_policy_launch_shape(N, E, n, impl):
    """The two sides of the 256-thread switch (N * gy < 256 and more than 4 tiles): one agent with 4 and with 5 tiles,
    and two agents with 50: each equals its per-slot evaluation bit for bit"""
    c = O.case("sigmoid", 30, 50, E=E, N=N, T=5 if E == 80 else None)
    r = O.ref(c)
    with impl_option(impl):
        pd = params_dev(r)
        od, chk_obs = obs_dev(r)
        for padded in (False, True):
            assert_same_launches(slot_outputs(r, pd, od, 0, n, padded), per_slot_outputs(r, pd, od, 0, n, padded),
                                 f"{n} slots")
        chk_obs("obs")


@pytest.mark.parametrize("c,impl", with_impls(O.BASE_CASES))
def test_policy_poisoned_neighbour(c, impl):
    """Changing env e's obs changes env e's outputs only: every other env's are the same bits (e = 5 inside the full
    tile, e = 16 the ragged tile's only env)"""
    r = O.ref(c)
    with impl_option(impl):
        pd = params_dev(r)
        od, _ = obs_dev(r)
        base = slot_outputs(r, pd, od, 0, c.T, False)
        for e in (5, 16):
            obs2 = r.obs.clone()
            obs2[:, e] = (obs2[:, e] + 1.0) * (obs2[:, e] != 0)       # (columns past in_dims stay zero)
            od2, _ = obs_dev(r, obs=obs2)
            got = slot_outputs(r, pd, od2, 0, c.T, False)
            keep = torch.ones(c.E, dtype=torch.bool)
            keep[e] = False
            a, b = base[0].view(c.N, c.T, c.E), got[0].view(c.N, c.T, c.E)
            assert torch.equal(a[:, :, keep], b[:, :, keep]), e
            assert not torch.equal(a[:, :, e], b[:, :, e]), e
            if base[1] is not None:
                assert torch.equal(base[1][:, keep], got[1][:, keep]), e


@pytest.mark.parametrize("deterministic", [False, True], ids=["sample", "deterministic"])
@pytest.mark.parametrize("c,impl", with_impls([O.case("sigmoid", 30, 50), O.case("softmax", 30, 10),
                                               O.case(None, 30, 50), O.case("sigmoid", 30, 50, L=8)]))
def test_policy_carry_at_ragged_hidden(c, impl, deterministic):
    """tests/test_gru_gpu.py::test_gru_carried_state_equals_recompute's loop at H = 50 and H = 10, the carried state in
    a guarded buffer of exactly carry_floats elements"""
    from d2dhip import gru
    r = O.ref(c)
    with impl_option(impl):
        pd = params_dev(r)
        od, chk_obs = obs_dev(r)
        hc, chk_hc = O.guarded(shape=(gru.carry_floats(pd, c.E, c.L, c.ep),), dtype=torch.float32)
        kw = dict(seed=77, env_base=5, deterministic=deterministic)
        for t in range(c.T):
            pos = t % c.ep
            cin = 1 <= pos < c.L
            if c.kind is None:
                v0 = gru.policy(pd, od, None, c.L, c.ep, t, 1)
                v1 = gru.policy(pd, od, None, c.L, c.ep, t, 1, hcarry=hc, carry_in=cin)
                assert torch.equal(v0, v1), f"value, slot {t}"
            else:
                a0, l0 = gru.policy(pd, od, c.kind, c.L, c.ep, t, 1, rng_step=3 + t, **kw)
                a1, l1 = gru.policy(pd, od, c.kind, c.L, c.ep, t, 1, rng_step=3 + t, hcarry=hc, carry_in=cin, **kw)
                assert torch.equal(a0, a1), f"actions, slot {t}"
                assert torch.equal(l0, l1), f"log-probs, slot {t}"
        torch.cuda.synchronize()
        chk_hc("hcarry")
        chk_obs("obs")


# ------------------------------------------------------------------------------------------------------ grad

def grad_option(history):
    from d2dhip import _lib
    return option(_lib.D2D_OPT_GRU_GRAD_HISTORY, 1 if history else 0)


def per_sample(x_nte, layout):
    """A per-sample input [N][T][E] (CPU) on the device as contiguous [T][E][N] ("ten"), as [N][E*T] env-major ("net"),
    or as a non-contiguous [T][E][N] view of a wider NaN-filled tensor ("view"); always inside a guarded buffer"""
    N, T, E = x_nte.shape
    if layout == "ten":
        return O.guarded(src=x_nte.permute(1, 2, 0).contiguous())
    if layout == "net":
        return O.guarded(src=x_nte.permute(0, 2, 1).reshape(N, E * T).contiguous())
    wide, chk = O.guarded(shape=(T, E + 3, N + 2), dtype=torch.float32)
    v = wide[:, 2:2 + E, 1:1 + N]
    v.copy_(x_nte.permute(1, 2, 0))
    return v, chk


def run_grads(r, fmt="f32", history=False, clip=0.1, beta=0.05, scale=None, layout="ten"):
    """One d2d_gru_grad launch on guarded buffers -> ({name: gradient}, stats [N][2]) on the device"""
    from d2dhip import gru
    c = r.c
    pd = params_dev(r)
    od, chk_obs = obs_dev(r, fmt)
    acts, lo, W = r.train()
    checks = [(chk_obs, "obs")]
    W_d, chk = per_sample(W, layout)
    checks.append((chk, "weight"))
    kw = {}
    if c.kind is not None:
        lo_d, chk = per_sample(lo, layout)
        checks.append((chk, "logp_old"))
        a_d, chk = O.guarded(src=pack_actions(c, acts))
        checks.append((chk, "actions"))
        kw = dict(actions=a_d, logp_old=lo_d)
    grads = {}
    for name in O.NAMES:
        grads[name], chk = O.guarded(shape=tuple(r.p[name].shape), dtype=torch.float32)
        checks.append((chk, "g_" + name))
    stats, chk = O.guarded(shape=(c.N, 2), dtype=torch.float32)
    checks.append((chk, "stats"))
    with grad_option(history):
        gru.grads(pd, od, c.kind, c.L, c.ep, W_d, clip=clip, beta=beta, scale=scale, grads=grads, stats=stats, **kw)
        torch.cuda.synchronize()
    for chk, what in checks:
        chk(what)
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()), f"g_{name}: not written (NaN) or not finite"
    assert bool(torch.isfinite(stats[:, :1 if c.kind is None else 2]).all()), "stats"
    return grads, stats


def check_grads(r, got, stats, clip=0.1, beta=0.05, factor=1.0, what=""):
    """all eight tensors within 2e-5 max|g| + 1e-7 of float64 autograd (of the mean loss times `factor`), both loss sums
    rtol 1e-5 / atol 1e-4; exact zeros where the gradient is structurally zero"""
    c = r.c
    r64, s64, r32, _ = r.grads(clip, beta)
    bad = []
    for name in O.NAMES:
        want = r64[name] * factor
        scale = want.abs().max().item()
        err = (got[name].cpu().double() - want).abs().max().item()
        band = (r32[name] * factor - want).abs().max().item()
        tol = O.GRAD_RTOL * scale + O.GRAD_ATOL
        print(f"  {what}{name}: max|g| {scale:.3e}  |kernel-f64| {err:.2e}  |torchf32-f64| {band:.2e}  tol {tol:.2e}")
        if err > tol:
            bad.append((name, err, tol))
    assert not bad, bad
    for k, d in enumerate(r.dims):
        assert bool((got["w_ih"][k, :, d:] == 0).all()), "w_ih columns past the agent's in_dim"
    if c.L == 1:
        assert bool((got["w_hh"] == 0).all()), "history_len 1: W_hh never enters the graph"
    st = stats.cpu().double()
    torch.testing.assert_close(st[:, 0], s64[:, 0], rtol=1e-5, atol=1e-4)
    if c.kind is not None:
        torch.testing.assert_close(st[:, 1], s64[:, 1], rtol=1e-5, atol=1e-4)


def grad_case(c, fmt, history=False):
    r = O.ref(c)
    got, stats = run_grads(r, fmt, history)
    check_grads(r, got, stats)


def fmt_params(cases, fmts):
    """fmt "record": the cooperative kernel where H > 32 and F + 1 <= 48, else the row-history kernel on the record;
    "record-history": the record through the row-history kernel where the cooperative one would run"""
    out = []
    for c in cases:
        for f in fmts:
            if f != "f32" and c.frac != "none":
                continue
            if f == "record-history" and not (c.H > 32 and c.F + 1 <= 48):
                continue
            out.append(pytest.param(c, f, id=f"{O.cid(c)}-{f}"))
    return out


@pytest.mark.parametrize("c,fmt", fmt_params(O.MATRIX, ("f32", "record", "record-history")))
def test_grads_instance_matrix(c, fmt):
    """(HT, IT) in {1, 2, 4} x {1, 2, 3, 4} x kind on fp32 rows and on the record: at H = 64 the cooperative kernel
    (IT <= 3), the row-history kernel by option, and the record at IT = 4"""
    grad_case(c, "record" if fmt != "f32" else "f32", fmt == "record-history")


@pytest.mark.parametrize("c,fmt", fmt_params(O.RAGGED, ("f32", "record")))
def test_grads_ragged_sizes(c, fmt):
    """as the policy's, around the same base case; the record at H in (32, 64) runs the cooperative kernel with a
    partly filled (H = 50, 63), a barely used (H = 33) and an empty fourth tile (H = 48)"""
    grad_case(c, fmt)


@pytest.mark.parametrize("c", [c for c in O.FRAC + O.FRAC_WIDE + O.FRAC_LOW if c.frac != "none"], ids=O.cid)
def test_grads_fractional_inputs(c):
    """The xfrac branch: fp32 rows that are not bf16-exact take two more MFMAs per dW_ih tile, chosen by a wave-wide
    ballot per step.  "column" (1/3 in one column of every sample) is the pattern whose truncation adds up coherently:
    without the extra products dW_ih is 1e-4 of max|g| off.  At IT = 1 (F = 12), IT = 3 (F = 40) and IT = 4 (F = 63), all
    with HT = 4: the (4, 3) and (4, 4) instances returned garbage for any window holding an inexact input until their
    per-step branch was taken out (gru_kernels.hip, kSixProducts); and at every other (HT, IT), which keep the branch
    (FRAC_LOW: H = 16 and 32 at F = 12, 30, 40, 63, and H = 50 at F = 30)."""
    grad_case(c, "f32")


@pytest.mark.parametrize("c,fmt", fmt_params(O.WINDOW, ("f32", "record", "record-history")))
def test_grads_flush_edges(c, fmt):
    """L = 64 (one accumulation chain), 65 (a flush after the first step's chain) and 129 (two flushes): the cooperative
    kernel's LONGW instances on the record, the row-history kernel on both formats; L > episode and L = 1"""
    grad_case(c, "record" if fmt != "f32" else "f32", fmt == "record-history")


@pytest.mark.parametrize("layout", ["ten", "net", "view"])
@pytest.mark.parametrize("c", O.BASE_CASES, ids=O.cid)
def test_grads_arguments(c, layout):
    """weight / logp_old as contiguous [T][E][N], as [N][E*T] and as a strided view of a wider NaN-filled tensor;
    scale = 0.37 / (T E), beta = 0, clip = 0.2"""
    r = O.ref(c)
    got, stats = run_grads(r, "f32", clip=0.2, beta=0.0, scale=0.37 / (c.T * c.E), layout=layout)
    check_grads(r, got, stats, clip=0.2, beta=0.0, factor=0.37)


@pytest.mark.parametrize("fmt", ["f32", "record", "record-history"])
@pytest.mark.parametrize("c", O.BASE_CASES, ids=O.cid)
def test_grads_workspace_and_determinism(c, fmt):
    """The shared workspace filled with NaN before a launch: the results are finite (nothing is read that the launch
    did not write), and bitwise those of a second launch and of a launch after a zero fill"""
    from d2dhip import gru
    r = O.ref(c)
    rec, hist = fmt != "f32", fmt == "record-history"
    run_grads(r, "record" if rec else "f32", hist)                 # sizes gru._ws for this launch
    runs = []
    for fill in (float("nan"), None, 0.0):
        if fill is not None:
            gru._ws.buf.fill_(fill)
        g, s = run_grads(r, "record" if rec else "f32", hist)
        runs.append(({k: v.clone() for k, v in g.items()}, s.clone()))
    for g, s in runs[1:]:
        for name in O.NAMES:
            assert torch.equal(g[name], runs[0][0][name]), name
        assert torch.equal(s[:, :1 if c.kind is None else 2], runs[0][1][:, :1 if c.kind is None else 2])
    check_grads(r, *runs[0])


# ----------------------------------------------------------------------------------------------- empty batches

@pytest.mark.parametrize("fmt", ["f32", "record"])
@pytest.mark.parametrize("kind", O.KINDS, ids=lambda k: k or "value")
@pytest.mark.parametrize("T,E", [(0, 17), (10, 0), (0, 0)])
def test_grads_empty_batch(T, E, kind, fmt):
    """T = 0 or E = 0: d2d_gru_grad_workspace asks for 0 floats, d2d_gru_grad returns OK, every gradient and loss sum is
    an exact zero, and nothing outside the outputs is written -- not the one-float NaN workspace either"""
    from d2dhip import _lib, gru
    from d2dhip.record import ObsRecord
    c = O.case(kind, 30, 50)
    r = O.ref(c)
    pd = params_dev(r)
    obs = torch.zeros((T, E, c.N, c.F))
    od = obs.to(DEV) if fmt == "f32" else to_record(obs)
    assert isinstance(od, ObsRecord) == (fmt == "record")
    lib = _lib.require_gpu()
    d = gru.desc(pd, E, gru.KIND[kind], c.L, c.ep)
    gru.set_format(d, od)
    assert lib.d2d_gru_grad_workspace(ctypes.byref(d), T) == 0
    ws, chk_ws = O.guarded(shape=(1,), dtype=torch.float32)
    grads, checks = {}, [(chk_ws, "workspace")]
    for name in O.NAMES:
        grads[name], chk = O.guarded(shape=tuple(r.p[name].shape), dtype=torch.float32)
        checks.append((chk, "g_" + name))
    stats, chk = O.guarded(shape=(c.N, 2), dtype=torch.float32)
    checks.append((chk, "stats"))
    W = torch.zeros((T, E, c.N), device=DEV)
    kw = {} if kind is None else dict(actions=torch.zeros((T, E, c.N), dtype=torch.uint8, device=DEV), logp_old=W)
    saved = gru._ws.buf
    gru._ws.buf = ws
    try:
        gru.grads(pd, od, kind, c.L, c.ep, W, grads=grads, stats=stats, **kw)      # raises unless D2D_OK
        torch.cuda.synchronize()
        assert gru._ws.buf is ws, "the launch did not run on the guarded one-float workspace"
    finally:
        gru._ws.buf = saved
    for chk, what in checks:
        chk(what)
    assert bool(torch.isnan(ws).all()), "the workspace was written"
    for name in O.NAMES:
        assert bool((grads[name] == 0).all()), name
    assert bool((stats == 0).all())


@pytest.mark.parametrize("kind", O.KINDS, ids=lambda k: k or "value")
def test_no_agents_and_no_slots(kind):
    """N = 0 (grads and policy) and n_slots = 0 (policy): OK, and the outputs handed in are untouched"""
    from d2dhip import gru
    c = O.case(kind, 30, 50)
    r = O.ref(c)
    pd = params_dev(r)
    od, chk_obs = obs_dev(r)
    out, chk_out = O.guarded(shape=(c.N, c.E), dtype=torch.float32)
    act, chk_act = O.guarded(shape=(1, c.E, c.N), dtype=act_dtype(c))
    kw = {} if kind is None else dict(actions_out=act)
    gru.policy(pd, od, kind, c.L, c.ep, 2, 0, out=out, **kw)                         # n_slots = 0
    p0 = {k: v[:0].contiguous() for k, v in pd.items()}                               # N = 0
    obs0 = torch.zeros((c.T, c.E, 0, c.F), device=DEV)
    gru.policy(p0, obs0, kind, c.L, c.ep, 0, c.T, out=out, **kw)
    grads = {}
    checks = [(chk_out, "out"), (chk_act, "actions_out"), (chk_obs, "obs")]
    for name in O.NAMES:
        grads[name], chk = O.guarded(shape=tuple(r.p[name].shape), dtype=torch.float32)
        checks.append((chk, "g_" + name))
    stats, chk = O.guarded(shape=(c.N, 2), dtype=torch.float32)
    checks.append((chk, "stats"))
    W = torch.zeros((c.T, c.E, 0), device=DEV)
    gkw = {} if kind is None else dict(actions=torch.zeros((c.T, c.E, 0), dtype=torch.uint8, device=DEV), logp_old=W)
    gru.grads(p0, obs0, kind, c.L, c.ep, W, grads=grads, stats=stats, **gkw)
    torch.cuda.synchronize()
    for chk, what in checks:
        chk(what)
    for t in [out, stats] + list(grads.values()):
        assert bool(torch.isnan(t).all()), "an output was written"
    assert bool((act.view(torch.uint8) == 0xFF).all()), "actions_out was written"
