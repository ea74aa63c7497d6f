"""The categorical GRU head with 17..32 ids -- the second action tile of csrc/gru_kernels.hip (gru_policy_kernel /
gru_grad_kernel with AT = 2, policy_epilogue_cat2, ppo_dz_cat2) -- against float64 torch, with the checks, tolerances
and guarded buffers of tests/test_gru_edges_gpu.py (whose helpers run here unchanged): log-probs 1e-5 absolute;
deterministic ids exact where the margin exceeds 1e-5 (at most 1 % of a set's decisions may be closer); all eight
gradient tensors within 2e-5 max|g| + 1e-7 of float64 autograd; loss sums rtol 1e-5 / atol 1e-4; every output finite
and every guard intact; no fallback branch.  The input sets are tests/gru_actions_cases.py's, whose conditions
tests/test_gru_actions_cpu.py asserts on the CPU.  Each test prints max |kernel - f64| beside torch fp32's distance.

There is no hook that reports which instantiation a call ran, so no test here asserts that A <= 16 stays on the
one-tile kernels; tests/test_gru_edges_gpu.py runs those shapes, and the one-tile kernels' code is unchanged."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gru_actions_cases as C  # noqa: E402
import gru_oracle as O  # noqa: E402
import test_gru_edges_gpu as G  # noqa: E402  (helpers only: nothing of it is collected or changed here)

DEV = "cuda"


def with_impls(cases):
    return [pytest.param(c, i, id=f"{O.cid(c)}-{i}") for c in cases for i in G.impls(c)]


# ---------------------------------------------------------------------------------------------------- policy

@pytest.mark.parametrize("c,impl", with_impls(C.MATRIX + C.INPUTS + C.WINDOWS + C.BATCH))
def test_policy(c, impl):
    """forced log-probs of the padded windows; sampled actions with log-probs, re-evaluated in forced mode bit for
    bit; deterministic ids, padded and unpadded -- on the split kernel and on the fp32-MFMA kernel where both exist"""
    with G.impl_option(impl):
        G.policy_all(C.ref(c))


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("c,impl", with_impls([C.A17, C.A32]))
def test_policy_slot_ranges(c, impl, padded):
    """one launch over all slots equals one launch per slot, bit for bit"""
    r = C.ref(c)
    with G.impl_option(impl):
        pd = G.params_dev(r)
        od, chk_obs = G.obs_dev(r)
        each = G.per_slot_outputs(r, pd, od, 0, c.T, padded)
        G.assert_same_launches(G.slot_outputs(r, pd, od, 0, c.T, padded), each, "all slots")
        part = G.slot_outputs(r, pd, od, 3, 4, padded)
        G.assert_same_launches(part, (each[0][:, 3 * c.E:7 * c.E], each[1][3:7]), "slots 3 .. 6")
        G.check_logp(r, part[0], r.actions()[:, 3:7], padded, (3, 7), "slots 3 .. 6")
        chk_obs("obs")


@pytest.mark.parametrize("deterministic", [False, True], ids=["sample", "deterministic"])
@pytest.mark.parametrize("c,impl", with_impls([C.DRIVER]))
def test_policy_carried_state(c, impl, deterministic):
    """d2d_policy_gru_carry through two 12-slot episodes of the driver's 10-step window: bitwise the recompute's ids
    and log-probs; the carried state in a guarded buffer of exactly carry_floats elements"""
    from d2dhip import gru
    r = C.ref(c)
    with G.impl_option(impl):
        pd = G.params_dev(r)
        od, chk_obs = G.obs_dev(r)
        hc, chk_hc = O.guarded(shape=(gru.carry_floats(pd, c.E, c.L, c.ep),), dtype=torch.float32)
        kw = dict(seed=77, env_base=5, deterministic=deterministic)
        obs2 = torch.cat([od, od], 0)                                   # two episodes
        for t in range(2 * c.T):
            cin = 1 <= t % c.ep < c.L
            a0, l0 = gru.policy(pd, obs2, c.kind, c.L, c.ep, t, 1, rng_step=3 + t, **kw)
            a1, l1 = gru.policy(pd, obs2, c.kind, c.L, c.ep, t, 1, rng_step=3 + t, hcarry=hc, carry_in=cin, **kw)
            assert torch.equal(a0, a1), f"ids, slot {t}"
            assert torch.equal(l0, l1), f"log-probs, slot {t}"
            assert int(a0.max()) < c.A
        torch.cuda.synchronize()
        chk_hc("hcarry")
        chk_obs("obs")


@pytest.mark.parametrize("c,impl", with_impls(C.SAMPLER))
def test_sampler_against_host_philox(c, impl):
    """The sampled ids of 5 slots x 200 envs x 2 agents against the host Philox and the float64 CDF: equal everywhere
    except where u tot lies within 1e-6 of a CDF entry, and every id of the second tile drawn at least once"""
    r = C.ref(c)
    want, near = C.sampler_reference(r)                                  # [N][T * E]
    with G.impl_option(impl):
        pd = G.params_dev(r)
        od, chk_obs = G.obs_dev(r)
        a_s, lp_s = G.run_policy(r, pd, od, 0, c.T, sample=True)
        chk_obs("obs")
    got = G.unpack_actions(c, a_s).reshape(c.N, c.T * c.E).numpy()
    print(f"  {int(near.sum())} of {near.size} draws within {C.CDF_EDGE} of a CDF entry; "
          f"{int((got != want).sum())} ids differ from the float64 CDF's")
    assert np.array_equal(got[~near], want[~near])
    seen = set(got.reshape(-1).tolist())
    assert set(range(16, c.A)) <= seen, sorted(set(range(16, c.A)) - seen)
    G.check_logp(r, lp_s, G.unpack_actions(c, a_s), False, (0, c.T), "sampled")


# ------------------------------------------------------------------------------------------------------ grad

def run_grads_ws(r, clip=0.1, beta=0.05):
    """One d2d_gru_grad launch with workspace= a guarded tensor of exactly d2d_gru_grad_workspace floats; every other
    buffer guarded as in test_gru_edges_gpu.run_grads -> ({name: gradient}, stats [N][2])"""
    from d2dhip import _lib, gru
    c = r.c
    pd = G.params_dev(r)
    od, chk_obs = G.obs_dev(r)
    acts, lo, W = r.train()
    checks = [(chk_obs, "obs")]
    W_d, chk = G.per_sample(W, "ten")
    checks.append((chk, "weight"))
    lo_d, chk = G.per_sample(lo, "ten")
    checks.append((chk, "logp_old"))
    a_d, chk = O.guarded(src=G.pack_actions(c, acts))
    checks.append((chk, "actions"))
    grads = {}
    for name in O.NAMES:
        grads[name], chk = O.guarded(shape=tuple(r.p[name].shape), dtype=torch.float32)
        checks.append((chk, "g_" + name))
    assert tuple(grads["w2"].shape) == (c.N, c.A, c.H) and tuple(grads["b2"].shape) == (c.N, c.A)
    stats, chk = O.guarded(shape=(c.N, 2), dtype=torch.float32)
    checks.append((chk, "stats"))
    lib = _lib.require_gpu()
    d = gru.desc(pd, c.E, gru.KIND[c.kind], c.L, c.ep)
    gru.set_format(d, od)
    n_ws = lib.d2d_gru_grad_workspace(ctypes.byref(d), c.T)
    assert n_ws > 0
    ws, chk = O.guarded(shape=(n_ws,), dtype=torch.float32)
    checks.append((chk, "workspace"))
    gru.grads(pd, od, c.kind, c.L, c.ep, W_d, actions=a_d, logp_old=lo_d, clip=clip, beta=beta, grads=grads,
              stats=stats, workspace=ws)
    torch.cuda.synchronize()
    for chk, what in checks:
        chk(what)
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()), f"g_{name}: not written (NaN) or not finite"
    assert bool(torch.isfinite(stats).all()), "stats"
    return grads, stats


@pytest.mark.parametrize("c", C.MATRIX + C.INPUTS + C.WINDOWS + C.BATCH, ids=O.cid)
def test_grads(c):
    """all eight gradient tensors and both loss sums against float64 autograd, clip 0.1; g_w2 / g_b2 at their real
    [N][A][H] / [N][A] shapes inside guards; the workspace exactly the size the query answers, inside guards"""
    r = C.ref(c)
    got, stats = run_grads_ws(r)
    G.check_grads(r, got, stats)


@pytest.mark.parametrize("c", [C.A17, C.A32, C.DRIVER], ids=O.cid)
def test_grads_clip_02(c):
    r = C.ref(c)
    got, stats = run_grads_ws(r, clip=0.2)
    G.check_grads(r, got, stats, clip=0.2)


@pytest.mark.parametrize("c", [C.A17, C.A32], ids=O.cid)
def test_grads_deterministic(c):
    """two launches on a NaN-filled workspace give the same bits"""
    r = C.ref(c)
    g0, s0 = run_grads_ws(r)
    g1, s1 = run_grads_ws(r)
    for name in O.NAMES:
        assert torch.equal(g0[name], g1[name]), name
    assert torch.equal(s0, s1)


@pytest.mark.parametrize("T,E", [(0, 17), (10, 0)])
@pytest.mark.parametrize("A", [17, 32])
def test_grads_empty_batch(T, E, A):
    """T = 0 or E = 0: the workspace query answers 0, every gradient (g_w2 / g_b2 at the real A) and loss sum is an exact
    zero, nothing outside the outputs is written -- not the one-float NaN workspace either"""
    from d2dhip import _lib, gru
    c = C.acase(30, 50, A)
    r = C.ref(c)
    pd = G.params_dev(r)
    od = torch.zeros((T, E, c.N, c.F), device=DEV)
    lib = _lib.require_gpu()
    d = gru.desc(pd, E, 1, c.L, c.ep)
    assert lib.d2d_gru_grad_workspace(ctypes.byref(d), T) == 0
    ws, chk_ws = O.guarded(shape=(1,), dtype=torch.float32)
    grads, checks = {}, [(chk_ws, "workspace")]
    for name in O.NAMES:
        grads[name], chk = O.guarded(shape=tuple(r.p[name].shape), dtype=torch.float32)
        checks.append((chk, "g_" + name))
    stats, chk = O.guarded(shape=(c.N, 2), dtype=torch.float32)
    checks.append((chk, "stats"))
    W = torch.zeros((T, E, c.N), device=DEV)
    gru.grads(pd, od, "softmax", c.L, c.ep, W, actions=torch.zeros((T, E, c.N), dtype=torch.uint8, device=DEV),
              logp_old=W, grads=grads, stats=stats, workspace=ws)
    torch.cuda.synchronize()
    for chk, what in checks:
        chk(what)
    assert bool(torch.isnan(ws).all()), "the workspace was written"
    for name in O.NAMES:
        assert bool((grads[name] == 0).all()), name
    assert bool((stats == 0).all())


# -------------------------------------------------------------------------------------------------- refusals

def _refused(fn, word):
    with pytest.raises(NotImplementedError) as e:
        fn()
    assert "n_out" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("what", ["sigmoid", "H80", "record"])
def test_refusals(what):
    """through gru.policy / gru.grads: the sigmoid head with 17 channels, hidden 80 with 17 ids, the record input with
    17 ids -- NotImplementedError with a message naming the rule, before anything is launched"""
    from d2dhip import gru
    from mlp_oracle import to_record
    H = 80 if what == "H80" else 50
    kind = "sigmoid" if what == "sigmoid" else "softmax"
    c = O.case(kind, 30, H, A=17, T=5)
    p, _ = O.make_net(c.N, c.F, c.H, c.A, 1, None)
    pd = {k: v.to(DEV).contiguous() for k, v in p.items()}
    obs = O.make_obs(c.T, c.E, c.N, c.F, [c.F] * c.N, 2)
    od = to_record(obs) if what == "record" else obs.to(DEV)
    word = {"sigmoid": "softmax", "H80": "hidden", "record": "record"}[what]
    dt = torch.uint8 if kind == "softmax" else torch.int32
    acts = torch.zeros((c.T, c.E, c.N), dtype=dt, device=DEV)
    W = torch.zeros((c.T, c.E, c.N), device=DEV)
    _refused(lambda: gru.policy(pd, od, kind, c.L, c.ep, 0, c.T, forced=acts), word)
    _refused(lambda: gru.policy(pd, od, kind, c.L, c.ep, 0, 1, deterministic=True), word)
    _refused(lambda: gru.grads(pd, od, kind, c.L, c.ep, W, actions=acts, logp_old=W), word)
