"""The wide GRU kernels (csrc/gru_wide_kernels.hip, gru_l2_common.h: hidden sizes 65..128) against float64 torch, on
the input sets of tests/gru_wide_cases.py (tests/test_gru_wide_cpu.py asserts on the CPU the conditions that make
every comparison here strict).

The helpers and the tolerances are those of tests/test_gru_edges_gpu.py, used as they are: values and log-probs 1e-5
absolute (Bernoulli: lp_tol), deterministic actions exact off ties, gradients within 2e-5 max|g| + 1e-7 of float64
autograd, loss sums rtol 1e-5 / atol 1e-4, no fp32-band branch and no mask that drops samples; every input and
output lives in a 0xFF-filled guarded buffer whose guards are checked.  The one helper of its own is run_grads, which
hands d2dhip.gru.grads a caller workspace (the chunking of the update follows from its size).

Shapes: N = 2 agents, E = 17 envs (a full tile and a tile of one), one 5-slot episode for H >= 96 and two for
H = 65 / 72 / 80, 3-step windows unless the set is about the window; the largest are L = 65 at E = 3, T = 6."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gru_oracle as O  # noqa: E402
import gru_wide_cases as W  # noqa: E402
import test_gru_edges_gpu as G  # noqa: E402  (helpers only: nothing of it is collected or changed here)

DEV = G.DEV
CASES = W.all_cases()
H72 = [c for c in W.LOW if c.H == 72]
H80 = [c for c in W.LOW if c.H == 80 and c.F != 63]      # one set of each kind, two episodes


# ---------------------------------------------------------------------------------------------------- policy

@pytest.mark.parametrize("c", CASES, ids=O.cid)
def test_policy(c):
    """forced log-probs of the padded windows; sampled actions, bitwise their forced re-evaluation; deterministic
    actions, padded and unpadded; values padded and unpadded"""
    G.policy_all(O.ref(c))


@pytest.mark.parametrize("c", W.exact(CASES), ids=O.cid)
def test_policy_record_input(c):
    """the same integer data as the compact record (columns >= F of a record row are not inputs here)"""
    G.policy_all(O.ref(c), "record")


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
@pytest.mark.parametrize("c", W.BASE_CASES + H80, ids=O.cid)
def test_policy_slot_ranges(c, padded):
    """slot0 > 0 with n_slots > 1 (H = 80: slots 3 .. 6 of two 5-slot episodes, across the boundary; H = 100: slots
    2 .. 4 of one) and all slots in one launch equal one launch per slot bit for bit, and float64 within tolerance"""
    r = O.ref(c)
    pd = G.params_dev(r)
    od, chk_obs = G.obs_dev(r)
    each = G.per_slot_outputs(r, pd, od, 0, c.T, padded)
    G.assert_same_launches(G.slot_outputs(r, pd, od, 0, c.T, padded), each, "all slots")
    s0, s1 = (3, 7) if c.T == 10 else (2, 5)
    part = G.slot_outputs(r, pd, od, s0, s1 - s0, padded)
    sl = slice(s0 * c.E, s1 * c.E)
    G.assert_same_launches(part, (each[0][:, sl], None if each[1] is None else each[1][s0:s1]), "a slot range")
    if c.kind is None:
        G.check_values(r, part[0], padded, (s0, s1), "a slot range")
    else:
        G.check_logp(r, part[0], r.actions()[:, s0:s1], padded, (s0, s1), "a slot range")
    chk_obs("obs")


@pytest.mark.parametrize("c", W.BASE_CASES, ids=O.cid)
def test_policy_poisoned_neighbour(c):
    """Changing env e's obs changes env e's outputs only: every other env's are the same bits (e = 5 inside the full
    tile, e = 16 the ragged tile's only env)"""
    r = O.ref(c)
    pd = G.params_dev(r)
    od, _ = G.obs_dev(r)
    base = G.slot_outputs(r, pd, od, 0, c.T, False)
    for e in (5, 16):
        obs2 = r.obs.clone()
        obs2[:, e] = (obs2[:, e] + 1.0) * (obs2[:, e] != 0)       # (columns past in_dims stay zero)
        od2, _ = G.obs_dev(r, obs=obs2)
        got = G.slot_outputs(r, pd, od2, 0, c.T, False)
        keep = torch.ones(c.E, dtype=torch.bool)
        keep[e] = False
        a, b = base[0].view(c.N, c.T, c.E), got[0].view(c.N, c.T, c.E)
        assert torch.equal(a[:, :, keep], b[:, :, keep]), e
        assert not torch.equal(a[:, :, e], b[:, :, e]), e
        if base[1] is not None:
            assert torch.equal(base[1][:, keep], got[1][:, keep]), e


@pytest.mark.parametrize("fmt", ["f32", "record"])
@pytest.mark.parametrize("deterministic", [False, True], ids=["sample", "deterministic"])
@pytest.mark.parametrize("c", W.BASE_CASES + H72 + [W.WINDOW_MISC[0]], ids=O.cid)
def test_policy_carry_equals_recompute(c, deterministic, fmt):
    """Every slot in order with the carried state (a guarded buffer of exactly carry_floats elements) and without:
    the same bits, at H = 100 (HT = 7) and H = 72 (HT = 5), L = 3 and L = 8 > episode"""
    from d2dhip import gru
    r = O.ref(c)
    pd = G.params_dev(r)
    od, chk_obs = G.obs_dev(r, fmt)
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


@pytest.mark.parametrize("c", W.WINDOW_LONG[:3], ids=O.cid)
def test_policy_long_padded_window_under_graph_capture(c):
    """A padded L = 64 launch allocates nothing and synchronises nothing: it is captured, and the replay equals the
    eager launch bit for bit"""
    from d2dhip import gru
    r = O.ref(c)
    pd = G.params_dev(r)
    od, chk_obs = G.obs_dev(r)
    forced = None if c.kind is None else G.pack_actions(c, r.actions())
    _, eager = G.run_policy(r, pd, od, 0, c.T, padded=True, forced=forced)
    eager = eager.clone()
    out, chk_out = O.guarded(shape=(c.N, c.T * c.E), dtype=torch.float32)
    kw = {} if c.kind is None else dict(forced=forced.to(DEV), want_actions=False)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gru.policy(pd, od, c.kind, c.L, c.ep, 0, c.T, padded=True, out=out, **kw)
    graph.replay()
    torch.cuda.synchronize()
    chk_out("out")
    chk_obs("obs")
    assert torch.equal(out, eager)


# ------------------------------------------------------------------------------------------------------ grad

def workspace_floats(r, fmt="f32"):
    """(d2d_gru_grad_workspace's answer, the floats of one tile of every agent) for the set's update"""
    from d2dhip import _lib, gru
    c = r.c
    lib = _lib.require_gpu()
    d = gru.desc(G.params_dev(r), c.E, gru.KIND[c.kind], c.L, c.ep)
    d.obs_format = _lib.D2D_OBS_U8 if fmt == "record" else _lib.D2D_OBS_F32
    full = lib.d2d_gru_grad_workspace(ctypes.byref(d), c.T)
    tiles = c.T * ((c.E + 15) // 16)
    assert full > 0 and full % tiles == 0, "the whole batch of these sets is below the budget: one chunk"
    return full, full // tiles


def run_grads(r, fmt="f32", clip=0.1, beta=0.05, scale=None, layout="ten", ws_floats=None, fill=float("nan")):
    """One d2d_gru_grad launch on guarded buffers, the workspace (ws_floats, default the recommended size) among them
    and filled with NaN -> ({name: gradient}, stats [N][2]) on the device"""
    from d2dhip import gru
    c = r.c
    pd = G.params_dev(r)
    od, chk_obs = G.obs_dev(r, fmt)
    acts, lo, Wt = r.train()
    checks = [(chk_obs, "obs")]
    W_d, chk = G.per_sample(Wt, layout)
    checks.append((chk, "weight"))
    kw = {}
    if c.kind is not None:
        lo_d, chk = G.per_sample(lo, layout)
        checks.append((chk, "logp_old"))
        a_d, chk = O.guarded(src=G.pack_actions(c, acts))
        checks.append((chk, "actions"))
        kw = dict(actions=a_d, logp_old=lo_d)
    grads = {}
    for name in O.NAMES:
        grads[name], chk = O.guarded(shape=tuple(r.p[name].shape), dtype=torch.float32)
        checks.append((chk, "g_" + name))
    stats, chk = O.guarded(shape=(c.N, 2), dtype=torch.float32)
    checks.append((chk, "stats"))
    ws, chk = O.guarded(shape=(workspace_floats(r, fmt)[0] if ws_floats is None else ws_floats,), dtype=torch.float32)
    checks.append((chk, "workspace"))
    ws.fill_(fill)
    gru.grads(pd, od, c.kind, c.L, c.ep, W_d, clip=clip, beta=beta, scale=scale, grads=grads, stats=stats,
              workspace=ws, **kw)
    torch.cuda.synchronize()
    for chk, what in checks:
        chk(what)
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()), f"g_{name}: not written (NaN) or not finite"
    assert bool(torch.isfinite(stats).all()), "stats"
    return grads, stats


def same_bits(a, b):
    for name in O.NAMES:
        assert torch.equal(a[0][name], b[0][name]), name
    assert torch.equal(a[1], b[1]), "stats"


@pytest.mark.parametrize("c", CASES, ids=O.cid)
def test_grads(c):
    """all eight gradients and the loss sums on fp32 rows, from a NaN-filled workspace"""
    r = O.ref(c)
    G.check_grads(r, *run_grads(r))


@pytest.mark.parametrize("c", W.exact(CASES), ids=O.cid)
def test_grads_record_input(c):
    r = O.ref(c)
    G.check_grads(r, *run_grads(r, "record"))


@pytest.mark.parametrize("layout", ["ten", "net", "view"])
@pytest.mark.parametrize("c", W.BASE_CASES, ids=O.cid)
def test_grads_arguments(c, layout):
    """weight / logp_old as contiguous [T][E][N], as [N][E*T] and as a strided view of a wider NaN-filled tensor;
    scale = 0.37 / (T E), beta = 0, clip = 0.2"""
    r = O.ref(c)
    got, stats = run_grads(r, clip=0.2, beta=0.0, scale=0.37 / (c.T * c.E), layout=layout)
    G.check_grads(r, got, stats, clip=0.2, beta=0.0, factor=0.37)


@pytest.mark.parametrize("fmt", ["f32", "record"])
@pytest.mark.parametrize("c", W.BASE_CASES, ids=O.cid)
def test_grads_workspace_and_determinism(c, fmt):
    """A NaN-filled and a zero-filled workspace give the same bits (nothing is read that the launch did not write),
    and so does a second NaN-filled run"""
    r = O.ref(c)
    runs = [run_grads(r, fmt, fill=f) for f in (float("nan"), 0.0, float("nan"))]
    same_bits(runs[0], runs[1])
    same_bits(runs[0], runs[2])
    G.check_grads(r, *runs[0])


@pytest.mark.parametrize("fmt", ["f32", "record"])
@pytest.mark.parametrize("c", W.CHUNK, ids=O.cid)
def test_grads_chunking(c, fmt):
    """E = 33: 15 tiles per agent.  The recommended workspace holds them all (one BPTT + wgrad pair); a workspace of
    exactly one tile per agent runs 15 pairs, the later ones adding to the output; seven tiles per agent run 7 + 7 + 1.
    The sums differ in their order, so each is held to float64 on its own, and each is bitwise reproducible.  One
    float less than a tile of every agent is refused."""
    r = O.ref(c)
    full, one = workspace_floats(r, fmt)
    assert full == 15 * one
    for floats in (full, one, 7 * one + 5):
        a = run_grads(r, fmt, ws_floats=floats)
        G.check_grads(r, *a, what=f"{floats // one} tiles per chunk: ")
        same_bits(a, run_grads(r, fmt, ws_floats=floats))
    with pytest.raises(ValueError, match="one tile of every agent"):
        run_grads(r, fmt, ws_floats=one - 1)


@pytest.mark.parametrize("fmt", ["f32", "record"])
@pytest.mark.parametrize("kind", O.KINDS, ids=lambda k: k or "value")
@pytest.mark.parametrize("T,E", [(0, 17), (5, 0), (0, 0)])
def test_grads_empty_batch(T, E, kind, fmt):
    """T = 0 or E = 0: d2d_gru_grad_workspace asks for 0 floats, d2d_gru_grad returns OK, every gradient and loss sum is
    an exact zero, and nothing outside the outputs is written -- not the one-float NaN workspace either"""
    from d2dhip import _lib, gru
    from mlp_oracle import to_record
    c = W.case(kind, 30, 100)
    r = O.ref(c)
    pd = G.params_dev(r)
    obs = torch.zeros((T, E, c.N, c.F))
    od = obs.to(DEV) if fmt == "f32" else to_record(obs)
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
    Wt = torch.zeros((T, E, c.N), device=DEV)
    kw = {} if kind is None else dict(actions=torch.zeros((T, E, c.N), dtype=torch.uint8, device=DEV), logp_old=Wt)
    gru.grads(pd, od, kind, c.L, c.ep, Wt, grads=grads, stats=stats, workspace=ws, **kw)      # raises unless D2D_OK
    torch.cuda.synchronize()
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
    c = W.case(kind, 30, 100)
    r = O.ref(c)
    pd = G.params_dev(r)
    od, chk_obs = G.obs_dev(r)
    out, chk_out = O.guarded(shape=(c.N, c.E), dtype=torch.float32)
    act, chk_act = O.guarded(shape=(1, c.E, c.N), dtype=G.act_dtype(c))
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
    Wt = torch.zeros((c.T, c.E, 0), device=DEV)
    gkw = {} if kind is None else dict(actions=torch.zeros((c.T, c.E, 0), dtype=torch.uint8, device=DEV), logp_old=Wt)
    gru.grads(p0, obs0, kind, c.L, c.ep, Wt, grads=grads, stats=stats, **gkw)
    torch.cuda.synchronize()
    for chk, what in checks:
        chk(what)
    for t in [out, stats] + list(grads.values()):
        assert bool(torch.isnan(t).all()), "an output was written"
    assert bool((act.view(torch.uint8) == 0xFF).all()), "actions_out was written"


# --------------------------------------------------------------------------------------------------- control

@pytest.mark.parametrize("kind", O.KINDS, ids=lambda k: k or "value")
def test_narrow_path_is_untouched_by_wide_launches(kind):
    """Control: an H = 64 set (gru_kernels.hip) gives the same bits before and after policy and update launches of an
    H = 100 set on the same module state (the shared workspace buffer, the options), and float64 within tolerance
    both times -- the dispatch by hidden size leaves the narrow path what it is."""
    narrow, wide = O.ref(O.case(kind, 31, 64)), O.ref(W.case(kind, 30, 100))

    def narrow_outputs():
        pd = G.params_dev(narrow)
        od, _ = G.obs_dev(narrow)
        pol = G.slot_outputs(narrow, pd, od, 0, narrow.c.T, True)
        return pol, G.run_grads(narrow)

    before = narrow_outputs()
    G.policy_all(wide)
    run_grads(wide)
    G.run_grads(wide)          # through the module's own workspace buffer, which the narrow launches share
    after = narrow_outputs()
    G.assert_same_launches(before[0], after[0], "policy")
    same_bits((before[1][0], before[1][1][:, :1 if kind is None else 2]),
              (after[1][0], after[1][1][:, :1 if kind is None else 2]))
    G.check_grads(narrow, *after[1])
