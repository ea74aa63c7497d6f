"""The fused behaviour-policy kernels (d2d_policy_mlp_step: csrc/policy_kernels.hip policy_split_kernel and
policy_mlp_kernel, policy_split.h, policy_epilogue.h) against the float64 oracle of tests/mlp_oracle.py, with
NONZERO biases (uniform +-1/sqrt(fan_in), as every other tensor), at the smallest shapes where each code path exists
(mlp_oracle.SHAPES) and at batch sizes around the 16-env tile, the 32-env tile pair and the workgroup
(E in {1, 15, 16, 17, 31, 32, 33, 127, 128, 129} at N = 5: (env N + k) & 3 takes every residue, and 129 envs are 10
workgroups of which xcd_block remaps 8; N = 1 and 8 at E = 129; N = 3 at E = 300; heterogeneous in_dims twice).
tests/test_mlp_oracle_cpu.py checks on the reference alone that these inputs are well conditioned (for A >= 2 every
probability in [1e-3, 1 - 1e-3]; every tie mask <= 1 % of its cells).

Every launch goes through launch(): obs is an interior view with 256 NaN floats on each side (the split kernel reads
rows unclamped and relies on its buffer descriptor past the tensor); actions, logp and value are interior views of
buffers pre-filled with a sentinel (float bits 0x7FC0A5A5, a NaN; action bytes 0xA5) with 128 sentinel elements on
each side.  Afterwards the outer sentinels are bit-intact, no float sentinel and no NaN is left inside, and no action
sentinel is left inside wherever 0xA5 / 0xA5A5 is not a legal action (it is one for Bernoulli masks of exactly 8 or 16
channels: there the bitwise comparison of every action with the forced / oracle action does the same job).

Parity rule (the project's, tests/test_irdqn_gpu.py): |kernel - f64| <= max(1e-5, 2 |torch fp32 on the CPU - f64|),
elementwise, for log-probs and values.  Actions are compared exactly outside the oracle's tie mask (Bernoulli: per
channel bit).  The log-probs returned with deterministic or sampled actions equal BIT FOR BIT the forced evaluation
of those actions."""
import ctypes
import functools

import numpy as np
import pytest

import mlp_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 128                 # sentinel elements on each side of every output (one per agent of the widest run)
OBS_PAD = 256               # NaN floats (record: 0xFF bytes) on each side of the obs
SENT_F = 0x7FC0A5A5         # a NaN that no arithmetic produces
SENT_B = 0xA5
IDS = [f"{k}-F{F}-H{H}-A{A}" for k, F, H, A in O.SHAPES]


@pytest.fixture(params=["split", "f32"])
def impl(request):
    from d2dhip import _lib
    lib = _lib.require_gpu()
    lib.d2d_set_option(_lib.D2D_OPT_POLICY_F32_MFMA, 1 if request.param == "f32" else 0)
    yield request.param
    lib.d2d_set_option(_lib.D2D_OPT_POLICY_F32_MFMA, 0)


# ---- the reference, computed once per run and shared (never modified)

class Ref:
    """Inputs and float64 / CPU-float32 references of one (shape, N, E, in_dims, frac) run; prefix(E1) is the same
    for the first E1 envs (every quantity is per env, the draws by global env index)."""

    def __init__(self, shape, N, E, dims, frac, parts=None):
        self.shape, self.N, self.E, self.dims, self.frac = shape, N, E, dims, frac
        kind, F, H, A = shape
        self.full = parts is None        # a batch of mlp_oracle.batches (the CPU test caps its tie shares), not a slice
        if parts is not None:
            self.__dict__.update(parts)
            return
        self.actor, self.critic, self.obs = O.case_inputs(shape, N, E, dims, frac)
        self.p64, self.p32 = O.probs(self.actor, self.obs), O.probs(self.actor, self.obs, torch.float32)
        self.v64, self.v32 = O.values(self.critic, self.obs), O.values(self.critic, self.obs, torch.float32)
        g = torch.Generator().manual_seed(O.shape_seed(*shape) + 3)
        self.forced = (torch.rand((N, E, A), generator=g) < 0.4) if kind == "comb" else \
            torch.randint(0, A, (N, E), generator=g)
        self.det, self.det_tie = O.deterministic_actions(self.p64, kind)
        self.smp, self.smp_tie = O.sampled_actions(self.p64, kind, O.RNG["env_base"] + np.arange(E), np.arange(N),
                                                   O.RNG["rng_step"], O.RNG["seed"])

    def rows(self, lo, hi):
        per_env = ("p64", "p32", "v64", "v32", "forced", "det", "det_tie", "smp", "smp_tie")
        parts = {n: getattr(self, n)[:, lo:hi] for n in per_env}
        parts.update(actor=self.actor, critic=self.critic, obs=self.obs[lo:hi])
        return Ref(self.shape, self.N, hi - lo, self.dims, self.frac, parts)


@functools.lru_cache(maxsize=None)
def ref(shape, N, E, dims, frac):
    return Ref(shape, N, E, None if dims is None else list(dims), frac)


@functools.lru_cache(maxsize=8)
def device_nets(shape, N, dims):
    r = ref(shape, N, O.E_MAX if N != 3 else 300, dims, False)
    to = lambda net: {k: v.cuda().contiguous() for k, v in net.items()}  # noqa: E731
    return to(r.actor), to(r.critic)


# ---- one guarded launch

def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def act_dtype(kind, A):
    return torch.int16 if kind == "comb" and A > 8 else torch.uint8


def _act_sentinel(dt):
    return SENT_B if dt == torch.uint8 else (SENT_B * 257) - 65536


def sentinel_is_legal(kind, A):
    """0xA5 (0xA5A5) is a possible Bernoulli mask of exactly 8 (16) channels, and nothing else's action."""
    return kind == "comb" and A in (8, 16)


def pad_obs(obs):
    """obs [E][N][F] (CPU float32) as an interior contiguous view of a NaN-filled device buffer"""
    n = obs.numel()
    buf = torch.full((n + 2 * OBS_PAD,), float("nan"), device="cuda")
    view = buf[OBS_PAD:OBS_PAD + n].view(obs.shape)
    view.copy_(obs)
    return view


def pad_record(obs):
    """the compact record of integer obs [E][N][F] as an interior view of a 0xFF-filled device buffer"""
    from d2dhip.record import ObsRecord
    rec = O.to_record(obs[None])
    n = rec.data.numel()
    buf = torch.full((n + 2 * OBS_PAD,), 0xFF, dtype=torch.uint8, device="cuda")
    view = buf[OBS_PAD:OBS_PAD + n].view(rec.data.shape[1:])
    view.copy_(rec.data[0])
    return ObsRecord(view, rec.obs_dim, rec.signed)


def launch(actor, critic, obs, kind, A, nan_agents=(), refused=None, **kw):
    """policy_mlp_step on guarded buffers (module docstring) -> (actions [E][N], logp [N][E], value [N][E] or None)
    as CPU tensors.  obs: the device view of pad_obs / pad_record.  nan_agents: agents whose outputs may be NaN (their
    obs rows are).  refused: the exception the call must raise, after which no buffer may have been written."""
    from d2dhip.policy import policy_mlp_step
    E, N = obs.shape[0], obs.shape[1]
    adt = act_dtype(kind, A)
    asent = _act_sentinel(adt)
    abuf, av = _guarded(E * N, adt, asent)
    lbuf, lv = _guarded(N * E, torch.int32, SENT_F)
    vbuf, vv = _guarded(N * E, torch.int32, SENT_F)
    args = dict(actions=av.view(E, N), logp=lv.view(torch.float32).view(N, E), value=vv.view(torch.float32).view(N, E))
    if refused is not None:
        with pytest.raises(refused):
            policy_mlp_step(actor, obs, kind, critic, **args, **kw)
        torch.cuda.synchronize()
        assert bool((abuf == asent).all()) and bool((lbuf == SENT_F).all()) and bool((vbuf == SENT_F).all())
        return None
    acts, lp, val = policy_mlp_step(actor, obs, kind, critic, **args, **kw)
    torch.cuda.synchronize()
    stored_a = kw.get("want_actions", True) or kw.get("forced") is None
    stored_v = critic is not None and kw.get("want_value", True)
    assert (acts is not None) == stored_a and (val is not None) == stored_v
    for name, buf, sent, stored in (("actions", abuf, asent, stored_a), ("logp", lbuf, SENT_F, True),
                                    ("value", vbuf, SENT_F, stored_v)):
        assert bool((buf[:GUARD] == sent).all()) and bool((buf[-GUARD:] == sent).all()), f"{name}: written outside"
        if not stored:
            assert bool((buf == sent).all()), f"{name}: written though omitted"
        elif name != "actions" or not sentinel_is_legal(kind, A):
            assert not bool((buf[GUARD:-GUARD] == sent).any()), f"{name}: a cell was never written"
    ok = torch.ones(N, dtype=torch.bool)
    ok[list(nan_agents)] = False
    lp = lp.cpu()
    assert not bool(lp[ok].isnan().any()), "NaN log-prob"
    if val is not None:
        val = val.cpu()
        assert not bool(val[ok].isnan().any()), "NaN value"
    return (acts.cpu() if acts is not None else None), lp, val


# ---- comparisons

def pack(kind, actions):
    """oracle actions (bits [N][E][A] / ids [N][E]) -> the kernel's [E][N] tensor"""
    from d2dhip.envbatch import pack_masks_torch
    if kind == "comb":
        return pack_masks_torch(actions.transpose(0, 1)).contiguous()
    return actions.t().to(torch.uint8).contiguous()


def unpack(kind, A, acts):
    """the kernel's [E][N] actions -> bits [N][E][A] (no bit at or past A may be set) / ids [N][E]"""
    if kind == "comb":
        m = acts.t().to(torch.int64) & 0xFFFF
        assert not bool((m >> A).any()), "mask bits past A"
        return ((m.unsqueeze(-1) >> torch.arange(A)) & 1).bool()
    ids = acts.t().to(torch.int64)
    assert bool((ids < A).all()), "id past A"
    return ids


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class Errors:
    """max |kernel - f64| beside torch fp32's, per quantity, and the largest tie share, over a test's runs"""

    def __init__(self):
        self.e = {"logp": [0.0, 0.0], "value": [0.0, 0.0]}
        self.tie = 0.0

    def close(self, what, got, r64, r32):
        err, err32 = (got.double() - r64).abs(), (r32.double() - r64).abs()
        self.e[what][0] = max(self.e[what][0], err.max().item())
        self.e[what][1] = max(self.e[what][1], err32.max().item())
        bad = err > torch.maximum(torch.full_like(err, 1e-5), 2 * err32)
        assert not bool(bad.any()), (what, err[bad].max().item(), int(bad.sum()), err32.max().item())

    def merge(self, other):
        for what, (e, e32) in other.e.items():
            self.e[what] = [max(self.e[what][0], e), max(self.e[what][1], e32)]
        self.tie = max(self.tie, other.tie)

    def line(self, tag):
        return (f"ERR {tag}: logp {self.e['logp'][0]:.2e} (torch fp32 {self.e['logp'][1]:.2e})  "
                f"value {self.e['value'][0]:.2e} (torch fp32 {self.e['value'][1]:.2e})  tie share {self.tie:.5f}")


def check_actions(kind, got, want, tie, errs, full):
    """got == want outside the tie mask (Bernoulli: every channel bit on its own).  The mask's share is capped at
    1 % on the full batches, the ones tests/test_mlp_oracle_cpu.py checks on the CPU; a slice of a batch (one env is
    five cells) keeps the mask per cell without a cap of its own."""
    if full:
        errs.tie = max(errs.tie, tie.double().mean().item())
        assert tie.double().mean().item() <= 0.01
    assert bool(((got == want) | tie).all()), int(((got != want) & ~tie).sum())


def run_modes(r, impl, total, obs=None, env_base=None, rows=""):
    """The three modes of one run, each checked against the reference r: (a) forced with the critic, (b)
    deterministic without it, (c) sampled with the critic.  Returns every output, for the bitwise comparisons between
    runs, and prints the run's own error figures (merged into `total`, the test's)."""
    kind, F, H, A = r.shape
    errs = Errors()
    actor, critic = device_nets(r.shape, r.N, None if r.dims is None else tuple(r.dims))
    obs = pad_obs(r.obs) if obs is None else obs
    lp64 = lambda acts: O.logp(r.p64, kind, acts)  # noqa: E731
    lp32 = lambda acts: O.logp(r.p32, kind, acts)  # noqa: E731
    # a. forced, with the critic
    forced = pack(kind, r.forced).cuda()
    a_acts, a_lp, a_val = launch(actor, critic, obs, kind, A, forced=forced)
    assert torch.equal(a_acts, forced.cpu()), "forced actions are returned as given"
    errs.close("logp", a_lp, lp64(r.forced), lp32(r.forced))
    errs.close("value", a_val, r.v64, r.v32)
    # b. deterministic, no critic
    b_acts, b_lp, none = launch(actor, None, obs, kind, A, deterministic=True)
    assert none is None
    got = unpack(kind, A, b_acts)
    check_actions(kind, got, r.det, r.det_tie, errs, r.full)
    _, b_lp2, _ = launch(actor, None, obs, kind, A, forced=b_acts.cuda())
    assert bits_equal(b_lp, b_lp2), "deterministic log-probs differ from their forced evaluation"
    errs.close("logp", b_lp, lp64(got), lp32(got))
    # c. sampled (nonzero seed, env_base, rng_step), with the critic
    rng = dict(O.RNG)
    if env_base is not None:
        rng["env_base"] = env_base
    c_acts, c_lp, c_val = launch(actor, critic, obs, kind, A, **rng)
    got = unpack(kind, A, c_acts)
    check_actions(kind, got, r.smp, r.smp_tie, errs, r.full)
    _, c_lp2, c_val2 = launch(actor, critic, obs, kind, A, forced=c_acts.cuda())
    assert bits_equal(c_lp, c_lp2), "sampled log-probs differ from their forced evaluation"
    assert bits_equal(c_val, c_val2) and bits_equal(c_val, a_val)
    errs.close("logp", c_lp, lp64(got), lp32(got))
    print(errs.line(f"{IDS[O.SHAPES.index(r.shape)]} {impl} {'frac' if r.frac else 'int'} N {r.N} E {r.E}{rows}"
                    f"{' het' if r.dims else ''}"))
    total.merge(errs)
    return dict(a_lp=a_lp, a_val=a_val, b_acts=b_acts, b_lp=b_lp, c_acts=c_acts, c_lp=c_lp)


def assert_rows_equal(small, big, lo, hi, what):
    """every output of the run on envs [lo, hi) alone equals, bit for bit, those rows of the larger run"""
    for name, t in small.items():
        if name.endswith("acts"):
            assert torch.equal(t, big[name][lo:hi]), (what, name)
        else:
            assert bits_equal(t, big[name][:, lo:hi].contiguous()), (what, name)


# ---- a-c and e: parity at every E edge, batch independence

@pytest.mark.parametrize("shape", O.SHAPES, ids=IDS)
def test_parity_at_batch_edges(shape, impl):
    for frac in (False, True):
        errs = Errors()
        full = ref(shape, 5, O.E_MAX, None, frac)
        big = run_modes(full, impl, errs)
        for E1 in O.E_EDGES[:-1]:
            # e. the same envs in a smaller batch: the same bits (and the same checks against the reference)
            assert_rows_equal(run_modes(full.rows(0, E1), impl, errs), big, 0, E1, f"E {E1}")
        # rows [33:] alone with env_base + 33: the draw belongs to (env, agent, step), not to a batch position
        tail = run_modes(full.rows(33, O.E_MAX), impl, errs, env_base=O.RNG["env_base"] + 33, rows=" rows [33:]")
        assert_rows_equal(tail, big, 33, O.E_MAX, "rows [33:]")
        print(errs.line(f"ALL {IDS[O.SHAPES.index(shape)]} {impl} {'frac' if frac else 'int'} N 5"))


@pytest.mark.parametrize("shape", O.SHAPES, ids=IDS)
def test_parity_at_other_agent_counts(shape, impl):
    for frac in (False, True):
        errs = Errors()
        for N, E, dims in O.batches(shape)[1:]:
            run_modes(ref(shape, N, E, None if dims is None else tuple(dims), frac), impl, errs)
        print(errs.line(f"ALL {IDS[O.SHAPES.index(shape)]} {impl} {'frac' if frac else 'int'} N 1, 8, 3, het"))


# ---- d. option and argument variants

@pytest.mark.parametrize("shape", O.SHAPES, ids=IDS)
def test_option_and_argument_variants(shape, impl):
    from d2dhip import _lib
    lib = _lib.require_gpu()
    kind, F, H, A = shape
    r = ref(shape, 5, O.E_MAX, None, True)
    actor, critic = device_nets(shape, 5, None)
    obs = pad_obs(r.obs)
    forced = pack(kind, r.forced).cuda()
    base = {"forced": launch(actor, critic, obs, kind, A, forced=forced),
            "det": launch(actor, critic, obs, kind, A, deterministic=True),
            "smp": launch(actor, critic, obs, kind, A, **O.RNG)}
    same = lambda x, y: torch.equal(x[0], y[0]) and bits_equal(x[1], y[1]) and bits_equal(x[2], y[2])  # noqa: E731
    try:
        lib.d2d_set_option(_lib.D2D_OPT_POLICY_CRITIC_SPLIT, 1)
        split = {"forced": launch(actor, critic, obs, kind, A, forced=forced),
                 "det": launch(actor, critic, obs, kind, A, deterministic=True),
                 "smp": launch(actor, critic, obs, kind, A, **O.RNG)}
        a4, lp4, v4 = launch(actor, critic, obs, kind, A, want_value=False, **O.RNG)
    finally:
        lib.d2d_set_option(_lib.D2D_OPT_POLICY_CRITIC_SPLIT, 0)
    for mode in base:
        assert same(split[mode], base[mode]), f"actor + value-only launches differ from the fused one ({mode})"
    assert v4 is None and torch.equal(a4, base["smp"][0]) and bits_equal(lp4, base["smp"][1])
    # want_value = False / want_actions = False: the omitted buffer stays untouched (launch() asserts it)
    a5, lp5, v5 = launch(actor, critic, obs, kind, A, want_value=False, **O.RNG)
    assert v5 is None and torch.equal(a5, base["smp"][0]) and bits_equal(lp5, base["smp"][1])
    a6, lp6, v6 = launch(actor, critic, obs, kind, A, forced=forced, want_actions=False)
    assert a6 is None and bits_equal(lp6, base["forced"][1]) and bits_equal(v6, base["forced"][2])
    # the device word rng_offset: rng_step = s with the word o is rng_step = s + o with none
    o = 3
    word = torch.tensor([o], dtype=torch.int32, device="cuda")
    rng = dict(O.RNG, rng_step=O.RNG["rng_step"] - o)
    assert same(launch(actor, critic, obs, kind, A, rng_offset=word.data_ptr(), **rng), base["smp"])
    if A > 1:   # (A = 1 has one possible action: nothing can differ)
        assert not torch.equal(launch(actor, critic, obs, kind, A, **rng)[0], base["smp"][0]), "rng_step is ignored"


# ---- f. poisoned neighbour

@pytest.mark.parametrize("shape", O.SHAPES, ids=IDS)
def test_poisoned_neighbour_rows(shape, impl):
    """Agent 1's whole obs rows are NaN: the other agents' outputs do not change by a bit (the split kernel reads
    the columns past F of agent 0's rows from agent 1's and removes them with a bit mask)."""
    kind, F, H, A = shape
    for frac in (False, True):
        r = ref(shape, 5, O.E_MAX, None, frac)
        actor, critic = device_nets(shape, 5, None)
        forced = pack(kind, r.forced).cuda()
        clean, poisoned = pad_obs(r.obs), pad_obs(r.obs)
        poisoned[:, 1, :] = float("nan")
        others = [0, 2, 3, 4]
        for kw in (dict(forced=forced), dict(deterministic=True), dict(O.RNG)):
            a0, lp0, v0 = launch(actor, critic, clean, kind, A, **kw)
            a1, lp1, v1 = launch(actor, critic, poisoned, kind, A, nan_agents=(1,), **kw)
            assert torch.equal(a0[:, others], a1[:, others]), kw.keys()
            assert bits_equal(lp0[others], lp1[others]) and bits_equal(v0[others], v1[others]), kw.keys()


# ---- g. the compact record

@pytest.mark.parametrize("shape", [s for s in O.SHAPES if s[1] <= 63], ids=[i for i, s in zip(IDS, O.SHAPES) if s[1] <= 63])
def test_compact_record_equals_fp32_rows(shape, impl):
    kind, F, H, A = shape
    full = ref(shape, 5, O.E_MAX, None, False)
    actor, critic = device_nets(shape, 5, None)
    for E1 in (1, 17, 33, O.E_MAX):
        r = full.rows(0, E1)
        rows, rec = pad_obs(r.obs), pad_record(r.obs)
        forced = pack(kind, r.forced).cuda()
        for kw in (dict(forced=forced), dict(deterministic=True), dict(O.RNG)):
            if impl == "f32":
                # the fp32-MFMA kernel reads fp32 rows only: the library's error, and nothing written
                launch(actor, critic, rec, kind, A, refused=NotImplementedError, **kw)
                continue
            a0, lp0, v0 = launch(actor, critic, rows, kind, A, **kw)
            a1, lp1, v1 = launch(actor, critic, rec, kind, A, **kw)
            assert torch.equal(a0, a1) and bits_equal(lp0, lp1) and bits_equal(v0, v1), (E1, kw.keys())


# ---- single tests

def _image(F, H):
    N, E, A = H, 2 * F + 4, 3
    g = torch.Generator().manual_seed(F * 1000 + H)
    actor, critic = O.make_params(N, F, H, A, F + H)
    W = torch.randn((H, F), generator=g) * 0.05           # full-mantissa weights of both signs
    W[:, 1::7] = 0.0                                       # and exact zeros
    critic["w1"] = W.expand(N, H, F).contiguous()
    critic["w2"] = torch.eye(H).view(N, 1, H).contiguous()
    critic["b2"] = torch.zeros(N, 1)
    c1 = torch.randn((N, H), generator=g) * 0.3
    x = torch.zeros(E, N, F)
    e = torch.arange(E - 1)
    x[e, :, e % F] = 1.0
    to = lambda net: {k: v.cuda().contiguous() for k, v in net.items()}  # noqa: E731
    relu = lambda t: torch.where(t > 0, t, torch.zeros_like(t))  # noqa: E731
    # leg 1
    critic["b1"] = torch.zeros(N, H)
    _, _, val = launch(to(actor), to(critic), pad_obs(x), "comb", A, deterministic=True)
    want = torch.zeros(N, E)
    want[:, :E - 1] = relu(W[:, e % F])
    assert bits_equal(val, want), int((val.view(torch.int32) != want.view(torch.int32)).sum())
    # leg 2
    critic["b1"] = c1
    _, _, val = launch(to(actor), to(critic), pad_obs(torch.zeros(E, N, F)), "comb", A, deterministic=True)
    want = relu(c1.diagonal())[:, None].expand(N, E).contiguous()
    assert bits_equal(val, want), int((val.view(torch.int32) != want.view(torch.int32)).sum())


@pytest.mark.parametrize("which,F,H", [("split", 30, 64), ("split", 31, 128), ("split", 63, 64), ("f32", 64, 64),
                                       ("f32", 30, 64)])
def test_critic_layer1_image_is_bit_exact(which, F, H):
    """N = H agents share one critic layer-1 matrix W; agent k's layer 2 is e_k, c2 = 0.
    Leg 1: c1 = 0, env e has x = e_(e mod F) and the last env x = 0: value[k][e] == relu(W[k][e mod F]) bit for bit
    (+0 for negatives), 0 for the zero env.  Leg 2: x = 0, random c1: value[k][e] == relu(c1[k][k]).
    Both are exact: the three bf16 parts of a weight times 1 re-add to the weight in the order the kernel sums them
    (l + m has at most 16 significant bits), and the fp32 kernel's fmaf chain adds zeros."""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    lib.d2d_set_option(_lib.D2D_OPT_POLICY_F32_MFMA, 1 if which == "f32" else 0)
    try:
        _image(F, H)
    finally:
        lib.d2d_set_option(_lib.D2D_OPT_POLICY_F32_MFMA, 0)


@pytest.mark.parametrize("kind", ["comb", "chsel"])
def test_clamp_at_the_extreme_probabilities(kind, impl):
    """w2 = 0 and b2 = (+30, -30, 0, 0): p = (1 - 2e-13, 9e-27, 9e-14, 9e-14) for every input.  Forced on action 0 and
    on action 1, the log-probs are the clamped ones (p in [2^-23, 1 - 2^-23], torch's float32 eps) within 1e-5."""
    N, E, F, H, A = 3, 33, 12, 16, 4
    actor, _ = O.make_params(N, F, H, A, 5)
    actor["w2"] = torch.zeros(N, A, H)
    actor["b2"] = torch.tensor([30.0, -30.0, 0.0, 0.0]).expand(N, A).contiguous()
    obs = O.make_obs(E, N, F, None, 6, False)
    p64 = O.probs(actor, obs)
    assert p64[..., 0].min().item() > 1 - 2.0 ** -23 and p64[..., 1:].max().item() < 2.0 ** -23
    dev = {k: v.cuda().contiguous() for k, v in actor.items()}
    for a in (0, 1):
        if kind == "comb":
            acts = torch.zeros((N, E, A), dtype=torch.bool)
            acts[..., a] = True
        else:
            acts = torch.full((N, E), a)
        _, lp, _ = launch(dev, None, pad_obs(obs), kind, A, forced=pack(kind, acts).cuda())
        want = O.logp(p64, kind, acts)
        assert (lp.double() - want).abs().max().item() <= 1e-5, (a, lp[0, 0].item(), want[0, 0].item())


@pytest.mark.parametrize("E,N", [(0, 5), (33, 0), (0, 0)])
def test_empty_batch_writes_nothing(E, N, impl):
    from d2dhip import _lib
    lib = _lib.require_gpu()
    F, H, A = 12, 16, 4
    t = torch.zeros(4096, device="cuda")                    # stands for every input: never read
    abuf = torch.full((256,), SENT_B, dtype=torch.uint8, device="cuda")
    lbuf = torch.full((256,), SENT_F, dtype=torch.int32, device="cuda")
    vbuf = torch.full((256,), SENT_F, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    for forced in (None, p):
        for det in (0, 1):
            desc = _lib.MlpDesc(N, E, F, H, A, 1, p, p, p, p, p, p, p, p, 1234, 77)
            rc = lib.d2d_policy_mlp_step(desc, p, forced, 5, det, abuf[GUARD:].data_ptr(), lbuf[GUARD:].data_ptr(),
                                         vbuf[GUARD:].data_ptr(), _lib.stream_ptr())
            assert rc == 0, lib.d2d_last_error()
    torch.cuda.synchronize()
    assert bool((abuf == SENT_B).all()) and bool((lbuf == SENT_F).all()) and bool((vbuf == SENT_F).all())
