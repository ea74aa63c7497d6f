"""The wide behaviour-policy slot (d2d_policy_mlp_wide_step, csrc/mlp_wide_kernels.hip policy_wide_kernel: hidden
65..128 with obs_dim 32..63) against the float64 oracle of tests/mlp_oracle.py, by the criteria of
tests/test_policy_edges_gpu.py, whose guarded launch and comparisons it imports: obs, actions, log-probs
and values are interior views between NaN / sentinel guards that stay bit-intact, and no NaN comes out.

Shapes: mlp_wide_cases.SHAPES, the smallest at which each path can go wrong (both edges of the hidden and input
ranges, a ragged last hidden tile, A = 1 / <= 8 / > 8, both kinds).  Batches: E in {1, 15, 16, 17, 31, 32, 33, 127,
128, 129} at N = 5 (the 16-env tile and the 4-wave workgroup), N = 1 and 8 at E = 129, N = 3 at E = 300, two
heterogeneous in_dims sets with agents narrower than 32 columns; integer and fractional obs.
tests/test_mlp_wide_cpu.py checks on the oracle alone that these inputs are well conditioned.

Parity: |kernel - f64| <= max(1e-5, 2 |torch fp32 on the CPU - f64|), elementwise, for log-probs and values.  Actions
equal the oracle's outside its tie mask; the log-probs returned with deterministic or sampled actions equal BIT FOR
BIT the forced evaluation of those actions.  Bitwise too: the same envs in a smaller batch or from row 33 on with
env_base + 33; rng_step = s with the device word o against rng_step = s + o; want_value = False / want_actions =
False; the compact record (64-byte rows) against fp32 rows on integer obs; every agent beside a NaN-poisoned one."""
import ctypes
import functools

import pytest

import mlp_oracle as O
import mlp_wide_cases as C
import test_policy_edges_gpu as P
from test_policy_edges_gpu import (GUARD, SENT_B, SENT_F, Errors, assert_rows_equal, bits_equal, check_actions, launch,
                                   pack, pad_obs, pad_record, unpack)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@functools.lru_cache(maxsize=None)
def ref(shape, N, E, dims, frac):
    from d2dhip import _lib
    assert _lib.mlp_wide(shape[1], shape[2]), "every shape of this file runs on the wide entry point"
    return P.Ref(shape, N, E, None if dims is None else list(dims), frac)


@functools.lru_cache(maxsize=8)
def device_nets(shape, N, dims):
    r = ref(shape, N, O.E_MAX if N != 3 else 300, dims, False)
    to = lambda net: {k: v.cuda().contiguous() for k, v in net.items()}  # noqa: E731
    return to(r.actor), to(r.critic)


def run_modes(r, total, obs=None, env_base=None, rows=""):
    """The three modes of one run against the reference r: (a) forced with the critic, (b) deterministic without it,
    (c) sampled with the critic.  Returns every output for the bitwise comparisons between runs."""
    kind, F, H, A = r.shape
    errs = Errors()
    actor, critic = device_nets(r.shape, r.N, None if r.dims is None else tuple(r.dims))
    obs = pad_obs(r.obs) if obs is None else obs
    lp64 = lambda acts: O.logp(r.p64, kind, acts)  # noqa: E731
    lp32 = lambda acts: O.logp(r.p32, kind, acts)  # noqa: E731
    forced = pack(kind, r.forced).cuda()
    a_acts, a_lp, a_val = launch(actor, critic, obs, kind, A, forced=forced)
    assert torch.equal(a_acts, forced.cpu()), "forced actions are returned as given"
    errs.close("logp", a_lp, lp64(r.forced), lp32(r.forced))
    errs.close("value", a_val, r.v64, r.v32)
    b_acts, b_lp, none = launch(actor, None, obs, kind, A, deterministic=True)
    assert none is None
    got = unpack(kind, A, b_acts)
    check_actions(kind, got, r.det, r.det_tie, errs, r.full)
    _, b_lp2, _ = launch(actor, None, obs, kind, A, forced=b_acts.cuda())
    assert bits_equal(b_lp, b_lp2), "deterministic log-probs differ from their forced evaluation"
    errs.close("logp", b_lp, lp64(got), lp32(got))
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
    print(errs.line(f"{C.SID(r.shape)} wide {'frac' if r.frac else 'int'} N {r.N} E {r.E}{rows}{' het' if r.dims else ''}"))
    total.merge(errs)
    return dict(a_lp=a_lp, a_val=a_val, b_acts=b_acts, b_lp=b_lp, c_acts=c_acts, c_lp=c_lp)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_parity_at_batch_edges(shape):
    for frac in (False, True):
        errs = Errors()
        full = ref(shape, 5, O.E_MAX, None, frac)
        big = run_modes(full, errs)
        for E1 in O.E_EDGES[:-1]:
            assert_rows_equal(run_modes(full.rows(0, E1), errs), big, 0, E1, f"E {E1}")
        tail = run_modes(full.rows(33, O.E_MAX), errs, env_base=O.RNG["env_base"] + 33, rows=" rows [33:]")
        assert_rows_equal(tail, big, 33, O.E_MAX, "rows [33:]")
        print(errs.line(f"ALL {C.SID(shape)} wide {'frac' if frac else 'int'} N 5"))


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_parity_at_other_agent_counts(shape):
    for frac in (False, True):
        errs = Errors()
        for N, E, dims in C.batches(shape)[1:]:
            run_modes(ref(shape, N, E, None if dims is None else tuple(dims), frac), errs)
        print(errs.line(f"ALL {C.SID(shape)} wide {'frac' if frac else 'int'} N 1, 8, 3, het"))


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_argument_variants(shape):
    kind, F, H, A = shape
    r = ref(shape, 5, O.E_MAX, None, False)
    actor, critic = device_nets(shape, 5, None)
    obs = pad_obs(r.obs)
    forced = pack(kind, r.forced).cuda()
    base = {"forced": launch(actor, critic, obs, kind, A, forced=forced),
            "smp": launch(actor, critic, obs, kind, A, **O.RNG)}
    same = lambda x, y: torch.equal(x[0], y[0]) and bits_equal(x[1], y[1]) and bits_equal(x[2], y[2])  # noqa: E731
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
    if A > 1:
        assert not torch.equal(launch(actor, critic, obs, kind, A, **rng)[0], base["smp"][0]), "rng_step is ignored"


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_poisoned_neighbour_rows(shape):
    """Agent 1's whole obs rows are NaN: the other agents' outputs do not change by a bit."""
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


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_compact_record_equals_fp32_rows(shape):
    """64-byte record rows (D2D_RECORD_BYTES(32..63) = 64) against fp32 rows of the same integers: the same bits,
    also with heterogeneous in_dims (narrow agents: the record's chunk 1 holds their bias byte only)."""
    kind, F, H, A = shape
    from d2dhip import _lib
    assert _lib.record_bytes(F) == 64
    for dims in [None] + ([C.HET[shape]] if shape in C.HET else []):
        full = ref(shape, 5, O.E_MAX, None if dims is None else tuple(dims), False)
        actor, critic = device_nets(shape, 5, None if dims is None else tuple(dims))
        for E1 in (1, 17, 33, O.E_MAX):
            r = full.rows(0, E1)
            rows, rec = pad_obs(r.obs), pad_record(r.obs)
            assert rec.data.shape[-1] == 64
            forced = pack(kind, r.forced).cuda()
            for kw in (dict(forced=forced), dict(deterministic=True), dict(O.RNG)):
                a0, lp0, v0 = launch(actor, critic, rows, kind, A, **kw)
                a1, lp1, v1 = launch(actor, critic, rec, kind, A, **kw)
                assert torch.equal(a0, a1) and bits_equal(lp0, lp1) and bits_equal(v0, v1), (E1, kw.keys())


@pytest.mark.parametrize("kind", ["comb", "chsel"])
def test_clamp_at_the_extreme_probabilities(kind):
    """w2 = 0 and b2 = (+30, -30, 0, 0): p = (1 - 2e-13, 9e-27, 9e-14, 9e-14) for every input.  Forced on action 0 and
    on action 1, the log-probs are the clamped ones (p in [2^-23, 1 - 2^-23], torch's float32 eps) within 1e-5."""
    N, E, F, H, A = 3, 33, 46, 100, 4
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
def test_empty_batch_writes_nothing(E, N):
    from d2dhip import _lib
    lib = _lib.require_gpu()
    F, H, A = 46, 128, 4
    t = torch.zeros(65536, device="cuda")                   # stands for every input: never read
    abuf = torch.full((256,), SENT_B, dtype=torch.uint8, device="cuda")
    lbuf = torch.full((256,), SENT_F, dtype=torch.int32, device="cuda")
    vbuf = torch.full((256,), SENT_F, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    for forced in (None, p):
        for det in (0, 1):
            desc = _lib.MlpDesc(N, E, F, H, A, 1, p, p, p, p, p, p, p, p, 1234, 77)
            rc = lib.d2d_policy_mlp_wide_step(desc, p, forced, 5, det, abuf[GUARD:].data_ptr(), lbuf[GUARD:].data_ptr(),
                                              vbuf[GUARD:].data_ptr(), _lib.stream_ptr())
            assert rc == 0, lib.d2d_last_error()
    torch.cuda.synchronize()
    assert bool((abuf == SENT_B).all()) and bool((lbuf == SENT_F).all()) and bool((vbuf == SENT_F).all())
