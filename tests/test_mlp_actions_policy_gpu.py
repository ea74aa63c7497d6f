"""The behaviour-policy slot for 17..32 action ids (d2d_policy_mlp_actions_step, csrc/mlp_actions_kernels.hip
policy_actions_kernel) against the float64 oracle of tests/mlp_oracle.py, by the criteria of
tests/test_policy_edges_gpu.py, whose guarded launch and comparisons it imports: obs, actions, log-probs
and values are interior views between NaN / sentinel guards that stay bit-intact, and no NaN comes out.

Shapes: mlp_actions_cases.SHAPES.  Batches: E in {1, 15, 16, 17, 31, 32, 33, 129} at N = 5 (the 16-env tile and the
4-wave workgroup), N = 1 and 8 at E = 129, heterogeneous in_dims; integer and fractional obs.
tests/test_mlp_actions_cpu.py checks on the oracle alone that these inputs are well conditioned.

Parity: |kernel - f64| <= max(1e-5, 2 |torch fp32 on the CPU - f64|), elementwise, for forced log-probs and values.
Sampled and deterministic ids equal the oracle's (host Philox on the same counter, float64 CDF over ids 0 .. A - 1;
first index of the maximum) outside its tie mask; for A = 17 and A = 32 every id of tile 1 is drawn; their log-probs
equal BIT FOR BIT the forced evaluation of the same ids.  Bitwise too: the same envs in a smaller batch or from row 33
on with env_base + 33; rng_step = s with the device word o against rng_step = s + o; want_value = False /
want_actions = False; every agent beside a NaN-poisoned one.  The clamp is hit on purpose; empty batches write
nothing; the record input is refused with nothing written."""
import ctypes
import functools

import pytest

import mlp_actions_cases as C
import mlp_oracle as O
from test_policy_edges_gpu import (GUARD, SENT_B, SENT_F, Errors, assert_rows_equal, bits_equal, check_actions, launch,
                                   pack, pad_obs, pad_record, unpack)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
KIND = C.KIND


def ref(shape, N, E, dims, frac):
    from d2dhip import _lib
    assert _lib.mlp_actions(shape[1], shape[2], shape[3], 1), "every shape of this file runs on the new entry point"
    return C.policy_ref(shape, N, E, dims, frac)


@functools.lru_cache(maxsize=8)
def device_nets(shape, N, dims):
    r = ref(shape, N, C.E_MAX, dims, False)
    to = lambda net: {k: v.cuda().contiguous() for k, v in net.items()}  # noqa: E731
    return to(r.actor), to(r.critic)


def run_modes(r, total, env_base=None, rows=""):
    """The three modes of one run against the reference r: (a) forced with the critic, (b) deterministic without it,
    (c) sampled with the critic.  Returns every output for the bitwise comparisons between runs."""
    kind, F, H, A = r.shape
    errs = Errors()
    actor, critic = device_nets(r.shape, r.N, None if r.dims is None else tuple(r.dims))
    obs = pad_obs(r.obs)
    lp64 = lambda acts: O.logp(r.p64, kind, acts)  # noqa: E731
    lp32 = lambda acts: O.logp(r.p32, kind, acts)  # noqa: E731
    forced = pack(kind, r.forced).cuda()
    a_acts, a_lp, a_val = launch(actor, critic, obs, kind, A, forced=forced)
    assert torch.equal(a_acts, forced.cpu()), "forced ids are returned as given"
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
    print(errs.line(f"{C.SID(r.shape)} {'frac' if r.frac else 'int'} N {r.N} E {r.E}{rows}{' het' if r.dims else ''}"))
    total.merge(errs)
    return dict(a_lp=a_lp, a_val=a_val, b_acts=b_acts, b_lp=b_lp, c_acts=c_acts, c_lp=c_lp)


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_parity_at_batch_edges(shape):
    A = shape[3]
    for frac in (False, True):
        errs = Errors()
        full = ref(shape, 5, C.E_MAX, None, frac)
        big = run_modes(full, errs)
        if shape in C.TILE1_SHAPES:
            drawn = set(big["c_acts"].reshape(-1).tolist())
            assert set(range(16, A)) <= drawn, f"ids of tile 1 never drawn: {sorted(set(range(16, A)) - drawn)}"
        for E1 in C.E_EDGES[:-1]:
            assert_rows_equal(run_modes(full.rows(0, E1), errs), big, 0, E1, f"E {E1}")
        tail = run_modes(full.rows(33, C.E_MAX), errs, env_base=O.RNG["env_base"] + 33, rows=" rows [33:]")
        assert_rows_equal(tail, big, 33, C.E_MAX, "rows [33:]")
        print(errs.line(f"ALL {C.SID(shape)} {'frac' if frac else 'int'} N 5"))


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_parity_at_other_agent_counts(shape):
    for frac in (False, True):
        errs = Errors()
        for N, E, dims in C.batches(shape)[1:]:
            run_modes(ref(shape, N, E, None if dims is None else tuple(dims), frac), errs)
        print(errs.line(f"ALL {C.SID(shape)} {'frac' if frac else 'int'} N 1, 8, het"))


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_argument_variants(shape):
    kind, F, H, A = shape
    r = ref(shape, 5, C.E_MAX, None, False)
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
    # the actor-only instantiation gives the actor's bits
    a7, lp7, v7 = launch(actor, None, obs, kind, A, **O.RNG)
    assert v7 is None and torch.equal(a7, base["smp"][0]) and bits_equal(lp7, base["smp"][1])
    # the device word rng_offset: rng_step = s with the word o is rng_step = s + o with none
    o = 3
    word = torch.tensor([o], dtype=torch.int32, device="cuda")
    rng = dict(O.RNG, rng_step=O.RNG["rng_step"] - o)
    assert same(launch(actor, critic, obs, kind, A, rng_offset=word.data_ptr(), **rng), base["smp"])
    assert not torch.equal(launch(actor, critic, obs, kind, A, **rng)[0], base["smp"][0]), "rng_step is ignored"


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_poisoned_neighbour_rows(shape):
    """Agent 1's whole obs rows are NaN: the other agents' outputs do not change by a bit."""
    kind, F, H, A = shape
    for frac in (False, True):
        r = ref(shape, 5, C.E_MAX, None, frac)
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


def test_clamp_at_the_extreme_probabilities():
    """w2 = 0 and b2 = +30 at id 0, -30 at ids 1 and 16, 0 elsewhere: p_0 > 1 - 2^-23 and p_1 = p_16 < 2^-23 for
    every input.  Forced on each, the log-probs are the clamped ones (p in [2^-23, 1 - 2^-23]) within 1e-5."""
    N, E, F, H, A = 3, 33, 24, 64, 17
    actor, _ = O.make_params(N, F, H, A, 5)
    actor["w2"] = torch.zeros(N, A, H)
    b2 = torch.zeros(A)
    b2[0], b2[1], b2[16] = 30.0, -30.0, -30.0
    actor["b2"] = b2.expand(N, A).contiguous()
    obs = O.make_obs(E, N, F, None, 6, False)
    p64 = O.probs(actor, obs)
    assert p64[..., 0].min().item() > 1 - 2.0 ** -23 and p64[..., 1].max().item() < 2.0 ** -23
    dev = {k: v.cuda().contiguous() for k, v in actor.items()}
    for a in (0, 1, 16):
        acts = torch.full((N, E), a)
        _, lp, _ = launch(dev, None, pad_obs(obs), KIND, A, forced=pack(KIND, acts).cuda())
        want = O.logp(p64, KIND, acts)
        assert abs(want[0, 0].item() - (-(2.0 ** -23) if a == 0 else -15.942385)) < 1e-4
        assert (lp.double() - want).abs().max().item() <= 1e-5, (a, lp[0, 0].item(), want[0, 0].item())


@pytest.mark.parametrize("E,N", [(0, 5), (33, 0), (0, 0)])
def test_empty_batch_writes_nothing(E, N):
    from d2dhip import _lib
    lib = _lib.require_gpu()
    F, H, A = 24, 128, 17
    t = torch.zeros(65536, device="cuda")                   # stands for every input: never read
    abuf = torch.full((256,), SENT_B, dtype=torch.uint8, device="cuda")
    lbuf = torch.full((256,), SENT_F, dtype=torch.int32, device="cuda")
    vbuf = torch.full((256,), SENT_F, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(t.data_ptr())
    for forced in (None, p):
        for det in (0, 1):
            desc = _lib.MlpDesc(N, E, F, H, A, 1, p, p, p, p, p, p, p, p, 1234, 77)
            rc = lib.d2d_policy_mlp_actions_step(desc, p, forced, 5, det, abuf[GUARD:].data_ptr(),
                                                 lbuf[GUARD:].data_ptr(), vbuf[GUARD:].data_ptr(), _lib.stream_ptr())
            assert rc == 0, lib.d2d_last_error()
    torch.cuda.synchronize()
    assert bool((abuf == SENT_B).all()) and bool((lbuf == SENT_F).all()) and bool((vbuf == SENT_F).all())


def test_record_input_is_refused_with_nothing_written():
    shape = C.SHAPES[0]
    kind, F, H, A = shape
    r = ref(shape, 5, C.E_MAX, None, False).rows(0, 17)
    actor, critic = device_nets(shape, 5, None)
    rec = pad_record(r.obs)
    for kw in (dict(forced=pack(kind, r.forced).cuda()), dict(deterministic=True), dict(O.RNG)):
        launch(actor, critic, rec, kind, A, refused=NotImplementedError, **kw)
