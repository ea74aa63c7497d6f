"""The iRDQN kernels (csrc/rdqn_kernels.hip: rdqn_q_kernel<REC, CARRY>, rdqn_bptt_kernel<REC>, rdqn_wgrad_kernel, and
the helpers they take from csrc/gru_l2_common.h) at every hidden and input tile count, ragged size, load branch and edge
rule, against float64 torch (tests/irdqn_oracle.py; the input sets and their references are tests/irdqn_cases.py's,
shared with tests/test_irdqn_edges_cpu.py, which asserts on the CPU the conditions that make every comparison here
strict).

Shapes are the smallest at which each path exists: N = 2 agents, E = 3 envs, B = 17 samples (a full 16-sample tile and
a tile of one), 3-step windows on a ring of 7 rows, F = 30, H = 50, A = 8, one size varying at a time.  Tolerances:
Q-values 1e-5 absolute; qmax and the greedy action bitwise the max / lowest-index argmax of the kernel's own q, and
float64's argmax wherever its margin exceeds 1e-5 (at most 1 % of a set's decisions may be closer); every *block* of
every gradient (irdqn_cases.blocks: each gate of the GRU tensors and each hidden head layer, the rows of the last hidden
tile and the rest apart; w3; b3) within 2e-5 max|g64 of that block| + 1e-7 of float64 autograd; the loss rtol 1e-5,
atol 1e-7 -- with no fallback to torch fp32's band and no tensor-wide scale.  Every output, and every input but the
parameters, lives inside a 0xFF-filled (NaN) guarded buffer; every guard must be intact after every call and every
output finite.  The gradient entry is called through ctypes on its own workspace of exactly d2d_rdqn_grad_workspace
floats, guarded and NaN-filled (and once zero-filled: bitwise the same), with the ten gradient tensors and the loss
NaN-pre-filled.  Each comparison prints |kernel - f64| beside torch fp32's own distance.

What this file found: no defect.  The kernels as they were pass all 187 tests (5 s on an MI355X): Q-values at most
2.1e-7 from float64 (torch fp32: 1.8e-7) against 1e-5; the worst gradient block at 0.22 of its own tolerance (the
non-last rows of a W_ih gate with the ring times 40, where torch fp32 is at 0.21), at unit input scale at 0.052 (torch
fp32: 0.033), the median set's worst block at 0.02; every guard intact, no output left unwritten on a NaN-filled
workspace.  That the tests can fail was checked with four one-line changes on an uncommitted copy, each of which the
suite as it was let pass: the draw taken from Philox stream 3 and `u > eps` for `u >= eps` both fail
test_epsilon_greedy_draws_are_pinned_to_philox, dropping `act >= a.A` from the exclusion fails
test_excluded_and_two_bit_action_masks (the loss), and dropping the Q kernel's kMaxWindow clamp fails
test_env_and_window_clamps."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import gru_oracle as O  # noqa: E402
import irdqn_cases as C  # noqa: E402
from mlp_oracle import to_record  # noqa: E402
from oracle.philox import philox4x32_10  # noqa: E402
from test_irdqn_gpu import masks_to_idx  # noqa: E402

DEV = "cuda"
CASES = C.all_cases()
STREAM_RDQN = 4             # the Philox stream of the epsilon-greedy draw (3 is the policies' sampling)


class Guards:
    """guarded device buffers of one test and their checks"""

    def __init__(self):
        self.checks = []

    def put(self, what, src):
        v, chk = O.guarded(src=src.contiguous())
        self.checks.append((chk, what))
        return v

    def new(self, what, shape, dtype, fill=None):
        v, chk = O.guarded(shape=tuple(shape), dtype=dtype)
        self.checks.append((chk, what))
        if fill is not None:
            v.fill_(fill)
        return v

    def check(self):
        torch.cuda.synchronize()
        for chk, what in self.checks:
            chk(what)


def params_dev(p):
    return {k: v.to(DEV).contiguous() for k, v in p.items()}


def samples_dev(g, samples):
    return g.put("samples", torch.tensor(samples, dtype=torch.int32).view(-1, 3))


def record_of(g, ring):
    """the compact record of an integer ring, its bytes in a guarded buffer"""
    from d2dhip.record import ObsRecord
    rec = to_record(ring)
    return ObsRecord(g.put("record", rec.data), rec.obs_dim, rec.signed)


def run_q(g, pd, ring_d, s_d, want=(True, True, True), **kw):
    """One Q launch into guarded outputs -> (q, qmax, action masks), None where not wanted"""
    from d2dhip import rdqn
    N, A, B = pd["w3"].shape[0], pd["w3"].shape[1], s_d.shape[0]
    out = {}
    if want[0]:
        out["q"] = g.new("q", (N, B, A), torch.float32)
    if want[1]:
        out["qmax"] = g.new("qmax", (N, B), torch.float32)
    if want[2]:
        out["action"] = g.new("action", (B, N), rdqn.mask_dtype(A))
    q, qmax, act = rdqn.q_values(pd, ring_d, s_d, want_q=want[0], want_qmax=want[1], want_action=want[2], out=out, **kw)
    g.check()
    assert (q is None) == (not want[0]) and (qmax is None) == (not want[1]) and (act is None) == (not want[2])
    for t in (q, qmax):
        assert t is None or bool(torch.isfinite(t).all()), "an output was not written (NaN) or is not finite"
    if act is not None:
        masks_to_idx(act)                                                     # every mask written, and one-hot
    return q, qmax, act


def masks_of(act, A):
    from d2dhip import rdqn
    return (torch.ones_like(act) << act).to(rdqn.mask_dtype(A))


def td_dev(g, c, act_masks, reward, done, qt):
    """the TD inputs in guarded buffers: (masks [B][N], reward [B][N], done [B] uint8, qmax_target [N][B])"""
    from d2dhip import rdqn
    return (g.put("action masks", act_masks.to(rdqn.mask_dtype(c.A))), g.put("reward", reward.float()),
            g.put("done", done.to(torch.uint8)), g.put("qmax_target", qt.float()))


def run_grad(g, pd, ring_d, s_d, L, td, loss, ring_episode=0, ws_fill=float("nan"), plain=False):
    """d2d_rdqn_grad_ex (plain: d2d_rdqn_grad) through ctypes on its own guarded workspace of exactly the floats the
    library asks for; the gradients and the loss go to NaN-filled guarded tensors -> (grads, loss [N])"""
    from d2dhip import _lib, rdqn
    from d2dhip.record import obs_arg
    lib = _lib.require_gpu()
    d = rdqn.desc(pd, ring_d, ring_episode)
    B = s_d.shape[0]
    n = lib.d2d_rdqn_grad_workspace(ctypes.byref(d), B, L)
    assert n > 0
    ws = g.new("workspace", (n,), torch.float32, fill=ws_fill)
    grads = {name: g.new("g_" + name, pd[name].shape, torch.float32) for name in C.NAMES}
    ls = g.new("loss", (d.n_agents,), torch.float32)
    assert all(bool(torch.isnan(t).all()) for t in list(grads.values()) + [ls])
    masks, reward, done, qt = td
    obs_p, fmt, sgn = obs_arg(ring_d)
    tail = (s_d.data_ptr(), B, L, masks.data_ptr(), reward.data_ptr(), done.data_ptr(), qt.data_ptr(), C.GAMMA,
            rdqn.LOSS[loss], *(grads[name].data_ptr() for name in C.NAMES), ls.data_ptr(), ws.data_ptr(), n,
            _lib.stream_ptr())
    if plain:
        assert fmt == _lib.D2D_OBS_F32
        rc = lib.d2d_rdqn_grad(ctypes.byref(d), obs_p, *tail)
    else:
        rc = lib.d2d_rdqn_grad_ex(ctypes.byref(d), obs_p, fmt, sgn, *tail)
    _lib.check(rc, "d2d_rdqn_grad")
    g.check()
    for name in C.NAMES:
        assert bool(torch.isfinite(grads[name]).all()), f"{name}: an element was not written (NaN) or is not finite"
    assert bool(torch.isfinite(ls).all())
    return grads, ls


def same_grads(x, y, what):
    for name in C.NAMES:
        assert torch.equal(x[0][name], y[0][name]), (what, name)
    assert torch.equal(x[1], y[1]), (what, "loss")


def check_blocks(c, got, ls, g64, l64, g32, what):
    """every block within GRAD_RTOL max|g64 of the block| + GRAD_ATOL; the loss rtol 1e-5, atol 1e-7"""
    worst, lines, bad = 0.0, [], []
    host = {name: got[name].cpu().double() for name in C.NAMES}
    for label, name, idx in C.blocks(c):
        assert host[name].shape == g64[name].shape
        ref = g64[name][idx]
        tol = C.block_tol(ref)
        err = (host[name][idx] - ref).abs().max().item()
        band = (g32[name][idx] - ref).abs().max().item()
        lines.append(f"{label} {err:.1e}/{band:.1e}/{tol:.1e}")
        worst = max(worst, err / tol)
        if err > tol:
            bad.append((label, err, tol, band))
    print(f"  {what}: per block |kernel - f64| / |torch fp32 - f64| / the block's tolerance: " + "  ".join(lines))
    print(f"  {what}: worst block at {worst:.3f} of its tolerance; loss {ls.cpu().tolist()} (f64 {l64.tolist()})")
    assert not bad, (what, bad)
    torch.testing.assert_close(ls.cpu().double(), l64, rtol=1e-5, atol=1e-7)


def check_q(r, q, qmax, act, shift=0, what=""):
    q64 = r.q(torch.float64, shift)
    qc = q.cpu()
    err = (qc.double() - q64).abs().max().item()
    band = (r.q(torch.float32, shift) - q64).abs().max().item()
    print(f"  {what}: max |kernel - f64| {err:.2e}  |torch fp32 - f64| {band:.2e}")
    assert err <= 1e-5, (what, err)
    check_greedy(qc, qmax, act)
    clear = r.margin(shift) > O.TIE                                           # [N][B]
    assert (~clear).double().mean().item() <= 0.01
    assert torch.equal(masks_to_idx(act).t()[clear], q64.argmax(-1)[clear]), what


def check_greedy(qc, qmax, act):
    """qmax and the action are the max and the lowest-index argmax of the kernel's own q, bitwise"""
    assert torch.equal(qmax.cpu(), qc.max(-1).values)
    first = (qc == qc.max(-1, keepdim=True).values).int().argmax(-1)         # lowest index among ties
    assert torch.equal(masks_to_idx(act), first.t())


# ------------------------------------------------------------------------------------------- all sets

@pytest.mark.parametrize("c", CASES, ids=C.cid)
def test_q_matches_float64(c):
    """window lengths 1, 2 and L mixed inside one tile; the episode ring with row_shift 0 and 1"""
    r = C.ref(c)
    g = Guards()
    pd, ring_d, s_d = params_dev(r.p), g.put("ring", r.ring), samples_dev(g, r.qsamples)
    for shift in r.shifts():
        q, qmax, act = run_q(g, pd, ring_d, s_d, ring_episode=c.ep, row_shift=shift)
        check_q(r, q, qmax, act, shift, f"row_shift {shift}")


@pytest.mark.parametrize("loss", C.LOSSES)
@pytest.mark.parametrize("c", CASES, ids=C.cid)
def test_grads_match_float64_per_block(c, loss):
    r = C.ref(c)
    g64, l64, _, g32, _ = r.td(loss)
    g = Guards()
    pd, ring_d, s_d = params_dev(r.p), g.put("ring", r.ring), samples_dev(g, r.samples)
    td = td_dev(g, c, masks_of(r.act, c.A), r.reward, r.done, r.qt)
    got = run_grad(g, pd, ring_d, s_d, c.L, td, loss, ring_episode=c.ep)
    check_blocks(c, got[0], got[1], g64, l64, g32, loss)
    for k, d in enumerate(r.dims):                                            # unused inputs: exactly zero
        assert bool((got[0]["w_ih"][k, :, d:] == 0).all())
    if c.L == 1:
        assert bool((got[0]["w_hh"] == 0).all())
    same_grads(got, run_grad(g, pd, ring_d, s_d, c.L, td, loss, ring_episode=c.ep), "a second run")
    same_grads(got, run_grad(g, pd, ring_d, s_d, c.L, td, loss, ring_episode=c.ep, ws_fill=0.0),
               "a zero-filled workspace")


def test_the_wrapper_fills_given_gradient_tensors():
    """d2dhip.rdqn.grads with NaN-pre-filled grads= / loss_out= (its own reused workspace): bitwise the ctypes call"""
    from d2dhip import rdqn
    c = C.BASE
    r = C.ref(c)
    g = Guards()
    pd, ring_d, s_d = params_dev(r.p), g.put("ring", r.ring), samples_dev(g, r.samples)
    td = td_dev(g, c, masks_of(r.act, c.A), r.reward, r.done, r.qt)
    for loss in C.LOSSES:
        want = run_grad(g, pd, ring_d, s_d, c.L, td, loss)
        grads = {name: g.new("g_" + name, pd[name].shape, torch.float32) for name in C.NAMES}
        ls = g.new("loss", (c.N,), torch.float32)
        got = rdqn.grads(pd, ring_d, s_d, c.L, *td, C.GAMMA, loss, grads=grads, loss_out=ls)
        g.check()
        assert got[0] is grads and got[1] is ls
        same_grads(got, want, loss)


# ------------------------------------------------------------------------------------------- lane independence

def test_every_sample_of_a_mixed_tile_is_its_own():
    """the q row, qmax and action of every sample of a mixed-length tile are bitwise those of the same sample launched
    alone (B = 1) and launched as the last of 17 (lane 0 of a second tile)"""
    c = C.BASE
    r = C.ref(c)
    g = Guards()
    pd, ring_d = params_dev(r.p), g.put("ring", r.ring)
    q, qmax, act = run_q(g, pd, ring_d, samples_dev(g, r.qsamples))
    assert {s[2] for s in r.qsamples[:16]} == {1, 2, c.L}
    for b, s in enumerate(r.qsamples):
        for batch, at in (([s], 0), ([x for i, x in enumerate(r.qsamples) if i != b] + [s], c.B - 1)):
            gb = Guards()
            q1, m1, a1 = run_q(gb, pd, ring_d, samples_dev(gb, batch))
            assert torch.equal(q1[:, at], q[:, b]) and torch.equal(m1[:, at], qmax[:, b]), (b, at)
            assert torch.equal(a1[at], act[b]), (b, at)


@pytest.mark.parametrize("loss", C.LOSSES)
def test_one_sample_alone_gives_its_own_gradients(loss):
    """B = 1 (fifteen padding lanes beside it): every block within its tolerance of float64 autograd of that sample"""
    c = C.BASE
    r = C.ref(c)
    pd = params_dev(r.p)
    for b in C.SINGLES:
        samples, act, reward, done, qt = C.single(r, b)
        with C.one_thread():
            g64, l64, _ = C.td_ref(c, r.p, r.ring, samples, act, reward, done, qt, loss, torch.float64)
            g32, _, _ = C.td_ref(c, r.p, r.ring, samples, act, reward, done, qt, loss, torch.float32)
        g = Guards()
        td = td_dev(g, c, masks_of(act, c.A), reward, done, qt)
        got = run_grad(g, pd, g.put("ring", r.ring), samples_dev(g, samples), c.L, td, loss)
        check_blocks(c, got[0], got[1], g64, l64, g32, f"sample {b}")


# ------------------------------------------------------------------------------------------- unaligned parameters

def off_by_one_float(t):
    """a contiguous copy of t one float into a 16-byte aligned buffer: data_ptr() % 16 == 4"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("name", ["w_ih", "w_hh", "w1", "w2", "w3"])
def test_an_unaligned_parameter_changes_no_bit(name):
    """F = 16, H = 52: every fragment load is a 16-byte one until a parameter tensor is not 16-byte aligned; then the
    same products in the same order are loaded as scalars"""
    c = C.UNALIGNED
    assert c.F % 4 == 0 and c.H % 4 == 0
    r = C.ref(c)
    g = Guards()
    pd, ring_d = params_dev(r.p), g.put("ring", r.ring)
    assert all(v.data_ptr() % 16 == 0 for v in pd.values())
    pu = dict(pd)
    pu[name] = off_by_one_float(pd[name])
    sq, sg = samples_dev(g, r.qsamples), samples_dev(g, r.samples)
    td = td_dev(g, c, masks_of(r.act, c.A), r.reward, r.done, r.qt)
    want, got = run_q(g, pd, ring_d, sq), run_q(g, pu, ring_d, sq)
    for x, y in zip(want, got):
        assert torch.equal(x, y)
    check_q(r, *got, what=f"unaligned {name}")
    for loss in C.LOSSES:
        same_grads(run_grad(g, pu, ring_d, sg, c.L, td, loss), run_grad(g, pd, ring_d, sg, c.L, td, loss), (name, loss))


# ------------------------------------------------------------------------------------------- acting

SEED = 0x9E3779B97F4A7C15    # a 64-bit seed with both key words set
ENV_BASE = 2 ** 32 - 2      # the env index wraps: envs 0, 1, 2 draw as 2^32 - 2, 2^32 - 1, 0


def draws(envs, N, seed, env_base, rng):
    """(u float32 [B][N], explore action [B][N]) of the epsilon-greedy draw, from oracle/philox.py"""
    e = ((env_base + np.asarray(envs, dtype=np.uint64)) % np.uint64(2 ** 32))[:, None]
    w = philox4x32_10(e, np.arange(N)[None, :], rng % 2 ** 32, STREAM_RDQN << 24, seed)
    u = (w[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u, (w[1] & np.uint64(1)).astype(np.int64)


def expected_actions(u, explore_action, greedy, eps_rows, ready):
    explore = ~(bool(ready) & (u >= np.asarray(eps_rows, dtype=np.float32)[:, None]))
    return torch.from_numpy(np.where(explore, explore_action, greedy))


def acting_setup(g):
    """the base set with an output bias that makes action A - 1 every greedy choice: explore actions (0 / 1) show"""
    c = C.BASE
    r = C.ref(c)
    p = {k: v.clone() for k, v in r.p.items()}
    p["b3"][:, c.A - 1] += 100.0
    pd, ring_d = params_dev(p), g.put("ring", r.ring)
    samples = r.qsamples
    assert {s[0] for s in samples} == set(range(c.E))
    return c, pd, ring_d, samples


def test_epsilon_greedy_draws_are_pinned_to_philox():
    g = Guards()
    c, pd, ring_d, samples = acting_setup(g)
    s_d = samples_dev(g, samples)
    envs = [s[0] for s in samples]
    greedy = masks_to_idx(run_q(g, pd, ring_d, s_d)[2]).numpy()
    assert (greedy == c.A - 1).all()
    rng = 0xFFFFFFFF + 3
    u, ea = draws(envs, c.N, SEED, ENV_BASE, rng)
    assert 0 < ea.sum() < ea.size and u.min() >= 0 and u.max() < 1
    # per-sample epsilon: 0 (always greedy), 1 (never), 2.0 (the learner's "not ready"), 0.5, and agent 0's own u --
    # greedy, u >= eps -- and the next float above it -- explore
    eps = np.zeros(c.B, dtype=np.float32)
    for b in range(c.B):
        eps[b] = (0.0, 1.0, 2.0, 0.5, u[b, 0], np.nextafter(u[b, 0], np.float32(1)))[b % 6]
    want = expected_actions(u, ea, greedy, eps, True)
    at_u, above_u = np.arange(c.B) % 6 == 4, np.arange(c.B) % 6 == 5
    assert (want.numpy()[at_u, 0] == c.A - 1).all() and (want.numpy()[above_u, 0] <= 1).all()
    role = np.arange(c.B) % 6
    assert (want.numpy()[role == 0] == c.A - 1).all() and (want.numpy()[role == 2] <= 1).all()
    eps_d = g.put("eps_rows", torch.from_numpy(eps))
    off = g.put("rng_offset", torch.tensor([3], dtype=torch.int32))
    kw = dict(mode="eps", seed=SEED, env_base=ENV_BASE, eps_rows=eps_d, ready=True)
    q, qmax, act = run_q(g, pd, ring_d, s_d, rng_step=0xFFFFFFFF, rng_offset=off.data_ptr(), **kw)
    assert torch.equal(masks_to_idx(act), want)
    # the device offset wraps with the step: bitwise the launch at step 2
    q2, qmax2, act2 = run_q(g, pd, ring_d, s_d, rng_step=2, **kw)
    assert torch.equal(act2, act) and torch.equal(q2, q) and torch.equal(qmax2, qmax)
    # q and qmax are the greedy launch's whatever the draw
    check_greedy(q.cpu(), qmax, run_q(g, pd, ring_d, s_d)[2])
    # not ready: every choice explores, whatever epsilon
    act_n = run_q(g, pd, ring_d, s_d, rng_step=2, **dict(kw, ready=False))[2]
    assert torch.equal(masks_to_idx(act_n), torch.from_numpy(ea))
    # a scalar epsilon, another step, no env base and seed 0
    u0, ea0 = draws(envs, c.N, 0, 0, 7)
    act_s = run_q(g, pd, ring_d, s_d, mode="eps", eps=0.5, rng_step=7)[2]
    assert torch.equal(masks_to_idx(act_s), expected_actions(u0, ea0, greedy, np.full(c.B, 0.5), True))
    # the draw belongs to (env, agent, step), not to the sample's place in the batch
    perm = np.random.default_rng(0).permutation(c.B)
    gp = Guards()
    act_p = run_q(gp, pd, ring_d, samples_dev(gp, [samples[i] for i in perm]), rng_step=2,
                  **dict(kw, eps_rows=gp.put("eps_rows", torch.from_numpy(eps[perm]))))[2]
    assert torch.equal(act_p.cpu(), act.cpu()[perm])


def test_forced_mode_with_guarded_masks_is_exact():
    g = Guards()
    c, pd, ring_d, samples = acting_setup(g)
    s_d = samples_dev(g, samples)
    gen = torch.Generator().manual_seed(1)
    em = (torch.rand(c.B, c.N, generator=gen) < 0.5).to(torch.uint8)
    ea = torch.randint(0, c.A, (c.B, c.N), generator=gen).to(torch.uint8)
    act = run_q(g, pd, ring_d, s_d, mode="forced", explore_mask=g.put("explore_mask", em),
                explore_action=g.put("explore_action", ea))[2]
    assert bool(em.any()) and not bool(em.all())
    assert torch.equal(masks_to_idx(act), torch.where(em.bool(), ea.long(), torch.full((c.B, c.N), c.A - 1)))


def test_every_combination_of_wanted_outputs():
    g = Guards()
    c, pd, ring_d, samples = acting_setup(g)
    s_d = samples_dev(g, samples)
    kw = dict(mode="eps", seed=SEED, env_base=ENV_BASE, eps=0.5, rng_step=11)
    full = run_q(g, pd, ring_d, s_d, **kw)
    assert bool((masks_to_idx(full[2]) <= 1).any()) and bool((masks_to_idx(full[2]) == c.A - 1).any())
    for bits in range(8):
        want = (bool(bits & 1), bool(bits & 2), bool(bits & 4))
        gw = Guards()
        got = run_q(gw, pd, ring_d, s_d, want=want, **kw)
        for x, y, w in zip(got, full, want):
            assert (x is None and not w) or torch.equal(x, y), (want,)


# ------------------------------------------------------------------------------------------- clamps, invalid actions

def test_env_and_window_clamps():
    """env < 0 and >= E, window lengths 0, -3 and 300 on a ring of 7 rows: bitwise the clamped triples.  The GRU's
    update gate is biased towards keeping its state, so that a window's 256th step back still reaches the Q-values
    (asserted: a window one ring period shorter gives other bits) and a missing clamp of 300 could not hide."""
    c = C.BASE
    r = C.ref(c)
    assert r.rows == 7
    p = {k: v.clone() for k, v in r.p.items()}
    p["b_hh"][:, c.H:2 * c.H] += 4.6                                          # z ~ 0.99
    g = Guards()
    pd, ring_d = params_dev(p), g.put("ring", r.ring)
    E = c.E
    given = [(-1, 2, 3), (E + 5, 4, 2), (1, 3, 0), (2, 5, -3), (0, 6, 300), (1, 1, 256), (-7, 0, 300), (2, 3, 1),
             (E, 5, 257)] + r.qsamples[:8]
    clamped = [(0, 2, 3), (E - 1, 4, 2), (1, 3, 1), (2, 5, 1), (0, 6, 256), (1, 1, 256), (0, 0, 256), (2, 3, 1),
               (E - 1, 5, 256)] + r.qsamples[:8]
    assert len(given) == 17
    got, want = run_q(g, pd, ring_d, samples_dev(g, given)), run_q(g, pd, ring_d, samples_dev(g, clamped))
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    shorter = run_q(g, pd, ring_d, samples_dev(g, [(0, 6, 256 - 7)]))[0]
    assert not torch.equal(shorter[:, 0], want[0][:, 4]), "the window's far end does not reach q: the test is blind"
    # the gradient entry clamps the env and takes L from its argument, not from the triple
    td = td_dev(g, c, masks_of(r.act, c.A), r.reward, r.done, r.qt)
    given = [((-1, E + 5, e)[b % 3] if b < 6 else e, last, (0, -3, 300, L)[b % 4])
             for b, (e, last, L) in enumerate(r.samples)]
    clamped = [((0, E - 1, e)[b % 3] if b < 6 else e, last, L) for b, (e, last, L) in enumerate(r.samples)]
    assert given != clamped
    for loss in C.LOSSES:
        same_grads(run_grad(g, pd, ring_d, samples_dev(g, given), c.L, td, loss),
                   run_grad(g, pd, ring_d, samples_dev(g, clamped), c.L, td, loss), loss)


@pytest.mark.parametrize("loss", C.LOSSES)
def test_excluded_and_two_bit_action_masks(loss):
    """A = 5: masks of 0 and of a bit at or above A (bits 6, 7) are excluded -- their loss and gradient are zero while
    the mean still divides by B -- and a two-bit mask takes its lowest bit.  Reference: float64 with those samples'
    coefficients zeroed."""
    c = C.INVALID
    r = C.ref(c)
    masks, act, weight = C.invalid_actions(r)
    with C.one_thread():
        a = (c, r.p, r.ring, r.samples, act, r.reward, r.done, r.qt, loss)
        g64, l64, _ = C.td_ref(*a, torch.float64, weight=weight)
        g32, _, _ = C.td_ref(*a, torch.float32, weight=weight)
    g = Guards()
    pd, ring_d, s_d = params_dev(r.p), g.put("ring", r.ring), samples_dev(g, r.samples)
    got = run_grad(g, pd, ring_d, s_d, c.L, td_dev(g, c, masks, r.reward, r.done, r.qt), loss)
    check_blocks(c, got[0], got[1], g64, l64, g32, loss)
    # with every sample excluded nothing is left: exact zeros
    none = run_grad(g, pd, ring_d, s_d, c.L, td_dev(g, c, torch.full_like(masks, 1 << 6), r.reward, r.done, r.qt), loss)
    assert all(bool((none[0][name] == 0).all()) for name in C.NAMES) and bool((none[1] == 0).all())


# ------------------------------------------------------------------------------------------- the plain entry points

def test_plain_entry_points_equal_their_ex_forms():
    from d2dhip import _lib, rdqn
    c = C.BASE
    r = C.ref(c)
    g = Guards()
    pd, ring_d = params_dev(r.p), g.put("ring", r.ring)
    s_d = samples_dev(g, r.qsamples)
    eps_d = g.put("eps_rows", torch.linspace(0, 1, c.B))
    kw = dict(mode="eps", seed=SEED, env_base=5, eps_rows=eps_d, rng_step=9)
    want = run_q(g, pd, ring_d, s_d, **kw)
    lib = _lib.require_gpu()
    d = rdqn.desc(pd, ring_d, 0, SEED, 5, None)
    q = g.new("q", (c.N, c.B, c.A), torch.float32)
    qmax = g.new("qmax", (c.N, c.B), torch.float32)
    act = g.new("action", (c.B, c.N), rdqn.mask_dtype(c.A))
    rc = lib.d2d_rdqn_q(ctypes.byref(d), ring_d.data_ptr(), s_d.data_ptr(), c.B, 0, _lib.D2D_RDQN_EPS, 0.0,
                        eps_d.data_ptr(), 1, None, None, 9, q.data_ptr(), qmax.data_ptr(), act.data_ptr(),
                        _lib.stream_ptr())
    _lib.check(rc, "d2d_rdqn_q")
    g.check()
    for x, y in zip((q, qmax, act), want):
        assert torch.equal(x, y)
    assert bool((masks_to_idx(act) <= 1).any())
    sg = samples_dev(g, r.samples)
    td = td_dev(g, c, masks_of(r.act, c.A), r.reward, r.done, r.qt)
    for loss in C.LOSSES:
        same_grads(run_grad(g, pd, ring_d, sg, c.L, td, loss, plain=True), run_grad(g, pd, ring_d, sg, c.L, td, loss),
                   loss)


# ------------------------------------------------------------------------------------------- record, carry

REC_CASES = [C.BASE, C.case(F=63)]     # a ragged narrow set (HT = 4, IT = 2) and IT = 4


@pytest.mark.parametrize("c", REC_CASES, ids=C.cid)
def test_record_instances_equal_the_fp32_ring_bitwise(c):
    """integer inputs (the set's ring rounded down: -1 .. 3, int8 and uint8 columns): rdqn_q_kernel<true, false> and
    rdqn_bptt_kernel<true> give the bits of the fp32 instances"""
    r = C.ref(c)
    ring = r.ring.floor()
    assert ring.min() == -1 and ring.max() == 3
    g = Guards()
    pd, ring_d, rec = params_dev(r.p), g.put("ring", ring), record_of(g, ring)
    assert torch.equal(rec.decode(), ring_d)
    sq, sg = samples_dev(g, r.qsamples), samples_dev(g, r.samples)
    for x, y in zip(run_q(g, pd, rec, sq), run_q(g, pd, ring_d, sq)):
        assert torch.equal(x, y)
    td = td_dev(g, c, masks_of(r.act, c.A), r.reward, r.done, r.qt)
    for loss in C.LOSSES:
        got = run_grad(g, pd, rec, sg, c.L, td, loss)
        same_grads(got, run_grad(g, pd, ring_d, sg, c.L, td, loss), loss)
        assert got[0]["w_ih"].abs().max() > 0


@pytest.mark.parametrize("fmt", ["f32", "record"])
@pytest.mark.parametrize("c", REC_CASES, ids=C.cid)
def test_carried_acting_equals_the_recompute_bitwise(c, fmt):
    """four acting slots (slot t: row t, window t + 1): slots 1 .. 3 run one GRU step on the carried h (in a guarded,
    NaN-filled scratch of exactly d2d_rdqn_carry_floats floats); q, qmax and the epsilon-greedy actions are bitwise
    those of the window's recompute"""
    from d2dhip import _lib, rdqn
    r = C.ref(c)
    ring = r.ring.floor()
    g = Guards()
    pd = params_dev(r.p)
    ring_d = g.put("ring", ring) if fmt == "f32" else record_of(g, ring)
    lib = _lib.require_gpu()
    n = lib.d2d_rdqn_carry_floats(ctypes.byref(rdqn.desc(pd, ring_d)), c.B)
    assert n == c.N * 32 * 16 * C.tiles(c)[0]
    st = rdqn.CarryState()
    st.h = g.new("hcarry", (n,), torch.float32)
    h0 = st.h
    s = torch.zeros((c.B, 3), dtype=torch.int32)
    s[:, 0] = torch.arange(c.B) % c.E
    s_d = g.put("samples", s)
    for t in range(4):
        s_d[:, 1], s_d[:, 2] = t, t + 1
        kw = dict(mode="eps", eps=0.5, seed=SEED, rng_step=t)
        got = run_q(g, pd, ring_d, s_d, carry=st, row=t, window=t + 1, **kw)
        assert st.h is h0 and bool(torch.isfinite(st.h).all())
        want = run_q(g, pd, ring_d, s_d, **kw)
        for x, y in zip(got, want):
            assert torch.equal(x, y), t
    assert (st.carried, st.recomputed) == (3, 1)
