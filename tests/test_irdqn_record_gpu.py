"""GPU checks of iRDQN on the compact obs record and of its carried acting state (csrc/rdqn_kernels.hip through
d2dhip/rdqn.py): neither changes any result, so everything here is bit-equality with the fp32 ring / the window's
recompute of the same build -- Q-values, maxima, actions, all ten gradients, the loss, and a whole learner run.  One
case also pins the record path to the float64 oracle (tests/irdqn_oracle.py) under the band rules of
tests/test_irdqn_gpu.py, and one to the reference's recorded updates under that file's own bounds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_irdqn_gpu import (check_grads, dev, fixture_learner, make_params, masks_to_idx, ref_q, ref_td,  # noqa: E402
                            td_inputs)
from test_irdqn_record_cpu import random_record  # noqa: E402

# F, H, A: IT = 1 .. 4; the bias byte F as the last byte of a row (31), just past the last word read (32), inside the
# last word read (5, 30, 46) and the last byte of a two-chunk row (63)
SHAPES = [(5, 16, 2), (12, 16, 4), (30, 100, 8), (31, 16, 2), (32, 16, 2), (46, 128, 16), (63, 16, 2)]
N, E = 3, 2
NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w1", "b1", "w2", "b2", "w3", "b3")


def rings(rows, F, seed):
    """A record ring with random garbage from byte F on, and the fp32 ring it decodes to (both on the device)."""
    from d2dhip.record import ObsRecord
    rec, _ = random_record((rows, E), N, F, seed, garbage=True)
    rec = ObsRecord(rec.data.cuda(), F, rec.signed.cuda())
    ring32 = rec.decode().contiguous()
    assert ring32.shape == (rows, E, N, F) and ring32.min() < 0 and ring32.max() == 255
    return rec, ring32


def masks(act, A):
    from d2dhip import rdqn
    return (torch.ones_like(act) << act).to(rdqn.mask_dtype(A)).cuda()


def both(fn, rec, ring32):
    """fn(ring) on the record and on the fp32 ring; asserts every tensor of the two results bit-equal."""
    got, want = fn(rec), fn(ring32)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(got, want)):
        if isinstance(x, dict):
            for n in NAMES:
                assert torch.equal(x[n], y[n]), (i, n)
        else:
            assert x.dtype == y.dtype and torch.equal(x, y), i
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"F{s[0]}-H{s[1]}-A{s[2]}")
def test_record_equals_fp32_bitwise(shape):
    from d2dhip import rdqn
    F, H, A = shape
    p, _ = make_params(F, H, A, seed=H + F)
    pd = dev(p)
    Lq, rows = 16, 16 + 7
    rec, ring32 = rings(rows, F, seed=F)
    rng = np.random.default_rng(F)
    for B in (1, 17, 33):
        # q: window lengths 1 .. L mixed in one tile, some windows wrapping the plain ring
        lens = [int(rng.integers(1, Lq + 1)) for _ in range(B)]
        lens[0], lens[-1] = Lq, 1 if B > 1 else Lq
        s = torch.tensor([(int(rng.integers(E)), int(rng.integers(rows)), S) for S in lens], dtype=torch.int32).cuda()
        q, qmax, act = both(lambda r: rdqn.q_values(pd, r, s), rec, ring32)
        assert q.shape == (N, B, A) and torch.isfinite(q).all()
        act_i, reward, done, qt = td_inputs(B, A, seed=B)
        for L in (1, 5, 16):
            sg = torch.tensor([(int(rng.integers(E)), int(rng.integers(rows)), L) for _ in range(B)],
                              dtype=torch.int32).cuda()
            for loss in ("huber", "mse"):
                g, ls = both(lambda r: rdqn.grads(pd, r, sg, L, masks(act_i, A), reward.cuda(), done.cuda(), qt.cuda(),
                                                  0.4, loss), rec, ring32)
                assert torch.isfinite(ls).all() and g["w_ih"].abs().max() > 0
    # a ring of whole episodes: transitions as indices, row_shift 0 (states) and 1 (successor states)
    T, n_ep, L, B = 6, 3, 5, 17
    rec, ring32 = rings(n_ep * (T + 1), F, seed=F + 1)
    lasts = [4, 7, 9, 17, 2, 0] + [int(rng.integers(n_ep * T)) for _ in range(B - 6)]
    s = torch.tensor([(b % E, last, L) for b, last in enumerate(lasts)], dtype=torch.int32).cuda()
    for shift in (0, 1):
        both(lambda r: rdqn.q_values(pd, r, s, ring_episode=T, row_shift=shift), rec, ring32)
    act_i, reward, done, qt = td_inputs(B, A, seed=3)
    for loss in ("huber", "mse"):
        both(lambda r: rdqn.grads(pd, r, s, L, masks(act_i, A), reward.cuda(), done.cuda(), qt.cuda(), 0.4, loss,
                                  ring_episode=T), rec, ring32)


def test_record_matches_float64():
    """The record path against the float64 oracle, under the band rules of tests/test_irdqn_gpu.py (Q: 1e-5 absolute or
    twice torch fp32's own distance; gradients: 2e-5 max|g|, or 4x torch fp32's distance where that is outside it).
    Inputs are the observations' own kind -- packet counts, channel bits, ACKs -- on the int8 / uint8 columns."""
    from d2dhip import rdqn
    from d2dhip.record import ObsRecord, encode
    F, H, A, L, B, rows = 30, 100, 8, 5, 33, 12
    p, dims = make_params(F, H, A, seed=5)
    rec, neg = random_record((rows, E), N, F, seed=9)                    # for its masks: neg [N][F], the int8 columns
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, 8, (rows, E, N, F), generator=g).float()
    x = torch.where(neg, torch.randint(-1, 2, x.shape, generator=g).float(), x)
    for k, d in enumerate(dims):
        x[:, :, k, d:] = 0
    rec = encode(x, rec.signed)
    assert torch.equal(rec.decode(), x) and x.min() == -1
    rec = ObsRecord(rec.data.cuda(), F, rec.signed.cuda())
    rng = np.random.default_rng(1)
    samples = [(int(rng.integers(E)), int(rng.integers(rows)), (1, 2, L)[b % 3]) for b in range(B)]
    q64, q32 = ref_q(p, x, samples, torch.float64), ref_q(p, x, samples, torch.float32)
    q = rdqn.q_values(dev(p), rec, torch.tensor(samples, dtype=torch.int32).cuda())[0]
    err = (q.cpu().double() - q64).abs()
    tol = torch.clamp(2 * (q32.double() - q64).abs(), min=1e-5)
    print(f"  max |kernel - f64| {err.max().item():.2e}  max |torch f32 - f64| {(q32.double() - q64).abs().max().item():.2e}")
    assert torch.all(err <= tol), (err - tol).max().item()
    samples = [(e, last, L) for e, last, _ in samples]
    act, reward, done, qt = td_inputs(B, A, seed=B)
    r64, l64, _ = ref_td(p, x, samples, L, act, reward, done, qt, 0.4, "huber", torch.float64)
    r32, _, _ = ref_td(p, x, samples, L, act, reward, done, qt, 0.4, "huber", torch.float32)
    got, ls = rdqn.grads(dev(p), rec, torch.tensor(samples, dtype=torch.int32).cuda(), L, masks(act, A), reward.cuda(),
                         done.cuda(), qt.cuda(), 0.4, "huber")
    torch.cuda.synchronize()
    check_grads(got, ls, r64, l64, r32, p)
    for k, d in enumerate(dims):
        assert torch.all(got["w_ih"][k, :, d:] == 0)


def walk(pd, ring, B, carry, slots, bump_before=None, L=5):
    """The acting loop over `slots` (slot t: row t, window min(t + 1, L)) with epsilon-greedy draws; bump_before: the
    slot before which a weight is written in place.  Returns the per-slot (q, qmax, action index)."""
    from d2dhip import rdqn
    s = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
    s[:, 0] = torch.arange(B, dtype=torch.int32, device="cuda") % E
    out = []
    for t in slots:
        if t == bump_before:
            pd["w_hh"][1, 2, 3] += 0.25
            pd["b_ih"].mul_(1.5)
        S = min(t + 1, L)
        s[:, 1], s[:, 2] = t, S
        kw = dict(carry=carry, row=t, window=S) if carry is not None else {}
        q, qmax, act = rdqn.q_values(pd, ring, s, mode="eps", eps=0.5, seed=7, rng_step=t, **kw)
        out.append((q.clone(), qmax.clone(), masks_to_idx(act)))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fmt", ["f32", "record"])
@pytest.mark.parametrize("case", [(5, 16, 2, 17), (30, 100, 8, 33), (46, 128, 16, 1)],
                         ids=lambda c: f"F{c[0]}-H{c[1]}-A{c[2]}-B{c[3]}")
def test_carry_equals_recompute_bitwise(case, fmt):
    """An episode of T = 8 slots at history_len 5: slots 1 .. 4 extend the previous window (carried), slots 5 .. 7 slide
    (the wrapper recomputes).  Then the same with a weight written between slots 2 and 3 and slot 5 skipped: the tag
    drops the carry, so no launch ever runs on a stale state."""
    from d2dhip import rdqn
    F, H, A, B = case
    p, _ = make_params(F, H, A, seed=F)
    rec, ring32 = rings(9, F, seed=H)
    ring = rec if fmt == "record" else ring32
    st = rdqn.CarryState()
    got, want = walk(dev(p), ring, B, st, range(8)), walk(dev(p), ring, B, None, range(8))
    assert (st.carried, st.recomputed) == (4, 4)
    assert st.h.numel() == N * 16 * -(-B // 16) * 16 * -(-H // 16)
    for t, (x, y) in enumerate(zip(got, want)):
        for a, b in zip(x, y):
            assert torch.equal(a, b), t
    acts = torch.stack([x[2] for x in got])
    assert (acts <= 1).any() and acts.shape == (8, B, N)                 # the epsilon draws took part
    slots = [0, 1, 2, 3, 4, 6, 7]
    st = rdqn.CarryState()
    got, want = walk(dev(p), ring, B, st, slots, bump_before=3), walk(dev(p), ring, B, None, slots, bump_before=3)
    assert (st.carried, st.recomputed) == (3, 4)                          # slots 1, 2 and 4 carried
    for t, (x, y) in zip(slots, zip(got, want)):
        for a, b in zip(x, y):
            assert torch.equal(a, b), t
    assert not torch.equal(got[3][0], walk(dev(p), ring, B, None, [3])[0][0])   # the write changed slot 3's Q-values


# ------------------------------------------------------------------------------------------------ the learner
def run_learner(E_, record, carry):
    from algorithms.irdqn import iRDQN
    from envs.combinatorial_env import CombinatorialEnv
    torch.manual_seed(0)
    np.random.seed(5)
    env = CombinatorialEnv(2, 2, np.array([3, 5]), np.ones(2) * 0.7, episode_length=6, n_envs=E_, device="cuda:0",
                           seed=3)                                          # deadlines differ: obs widths 7 and 9
    ln = iRDQN(env, history_len=3, replay_start_size=2, replay_buffer_size=10 ** 4, gamma=0.4,
               update_target_frequency=2, minibatch_size=8, learning_rate=1e-3, replay_record=record)
    ln.carry_state = carry
    assert ln.network.in_dims == [7, 9] and ln.replay_record is record
    scores = ln.train(6, early_stopping=False)
    tests = ln.test(2)
    torch.cuda.synchronize()
    return ln, scores, tests


@pytest.mark.parametrize("E_", [1, 4])
def test_learner_is_bit_equal_on_all_four_paths(E_):
    from d2dhip import _lib
    from d2dhip.record import ObsRecord
    base, scores0, tests0 = run_learner(E_, False, False)
    assert base.n_updates == 4 and not isinstance(base._ring, ObsRecord) and not base._carries
    for record, carry in ((False, True), (True, False), (True, True)):
        ln, scores, tests = run_learner(E_, record, carry)
        assert scores == scores0 and tests == tests0, (record, carry)
        assert torch.equal(torch.stack(ln.losses), torch.stack(base.losses))
        for net, net0 in ((ln.network, base.network), (ln.target_network, base.target_network)):
            for n in NAMES:
                assert torch.equal(net.params[n], net0.params[n]), (record, carry, n)
        assert torch.equal(ln._act_ring, base._act_ring) and torch.equal(ln._rew_ring, base._rew_ring)
        if carry:                                                         # prefix slots 1, 2 of every episode carried
            states = ln._carries.values()
            assert sum(s.carried for s in states) > 0
            assert all(s.carried * 2 == s.recomputed for s in states)     # T = 6, L = 3: 2 carried, 4 recomputed
        if record:
            F = base._ring.shape[-1]
            RB = _lib.record_bytes(F)
            assert isinstance(ln._ring, ObsRecord) and F == 9 and RB == 32
            assert torch.equal(ln._ring.decode(), base._ring)
            assert ln._ring.data.numel() * 4 * F == base._ring.numel() * 4 * RB
        else:
            assert torch.equal(ln._ring, base._ring)


# ------------------------------------------------------------------------- the reference's recorded runs
@pytest.mark.parametrize("loss", ["huber", "mse"])
def test_reference_first_update_on_the_record_ring(loss):
    """The recorded episodes of tests/golden/irdqn_common.npz in a record ring (record.encode): the first recorded
    update's losses and gradients are bit-equal to the fp32-ring learner's, and within test_reference_updates' own
    bounds of the reference's."""
    from d2dhip.record import ObsRecord, encode
    seen = {}
    for record in (False, True):
        ln, zc, z, cfg, O = fixture_learner(loss)
        ln.replay_record = record
        b = ln._bind_env()
        obs = torch.from_numpy(zc["buffer/obs"])                         # [episodes][T + 1][N][F]
        n_ep, T = obs.shape[0], obs.shape[1] - 1
        acts, rews = zc["buffer/actions"], zc["buffer/rewards"]
        ln._alloc_ring(b, n_ep)
        assert isinstance(ln._ring, ObsRecord) is record
        for ep in range(n_ep):
            slot = (ln._added // T) % ln._ring_ep
            rows = slice(slot * (T + 1), (slot + 1) * (T + 1))
            if record:
                ln._ring.data[rows, 0] = encode(obs[ep].cuda(), ln._ring.signed).data
            else:
                ln._ring[rows, 0] = obs[ep].cuda()
            ln._act_ring[slot * T:(slot + 1) * T, 0] = torch.from_numpy(1 << acts[ep * T:(ep + 1) * T]).to(torch.uint8).cuda()
            ln._rew_ring[slot * T:(slot + 1) * T, 0] = torch.from_numpy(rews[ep * T:(ep + 1) * T, 0]).int().cuda()
            ln._added += T
        grads_seen = []
        step = ln.optimizer.step
        ln.optimizer.step = lambda: (grads_seen.append({k: v.grad.clone() for k, v in ln.network.params.items()}),
                                     step())[1]
        ln._sample_chunks = lambda n_envs, length, B, L: (np.zeros(B, dtype=np.int64), z["upd/0/starts"])
        ln._update(1)
        torch.cuda.synchronize()
        seen[record] = (ln.losses[0].clone(), grads_seen[0], ln._ring)
    (l32, g32, ring32), (lrec, grec, rec) = seen[False], seen[True]
    assert torch.equal(rec.decode(), ring32) and torch.equal(lrec, l32)
    for k in NAMES:
        assert torch.equal(grec[k], g32[k]), k
    s64, _ = O.trajectory(zc, z, cfg, loss)
    s32, _ = O.trajectory(zc, z, cfg, loss, torch.float32)
    for i in range(ln.n_agents):
        want = float(z[f"upd/0/agent{i}/loss"])
        assert abs(lrec[i].item() - want) <= 1e-5 * abs(want)
    for k, sd in O.SD_NAMES.items():
        got = grec[k].cpu().double()
        ref = s64[0]["grads"][k]
        assert np.abs(ref[0].numpy() - z[f"upd/0/agent0/grad/{sd}"]).max() <= 1e-9 * np.abs(ref[0].numpy()).max()
        scale = ref.abs().max().item()
        err64 = (got - ref).abs().max().item()
        band = (s32[0]["grads"][k].double() - ref).abs().max().item()
        print(f"  {k}: max|g| {scale:.3e}  |kernel-ref| {err64:.2e}  |torchf32-ref| {band:.2e}")
        tol = 2e-5 * scale + 1e-7
        assert err64 <= (tol if band <= tol else 4 * band), (k, err64, tol, band)
