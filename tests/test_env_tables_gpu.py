"""The record-only step of the combinatorial env with the per-agent tables staged in LDS (csrc/env_kernels.hip,
comb_step<..., WAVE, kRecTables>: 33-64 agents, C <= 8, a step that writes the record and the reward alone; the
workgroup builds one image of the flip thresholds, the agent entries and the head of each Poisson row behind a
single barrier) against the C oracle in Philox mode and against the unpacked batch of the same build
(EnvBatch(packed=False)).  Every value is an integer: all comparisons are exact.  Every step of this file goes into
the record alone, so every step takes the new kernel; after every slot the buffers, channels, received, discarded,
the reward and the record (decoded and as bytes) are checked.

The parameters (tests/test_env_tables_cpu.py, tables_params, where the C oracle runs them as the control):
channel_switch cycles over {0, 1, 0.3, 1e-9, 0.999999999} per (agent, channel) -- thresholds 0, 2^32 and the
neighbours of both, the cases of the 32-bit narrowing; lbdas over {0.5, 6, 20} -- past the four staged CDF
entries the lookup continues in the global table; arrival_probs over {0.2, 0, 1}.

1. ragged blocks: E in {1, 3, 4, 5, 9} at N in {33, 50, 64} (four envs per 256-lane workgroup: idle waves that
   must still reach the barrier, a ragged last workgroup);
2. C = 8, 4 and 5 (5: the runtime-C staging loop) at N = 50 and 64;
3. aperiodic, periodic (slots in which no lane draws) and heterogeneous traffic;
4. uniform and mixed obs widths, DW = 1 and DW = 8; one unpacked shape (deadline 8, a full row);
5. a captured graph of reset + 3 steps replayed with two rng_off values;
6. the selection rule: steps with want_ack, with fp32 obs and with replayed flips and arrivals (the earlier
   kernels) leave the same state as the record-only step of a twin batch.
"""
import numpy as np
import pytest

from test_env_tables_cpu import L, tables_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import d2dhip
    d2dhip.require_gpu()


def _batches(params, E, seed):
    """The default batch (packed where eligible), the unpacked batch of the same env, and the C oracle."""
    from d2dhip.envbatch import EnvBatch
    from envs.combinatorial_env import CombinatorialEnv
    from oracle.c_oracle import COracle
    env = CombinatorialEnv(**params, n_envs=E, device="cuda:0", seed=seed)
    bp = env.batch()
    bs = [bp]
    if bp.packed:
        bs.append(EnvBatch(bp.spec, E, bp.device, seed=seed, env_base=0, packed=False))
        assert not bs[1].packed
    return bs, COracle("comb", params, n_envs=E, seed=seed)


def _check_state(b, c, where):
    assert np.array_equal(b.buffers_host(), c.buf), ("buffers", where)
    assert np.array_equal(b.channels_host(), c.chan), ("channels", where)
    assert np.array_equal(b.received.cpu().numpy().astype(np.uint32), c.recv), ("received", where)
    assert np.array_equal(b.discarded.cpu().numpy().astype(np.uint32), c.disc), ("discarded", where)


def _check_record(rec, obs, where):
    from d2dhip.record import encode
    assert np.array_equal(rec.decode().cpu().numpy(), obs), ("record", where)
    want = encode(torch.from_numpy(obs), rec.signed.cpu())
    assert np.array_equal(rec.data.cpu().numpy(), want.data.numpy()), ("record bytes", where)


def _run(params, E, seed, episodes=1, p_act=0.3):
    from d2dhip.envbatch import pack_masks
    bs, c = _batches(params, E, seed)
    s = bs[0].spec
    dev = bs[0].device
    recs = [b.record_buffer(()) for b in bs]
    rews = [torch.zeros(E, dtype=torch.int32, device=dev) for _ in bs]
    for ep in range(episodes):
        rs = bs[0].rng_step
        rc = c.reset(rng_step=rs)
        for j, b in enumerate(bs):
            b.rng_step = rs
            b.reset(want_obs=True, out_obs=recs[j])
            _check_record(recs[j], rc["obs"], ("reset", ep, j))
            _check_state(b, c, ("reset", ep, j))
        for t in range(L):
            rs = bs[0].rng_step
            a = bs[0].sample_actions(p_act)
            ac = c.sample_actions(rs, p=p_act)
            assert np.array_equal(a.cpu().numpy(), pack_masks(ac, s.C)), (ep, t)
            rs = bs[0].rng_step
            oc = c.step(ac, rng_step=rs)
            for j, b in enumerate(bs):
                where = (ep, t, j)
                b.rng_step = rs
                out = b.step(a, out_obs=recs[j], out_reward=rews[j])  # the record and the reward alone
                assert out["state"] is None and out["ack"] is None and out["success"] is None
                assert np.array_equal(out["reward"].cpu().numpy(), oc["reward"]), ("reward", where)
                _check_record(out["obs"], oc["obs"], where)
                _check_state(b, c, where)
    for b in bs[:1]:
        assert b.packed_now == b.packed  # no counter came near 16 bits (the control run of the CPU file)
    return bs


@pytest.mark.parametrize("N", [33, 50, 64])
@pytest.mark.parametrize("E", [1, 3, 4, 5, 9])
def test_ragged_blocks(N, E):
    bs = _run(tables_params(N, 8, [7, 14]), E, seed=100 + N + E)
    assert len(bs) == 2 and bs[0].packed


@pytest.mark.parametrize("N", [50, 64])
@pytest.mark.parametrize("C", [8, 4, 5])
def test_threshold_edges_at_every_channel_count(N, C):
    bs = _run(tables_params(N, C, [7, 14]), 5, seed=200 + N + C, episodes=2)
    assert len(bs) == 2 and bs[0].packed


@pytest.mark.parametrize("traffic", ["aperiodic", "periodic", "heterogeneous"])
def test_traffic_models(traffic):
    """N = 50, C = 5, E = 5: the shape of the control run."""
    _run(tables_params(50, 5, [7, 14], True, traffic), 5, seed=21, episodes=2)


@pytest.mark.parametrize("N,C,deadlines,hom,packed", [
    (64, 8, [7, 14], True, True),     # uniform widths: the scalar record placement
    (50, 8, [7, 14], False, True),    # mixed widths: the per-lane placement
    (40, 8, [3], True, True),         # DW = 1
    (64, 8, [20], True, True),        # DW = 8
    (64, 8, [8], True, False),        # a full row: the unpacked record-only step
], ids=["uniform", "mixed", "dw1", "dw8", "unpacked"])
def test_widths_and_rows(N, C, deadlines, hom, packed):
    bs = _run(tables_params(N, C, deadlines, hom), 5, seed=5)
    assert bs[0].packed == packed


@pytest.mark.parametrize("N,C", [(64, 8), (50, 5)])
def test_captured_graph_adds_the_device_offset(N, C):
    """reset + 3 record-only steps captured once, replayed with two rng_off values, against the eager run of an
    unpacked batch at the same Philox counters and against the C oracle."""
    from d2dhip.envbatch import pack_masks
    E = 6
    params = tables_params(N, C, [7, 14])
    (bp, bu), c = _batches(params, E, seed=9)
    dev = bp.device
    base = bp.rng_step
    acts_c = [c.sample_actions(base + i, p=0.3) for i in range(3)]
    acts = [bp.sample_actions(0.3) for _ in range(3)]
    for a, ac in zip(acts, acts_c):
        assert np.array_equal(a.cpu().numpy(), pack_masks(ac, C))
    base = bp.rng_step

    def buffers(b):
        return dict(rec=b.record_buffer(()), rew=torch.zeros(E, dtype=torch.int32, device=dev))

    def seq(b, o):
        b.reset(want_obs=True, out_obs=o["rec"])
        for a in acts:
            b.step(a, want_obs=True, out_obs=o["rec"], out_reward=o["rew"])
        b.sync_unpacked()  # captured with the steps: a replay refreshes the public state tensors too

    op, ou = buffers(bp), buffers(bu)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        seq(bp, op)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    bp.rng_step = base
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        seq(bp, op)
    bp.rng_step = base  # capturing ran nothing
    for off in (5, 77):
        bp.rng_off.fill_(off)
        g.replay()
        torch.cuda.synchronize()
        bu.rng_step = base + off
        seq(bu, ou)
        torch.cuda.synchronize()
        c.reset(rng_step=base + off)
        for i, ac in enumerate(acts_c):
            oc = c.step(ac, rng_step=base + off + 1 + i)
        for o in (op, ou):
            _check_record(o["rec"], oc["obs"], off)
            assert np.array_equal(o["rew"].cpu().numpy(), oc["reward"]), off
        for b in (bp, bu):
            _check_state(b, c, off)
    bp.rng_off.zero_()


@pytest.mark.parametrize("N,C", [(64, 8), (50, 5)])
def test_selection_rule_old_kernels_beside_the_new_one(N, C):
    """Twin batches from one seed: `new` takes the record-only step in every slot; `old` takes, in turn, a step with
    want_ack, a step with fp32 obs, and a replayed step whose flips and arrivals are the ones the Philox step
    made (read off the oracle's state: flips = channels before ^ after, the arrival is the cell at deadline - 1).
    None of the three is record-only, so each runs an earlier kernel; the state after every slot is the same."""
    from d2dhip.envbatch import pack_masks
    from envs.combinatorial_env import CombinatorialEnv
    from oracle.c_oracle import COracle
    E = 5
    params = tables_params(N, C, [7, 14])
    new = CombinatorialEnv(**params, n_envs=E, device="cuda:0", seed=31).batch()
    old = CombinatorialEnv(**params, n_envs=E, device="cuda:0", seed=31).batch()
    c = COracle("comb", params, n_envs=E, seed=31)
    dev = new.device
    rec_new, rec_old = new.record_buffer(()), old.record_buffer(())
    rs = new.rng_step
    c.reset(rng_step=rs)
    for b, r in ((new, rec_new), (old, rec_old)):
        b.rng_step = rs
        b.reset(want_obs=True, out_obs=r)
    d_last = np.resize(np.asarray([7, 14]), N) - 1
    for t in range(L):
        rs = new.rng_step
        a = new.sample_actions(0.3)
        ac = c.sample_actions(rs, p=0.3)
        rs = new.rng_step
        chan_before = c.chan.copy()
        oc = c.step(ac, rng_step=rs)
        flips = (chan_before ^ c.chan).astype(np.uint8)
        arrivals = np.take_along_axis(c.buf, np.broadcast_to(d_last[None, :, None], (E, N, 1)), axis=2)[:, :, 0]
        old.rng_step = rs
        mode = t % 3
        if mode == 0:
            out = old.step(a, out_obs=rec_old, want_ack=True)
            assert np.array_equal(out["ack"].cpu().numpy().astype(np.float64), oc["ack"]), t
        elif mode == 1:
            out = old.step(a, want_obs=True)
            assert np.array_equal(out["obs"].cpu().numpy(), oc["obs"]), t
        else:
            rp = (torch.from_numpy(pack_masks(flips, C)).to(dev).contiguous(),
                  torch.from_numpy(np.ascontiguousarray(arrivals, dtype=np.uint8)).to(dev))
            out = old.step(a, out_obs=rec_old, replay=rp)
            _check_record(out["obs"], oc["obs"], t)
        new.rng_step = rs
        out_new = new.step(a, out_obs=rec_new)
        _check_record(out_new["obs"], oc["obs"], t)
        assert np.array_equal(out["reward"].cpu().numpy(), out_new["reward"].cpu().numpy()), t
        for name in ("buffers", "channels", "received", "discarded"):
            assert torch.equal(getattr(old, name), getattr(new, name)), (name, t)
        _check_state(new, c, t)
