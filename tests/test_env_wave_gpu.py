"""The wave-per-env step of the combinatorial env (csrc/env_kernels.hip, comb_step<..., WAVE>: 33-64 agents, one env
per wavefront, scalar channel counts / acks / addresses, Philox with a wave-uniform head, the record built from scalar
ack words) against the C oracle in Philox mode and against the unpacked kernels of the same build
(EnvBatch(packed=False)).  Every value is an integer: all comparisons are exact.

1. two 12-slot episodes on N in {33, 50, 64} (the new path) and N = 32 (the segment path, as the control), C in
   {8, 4, 5} (5: the runtime-C instantiation), deadlines all 14, all 7 and alternating [7, 14], each with
   homogeneous_size True and False (False with mixed deadlines gives non-uniform widths: the generic record
   branch): the full product of these, each shape paired with one E of {1, 3, 4, 5, 9} in turn (four envs per
   256-lane block: a ragged last block and whole idle waves; raggedness does not depend on C or the deadlines), and
   every E of that set on N in {33, 50, 64} at C = 8, deadlines [7, 14].  The output combinations
   are taken in turn (the record alone; fp32 obs; obs + state + ack + success; record + bf16 state); after every slot
   the buffers, channels, received, discarded, reward and the record (decoded and as bytes) are checked;
2. further widths and rows: byte shift 0, word shifts 0 .. 4, full rows (not packed-eligible: the unpacked wave
   step), a 64-byte record, purely periodic traffic (slots in which no lane of the wave draws an arrival);
3. replay mode: recorded flips and / or arrivals, the branches that skip one or both Philox streams;
4. a captured graph of reset + 3 steps, replayed with two rng_off values, against the same steps run eagerly.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

L = 12


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import d2dhip
    d2dhip.require_gpu()


def _params(N, C, deadlines, homogeneous=True, traffic="heterogeneous"):
    d = np.resize(np.asarray(deadlines), N)
    return dict(n_agents=N, n_channels=C, deadlines=d, lbdas=np.full(N, 0.5), period=np.full(N, 2),
                arrival_probs=np.resize(np.array([.2, .6, 1.]), N), offsets=np.zeros(N), episode_length=L,
                traffic_model=traffic, homogeneous_size=homogeneous,
                periodic_devices=[k for k in range(N) if k % 3 == 0], channel_switch=np.full((N, C), 0.3))


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


# output combinations, taken in turn: (into the record, kwargs of step, bf16 state)
_COMBOS = [
    (True, dict(), False),                                                          # the record alone
    (False, dict(want_obs=True), False),                                            # fp32 obs
    (False, dict(want_obs=True, want_state=True, want_ack=True, want_success=True), False),
    (True, dict(), True),                                                           # record + bf16 state
]


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


def _run(params, E, seed, episodes=2, replay=None, p_act=0.3):
    """replay: None (Philox), or a function slot -> (recorded flips?, recorded arrivals?)."""
    from d2dhip.envbatch import pack_masks
    bs, c = _batches(params, E, seed)
    s = bs[0].spec
    dev = bs[0].device
    ld8 = -(-s.S // 8) * 8
    recs = [b.record_buffer(()) for b in bs]
    sbs = [torch.zeros((E, ld8), dtype=torch.bfloat16, device=dev) for _ in bs]
    rews = [torch.zeros(E, dtype=torch.int32, device=dev) for _ in bs]
    rng = np.random.default_rng(seed)
    for ep in range(episodes):
        rs = bs[0].rng_step
        rc = c.reset(rng_step=rs)
        for j, b in enumerate(bs):
            b.rng_step = rs
            b.reset(want_obs=True, out_obs=recs[j])
            _check_record(recs[j], rc["obs"], ("reset", ep, j))
            _check_state(b, c, ("reset", ep, j))
        for t in range(L):
            use_rec, kw, bf16 = _COMBOS[t % len(_COMBOS)]
            rs = bs[0].rng_step
            a = bs[0].sample_actions(p_act)
            ac = c.sample_actions(rs, p=p_act)
            assert np.array_equal(a.cpu().numpy(), pack_masks(ac, s.C)), (ep, t)
            rs = bs[0].rng_step
            fl = ar = None
            if replay is not None:
                rec_f, rec_a = replay(t)
                fl = (rng.random((E, s.N, s.C)) < 0.4).astype(np.uint8) if rec_f else None
                ar = rng.integers(0, 4, size=(E, s.N)).astype(np.uint8) if rec_a else None
            oc = c.step(ac, rng_step=rs, flips=fl, arrivals=ar)
            rp = None
            if replay is not None:
                rp = (None if fl is None else torch.from_numpy(pack_masks(fl, s.C)).to(dev).contiguous(),
                      None if ar is None else torch.from_numpy(ar).to(dev))
            for j, b in enumerate(bs):
                where = (ep, t, j)
                b.rng_step = rs
                kw_j = dict(kw)
                if use_rec:
                    kw_j["out_obs"] = recs[j]
                if bf16:
                    kw_j["out_state_bf16"] = sbs[j]
                out = b.step(a, out_reward=rews[j], replay=rp, **kw_j)
                assert np.array_equal(out["reward"].cpu().numpy(), oc["reward"]), ("reward", where)
                if use_rec:
                    _check_record(out["obs"], oc["obs"], where)
                elif out["obs"] is not None:
                    assert np.array_equal(out["obs"].cpu().numpy(), oc["obs"]), ("obs", where)
                if out["state"] is not None:
                    assert np.array_equal(out["state"].cpu().numpy()[:, : s.S], oc["state"]), ("state", where)
                if out["ack"] is not None:
                    assert np.array_equal(out["ack"].cpu().numpy().astype(np.float64), oc["ack"]), ("ack", where)
                if out["success"] is not None:
                    assert np.array_equal(out["success"].cpu().numpy(), oc["success"]), ("success", where)
                if bf16:
                    got = sbs[j].float().cpu().numpy()
                    assert np.array_equal(got[:, : s.S], oc["state"]) and not got[:, s.S:].any(), ("state_bf16", where)
                assert out["done"] == oc["done"]
                _check_state(b, c, where)
    return bs


_DEADLINES = {"d14": [14], "d7": [7], "d7-14": [7, 14]}
_ES = [1, 3, 4, 5, 9]
_GRID = [(N, C, dl, hom, _ES[i % len(_ES)]) for i, (N, C, dl, hom) in enumerate(
    itertools.product([33, 50, 64, 32], [8, 4, 5], list(_DEADLINES), [True, False]))]


@pytest.mark.parametrize("N,C,dl,hom,E", _GRID, ids=[f"N{n}-C{c}-{d}-{'hom' if h else 'het'}-E{e}" for n, c, d, h, e in _GRID])
def test_wave_step_matches_c_oracle_and_unpacked(N, C, dl, hom, E):
    bs = _run(_params(N, C, _DEADLINES[dl], hom), E, seed=1000 + 7 * N + C)
    assert len(bs) == 2 and bs[0].packed_now  # every grid shape has room for the mask


@pytest.mark.parametrize("N", [33, 50, 64])
@pytest.mark.parametrize("E", _ES)
def test_every_env_count_on_the_benchmark_shape(N, E):
    """Each E of the grid on one shape (the grid pairs every shape with one E only)."""
    _run(_params(N, 8, [7, 14], True), E, seed=77, episodes=1)


@pytest.mark.parametrize("N,C,deadlines,hom,traffic,packed", [
    (40, 8, [3], True, "heterogeneous", True),        # DW = 1, word shift 0, byte shift 3
    (40, 4, [4], True, "heterogeneous", False),       # DW = 1 full row: byte shift 0, word shift 1, unpacked
    (64, 8, [8], True, "heterogeneous", False),       # DW = 2 full row: byte shift 0, word shift 2
    (64, 8, [12, 5], True, "heterogeneous", False),   # DW = 3 full row: byte shift 0, word shift 3
    (64, 8, [11, 5], True, "heterogeneous", True),    # DW = 3 with the mask byte
    (50, 4, [16, 9], True, "heterogeneous", False),   # DW = 4 full row: word shift 4
    (50, 8, [16, 9], False, "heterogeneous", False),  # F = 32: a 64-byte record, the byte-level build
    (64, 8, [20], True, "heterogeneous", True),       # DW = 8
    (64, 8, [7, 14], True, "periodic", True),         # no lane draws on odd slots: the arrival block is skipped
    (33, 5, [7, 14], False, "aperiodic", True),       # Poisson arrivals alone
], ids=["w3", "w4-full", "w8-full", "w12-full", "w11", "w16-full", "rec64", "w20", "periodic", "aperiodic"])
def test_other_widths_rows_and_traffic(N, C, deadlines, hom, traffic, packed):
    bs = _run(_params(N, C, deadlines, hom, traffic), 5, seed=5, episodes=1)
    assert bs[0].packed == packed


@pytest.mark.parametrize("N,C,hom", [(64, 8, True), (50, 5, False)])
def test_replayed_flips_and_arrivals(N, C, hom):
    """Recorded flips and arrivals, flips alone, arrivals alone, in turn: the branches without one or both streams."""
    modes = [(True, True), (True, False), (False, True)]
    _run(_params(N, C, [7, 14], hom), 5, seed=3, episodes=1, replay=lambda t: modes[(t // len(_COMBOS)) % 3])


@pytest.mark.parametrize("N,C", [(64, 8), (50, 5)])
def test_captured_graph_adds_the_device_offset(N, C):
    """reset + 3 steps captured once, replayed with two rng_off values, against the eager run of an unpacked batch
    at the same Philox counters and against the C oracle: the device offset reaches the scalar Philox head."""
    from d2dhip.envbatch import pack_masks
    E = 6
    params = _params(N, C, [7, 14], True)
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
