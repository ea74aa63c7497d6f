"""The packed per-agent state of the combinatorial env (d2d_env_packed_state: the channel mask in the top byte of
the last buffer-row word, received | discarded << 16 in one counter word) against the unpacked
state and kernels of the same build (EnvBatch(packed=False)) and against the C oracle.  Every value is an
integer: all comparisons are exact.

1. packed == unpacked over two 12-slot episodes, every output combination in turn, on the eligible shapes (ragged
   last block, ragged wave, DW = 1, one env per workgroup), reading the state every slot (unpack each slot) and
   only at the end (a pure packed run); ineligible shapes fall back and still match the C oracle;
2. packed == C oracle in Philox mode without reading the state until each episode's end;
3. the counter bound: the switch to the unpacked kernels happens before a 16-bit counter would wrap, and the next
   reset returns to the packed path;
4. one fused env + policy slot after packed steps (unpack, native call, pack);
5. a captured graph of reset + 3 steps + a `received.sum(1)` read, replayed twice.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    import d2dhip
    d2dhip.require_gpu()


def _params(N, C, deadlines, L=12):
    return dict(n_agents=N, n_channels=C, deadlines=np.asarray(deadlines), lbdas=np.full(N, 0.5), period=np.full(N, 2),
                arrival_probs=np.resize(np.array([.2, .6, 1.]), N), offsets=np.zeros(N), episode_length=L,
                traffic_model="heterogeneous", homogeneous_size=True,
                periodic_devices=[k for k in range(N) if k % 3 == 0], channel_switch=np.full((N, C), 0.3))


def _pair(params, E, seed):
    """The same env twice: the default batch (packed where eligible) and the unpacked comparison batch."""
    from d2dhip.envbatch import EnvBatch
    from envs.combinatorial_env import CombinatorialEnv
    env = CombinatorialEnv(**params, n_envs=E, device="cuda:0", seed=seed)
    bp = env.batch()
    bu = EnvBatch(bp.spec, E, bp.device, seed=seed, env_base=0, packed=False)
    assert not bu.packed and not bu.packed_now
    return bp, bu


def _state(b):
    return [t.clone() for t in (b.buffers, b.channels, b.received, b.discarded)]


def _same_state(bp, bu, where):
    for x, y, name in zip(_state(bp), _state(bu), ("buffers", "channels", "received", "discarded")):
        assert torch.equal(x, y), (name, where)


# output combinations, taken in turn: (uses the record, kwargs of step)
_COMBOS = [
    (True, dict()),                                              # the record alone (the benchmark's step)
    (False, dict(want_obs=True)),                                # fp32 obs rows
    (False, dict(want_obs=True, want_state=True)),               # + the fp32 state
    (True, dict(bf16=True)),                                     # record + bf16 state
    (False, dict(want_obs=True, want_ack=True, want_success=True)),
    (True, dict(want_state=True, want_ack=True, want_success=True)),
]


def _run_both(bp, bu, every_slot, episodes=2, L=12):
    s, E = bp.spec, bp.E
    ld8 = -(-s.S // 8) * 8
    recs = [b.record_buffer(()) for b in (bp, bu)]
    sb = [torch.zeros((E, ld8), dtype=torch.bfloat16, device=bp.device) for _ in range(2)]
    rews = [torch.zeros(E, dtype=torch.int32, device=bp.device) for _ in range(2)]
    for ep in range(episodes):
        outs = []
        bu.rng_step = bp.rng_step
        for j, b in enumerate((bp, bu)):
            if ep == 0:
                outs.append(b.reset(want_obs=True, want_state=True, out_state_bf16=sb[j]))
            else:
                r = b.reset(want_obs=True, out_obs=recs[j])
                outs.append(dict(obs=r["obs"].data))
        for k in outs[0]:
            if outs[0][k] is not None:
                assert torch.equal(outs[0][k], outs[1][k]), ("reset", ep, k)
        assert torch.equal(sb[0], sb[1])
        if every_slot:
            _same_state(bp, bu, ("reset", ep))
        for t in range(L):
            use_rec, kw = _COMBOS[t % len(_COMBOS)]
            a = bp.sample_actions(0.3)
            res = []
            bu.rng_step = bp.rng_step
            for j, b in enumerate((bp, bu)):
                kw_j = {k: v for k, v in kw.items() if k != "bf16"}
                if use_rec:
                    kw_j["out_obs"] = recs[j]
                if kw.get("bf16"):
                    kw_j["out_state_bf16"] = sb[j]
                res.append(b.step(a, out_reward=rews[j], **kw_j))
            for k in ("obs", "state", "reward", "ack", "success"):
                x, y = res[0][k], res[1][k]
                if x is None:
                    assert y is None
                    continue
                x, y = (x.data, y.data) if use_rec and k == "obs" else (x, y)
                assert torch.equal(x, y), (ep, t, k)
            assert torch.equal(sb[0], sb[1]), (ep, t, "state_bf16")
            assert res[0]["done"] == res[1]["done"]
            if every_slot:
                _same_state(bp, bu, (ep, t))
    _same_state(bp, bu, "end")


@pytest.mark.parametrize("every_slot", [True, False], ids=["unpack-every-slot", "pure-packed"])
@pytest.mark.parametrize("N,C,deadlines,E", [
    (64, 8, [7, 14] * 32, 5),     # the benchmark's shape; 4 envs per 256-lane block: a ragged last block
    (8, 8, [7] * 8, 13),          # eight envs per wave, ragged wave
    (3, 4, [3] * 3, 7),           # DW = 1: the mask in the top byte of the only word
    (128, 8, [14] * 128, 3),      # one env per workgroup
], ids=["64x8", "8x8", "3x4", "128x8"])
def test_packed_equals_unpacked(N, C, deadlines, E, every_slot):
    bp, bu = _pair(_params(N, C, deadlines), E, seed=31)
    assert bp.packed and bp.packed_now
    _run_both(bp, bu, every_slot)
    assert bp.packed_now


def _oracle_case(params, E, steps, seed, want_packed, read_every_slot, episodes=2, p_act=0.25):
    """tests/test_env_gpu.py::_philox_case, with the state read every slot or only at each episode's end."""
    from d2dhip.envbatch import pack_masks
    from envs.combinatorial_env import CombinatorialEnv
    from oracle.c_oracle import COracle
    env = CombinatorialEnv(**params, n_envs=E, device="cuda", seed=seed)
    b = env.batch()
    s = b.spec
    assert b.packed == want_packed
    c = COracle("comb", params, n_envs=E, seed=seed)

    def same_state(where):
        assert np.array_equal(b.buffers_host(), c.buf), where
        assert np.array_equal(b.channels_host(), c.chan), where
        assert np.array_equal(b.received.cpu().numpy().astype(np.uint32), c.recv), where
        assert np.array_equal(b.discarded.cpu().numpy().astype(np.uint32), c.disc), where

    for ep in range(episodes):
        r = env.reset_batched(want_obs=True, want_state=True)
        rc = c.reset(rng_step=b.rng_step - 1)
        assert np.array_equal(r["obs"].cpu().numpy(), rc["obs"])
        assert np.array_equal(r["state"].cpu().numpy()[:, : s.S], rc["state"])
        for t in range(steps):
            rs = b.rng_step
            a = b.sample_actions(p_act)
            ac = c.sample_actions(rs, p=p_act)
            assert np.array_equal(a.cpu().numpy(), pack_masks(ac, s.C)), (ep, t)
            rs = b.rng_step
            out = env.step_batched(a, want_obs=True, want_state=True, want_ack=True, want_success=True)
            oc = c.step(ac, rng_step=rs)
            assert np.array_equal(out["obs"].cpu().numpy(), oc["obs"]), (ep, t)
            assert np.array_equal(out["state"].cpu().numpy()[:, : s.S], oc["state"]), (ep, t)
            assert np.array_equal(out["reward"].cpu().numpy(), oc["reward"]), (ep, t)
            assert np.array_equal(out["ack"].cpu().numpy().astype(np.float64), oc["ack"]), (ep, t)
            assert np.array_equal(out["success"].cpu().numpy(), oc["success"]), (ep, t)
            if read_every_slot:
                same_state((ep, t))
        same_state((ep, "end"))
    assert b.packed_now == want_packed


@pytest.mark.parametrize("N,C,D", [(6, 8, 8), (6, 8, 16), (6, 16, 14)], ids=["D8-full-row", "D16-full-row", "C16"])
def test_ineligible_shapes_fall_back_and_match_c_oracle(N, C, D):
    """A full row (D = 8, 16 with C = 8) has no room for the mask, and C > 8 was left unpacked: today's path."""
    params = dict(n_agents=N, n_channels=C, deadlines=np.array([D, max(1, D // 2)] * (N // 2)), lbdas=np.full(N, 0.3),
                  episode_length=8, traffic_model="aperiodic", channel_switch=np.full((N, C), 0.4))
    _oracle_case(params, E=33, steps=8, seed=7, want_packed=False, read_every_slot=True)


@pytest.mark.parametrize("name", ["comb_64x8_tiled", "comb_4x3_periodic", "comb_1x1_heavy"])
def test_packed_philox_matches_c_oracle(name):
    z = np.load(os.path.join(GOLDEN, f"env_{name}.npz"))
    params = load_params(z)
    params["episode_length"] = 15
    _oracle_case(params, E=257, steps=15, seed=20261015, want_packed=True, read_every_slot=False)


def test_counter_bound_switches_to_unpacked_before_a_wrap():
    """received <= (steps since reset + 1) * 255 with replayed arrivals of 255: slot 256 reaches 65,535 exactly and
    still runs packed, slot 257 must run unpacked; the next reset returns to the packed path."""
    N, C, E = 2, 2, 3
    params = dict(n_agents=N, n_channels=C, deadlines=np.array([3, 3]), lbdas=np.full(N, 0.5), episode_length=300,
                  traffic_model="aperiodic", channel_switch=np.full((N, C), 0.3))
    bp, bu = _pair(params, E, seed=5)
    assert bp.packed
    dev = bp.device
    arr = torch.full((E, N), 255, dtype=torch.uint8, device=dev)
    flips = torch.zeros((E, N), dtype=torch.uint8, device=dev)
    flips[:, 0] = 1
    bu.rng_step = bp.rng_step
    for b in (bp, bu):
        b.reset(want_obs=False, replay_arrivals=arr)
    assert bp.packed_now
    for t in range(1, 261):
        a = bp.sample_actions(0.5)
        bu.rng_step = bp.rng_step
        for b in (bp, bu):
            b.step(a, want_obs=False, replay=(flips, arr))
        assert bp.packed_now == (t <= 256), t
        if t in (255, 256, 257, 260):
            assert torch.equal(bp.received, bu.received), t
            assert torch.equal(bp.discarded, bu.discarded), t
            assert torch.equal(bp.buffers, bu.buffers) and torch.equal(bp.channels, bu.channels), t
            assert int(bu.received.min()) == int(bu.received.max()) == (t + 1) * 255
    assert int(bu.received.max()) > 65535 and int(bu.discarded.max()) > 0
    bu.rng_step = bp.rng_step
    for b in (bp, bu):
        b.reset(want_obs=False)
    assert bp.packed_now
    a = bp.sample_actions(0.5)
    bu.rng_step = bp.rng_step
    for b in (bp, bu):
        b.step(a, want_obs=False)
    assert bp.packed_now
    _same_state(bp, bu, "after the reset")


def test_fused_slot_after_packed_steps():
    """step_policy_fused on a packed batch: unpack, the native call on the unpacked state, pack."""
    from d2dhip.envbatch import EnvBatch
    from d2dhip.record import set_format
    from test_fused_slot_gpu import _learner
    E = 32
    lr_a, lr_b = _learner(E, H=64), _learner(E, H=64)
    lr_b._pseed = lr_a._policy_seed()
    ba = lr_a.env.batch()
    lr_b.env._batch = EnvBatch(ba.spec, E, ba.device, seed=lr_b.env.seed, env_base=lr_b.env.env_base, packed=False)
    bb = lr_b.env.batch()
    assert ba.packed and not bb.packed and (ba.spec.N, ba.spec.C) == (64, 8)
    recs = [b.record_buffer((2,)) for b in (ba, bb)]
    N = ba.spec.N
    acts = [[b.action_buffer() for _ in range(2)] for b in (ba, bb)]
    logps = [[torch.zeros((N, E), dtype=torch.float32, device="cuda:0") for _ in range(2)] for _ in range(2)]
    rews = [torch.zeros(E, dtype=torch.int32, device="cuda:0") for _ in range(2)]
    descs = []
    for j, (lr, b) in enumerate(((lr_a, ba), (lr_b, bb))):
        b.reset(want_obs=True, out_obs=recs[j][0])
        lr._policy_slot(recs[j], 0, 0, True, acts[j][0], logps[j][0], None, None, b)
        d = lr._mlp_desc(E, b.desc.env_base, critic=False)
        d.rng_offset = b.rng_off.data_ptr()
        set_format(d, recs[j][0])
        descs.append(d)
    for t in range(4):
        cur, nxt = t % 2, (t + 1) % 2
        for j, (lr, b) in enumerate(((lr_a, ba), (lr_b, bb))):
            if t == 2:  # the fused launch, after two packed steps
                b.step_policy_fused(acts[j][cur], recs[j][nxt], rews[j], descs[j], False, acts[j][nxt], logps[j][nxt])
            else:
                b.step(acts[j][cur], want_obs=True, out_obs=recs[j][nxt], out_reward=rews[j])
                lr._policy_slot(recs[j], 0, nxt, True, acts[j][nxt], logps[j][nxt], None, None, b)
        torch.cuda.synchronize()
        assert torch.equal(recs[0][nxt].data, recs[1][nxt].data), t
        assert torch.equal(rews[0], rews[1]), t
        assert torch.equal(acts[0][nxt], acts[1][nxt]) and torch.equal(logps[0][nxt], logps[1][nxt]), t
        if t >= 2:  # (the slot after the fused one steps the re-packed state)
            _same_state(ba, bb, t)
    assert ba.packed_now and ba.rng_step == bb.rng_step and ba.timestep == bb.timestep


def test_captured_graph_of_packed_steps():
    """reset + 3 steps + the `received.sum(1)` read of the learners' rollout, captured once and replayed with two
    rng_off values, against the eager unpacked run at the same Philox counters."""
    E = 8
    bp, bu = _pair(_params(64, 8, [7, 14] * 32), E, seed=9)
    assert bp.packed
    dev = bp.device
    acts = [bp.sample_actions(0.3) for _ in range(3)]
    base = bp.rng_step

    def buffers(b):
        return dict(rec=b.record_buffer(()), rew=torch.zeros(E, dtype=torch.int32, device=dev),
                    recv=torch.zeros(E, dtype=torch.int64, device=dev), disc=torch.zeros(E, dtype=torch.int64, device=dev))

    def seq(b, o):
        b.reset(want_obs=True, out_obs=o["rec"])
        for a in acts:
            b.step(a, want_obs=True, out_obs=o["rec"], out_reward=o["rew"])
        o["recv"].copy_(b.received.sum(1))
        o["disc"].copy_(b.discarded.sum(1))

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
        assert torch.equal(op["rec"].data, ou["rec"].data), off
        assert torch.equal(op["rew"], ou["rew"]), off
        assert torch.equal(op["recv"], ou["recv"]) and torch.equal(op["disc"], ou["disc"]), off
        assert int(ou["recv"].sum()) > 0
        _same_state(bp, bu, off)  # the captured unpack refreshed the public tensors
    bp.rng_off.zero_()
