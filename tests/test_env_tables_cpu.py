"""Host side of the record-only step of the combinatorial env (csrc/env_kernels.hip, comb_record_only /
kRecTables: 33-64 agents, C <= 8, a step that writes the record and the reward at most and replays nothing; the
workgroup stages the per-agent tables in LDS).  No GPU:

1. d2d_env_step_lds_bytes, the dynamic LDS of the kernel a step would launch: the table image
   (1536 + 1024 * ceil(C / 4) bytes, independent of N in 33..64 and of packed / unpacked) for the record-only step,
   and what the other kernels carved before for every call outside the selection rule;
2. the step's argument refusals are what they were (the query runs the same checks);
3. the parameters of tests/test_env_tables_gpu.py (tables_params) on the C oracle: byte cells and 16-bit counters
   are never at their limits, so every GPU batch of that file stays packed and no cell saturates.
"""
import ctypes

import numpy as np
import pytest

SWITCH = np.array([0.0, 1.0, 0.3, 1e-9, 0.999999999])  # thresholds 0, 2^32, and the neighbours of both
L = 12


def tables_params(N, C, deadlines, homogeneous=True, traffic="heterogeneous"):
    """channel_switch cycles over SWITCH per (agent, channel), lbdas over {0.5, 6, 20} (at 6 and 20 most Poisson
    draws pass the four staged CDF entries), arrival_probs over {0.2, 0, 1} (arrival thresholds 0 and 2^32)."""
    k, c = np.arange(N)[:, None], np.arange(C)[None, :]
    return dict(n_agents=N, n_channels=C, deadlines=np.resize(np.asarray(deadlines), N),
                lbdas=np.resize(np.array([0.5, 6.0, 20.0]), N), period=np.full(N, 2),
                arrival_probs=np.resize(np.array([0.2, 0.0, 1.0]), N), offsets=np.zeros(N), episode_length=L,
                traffic_model=traffic, homogeneous_size=homogeneous,
                periodic_devices=[i for i in range(N) if i % 4 == 0], channel_switch=SWITCH[(3 * k + c) % len(SWITCH)])


def _desc(N, C, D, kind=0):
    from d2dhip import _lib
    w = ctypes.c_void_p(16)
    kinds, period, offs = np.zeros(1024, np.uint8), np.ones(1024), np.zeros(1024)
    F = D + 2 * C if kind == 0 else D + C + 1
    d = _lib.EnvDesc(kind, N, C, D, F, 104, 104, 5, 0, 0, w, w, kinds.ctypes.data, period.ctypes.data,
                     offs.ctypes.data, None, None, w)
    return d, (kinds, period, offs)  # the host tables are kept alive by the caller


def _lds(lib, d, out=None, replay=None, packed=0):
    ref = ctypes.byref
    return lib.d2d_env_step_lds_bytes(ref(d), None if replay is None else ref(replay), None if out is None else ref(out),
                                      packed)


@pytest.mark.parametrize("N", [33, 64])
@pytest.mark.parametrize("C", [1, 5, 8])
def test_lds_bytes_of_the_record_only_step(N, C):
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    w = 16
    d, _keep = _desc(N, C, 14)
    image = 1536 + 1024 * ((C + 3) // 4)  # misc + always words, the arrival element, 16 B per four thresholds
    rec = _lib.EnvOut(None, None, w, None, None, w)      # reward + record
    for packed in (0, 1):
        assert _lds(lib, d, rec, packed=packed) == image
        assert _lds(lib, d, None, packed=packed) == image  # no output at all is record-only too
    # every output or replay input outside the rule keeps the earlier kernels and their carve
    slot = (64 * d.obs_dim + 3) & ~3
    assert _lds(lib, d, _lib.EnvOut(None, None, w, w, None, w)) == 0           # ack
    assert _lds(lib, d, _lib.EnvOut(None, None, w, None, w, w)) == 0           # success
    assert _lds(lib, d, rec, replay=_lib.EnvReplay(w, None)) == 0              # replayed flips
    assert _lds(lib, d, rec, replay=_lib.EnvReplay(None, w)) == 0              # replayed arrivals
    assert _lds(lib, d, _lib.EnvOut(w, None, w, None, None, None)) == 4 * 8 * slot            # fp32 obs, 512 lanes
    assert _lds(lib, d, _lib.EnvOut(None, w, w, None, None, w)) == 4 * 8 * (slot + 104)        # state
    assert _lds(lib, d, _lib.EnvOut(None, None, w, None, None, w, w, 104)) == 4 * 8 * (slot + 104)  # bf16 state


def test_lds_bytes_outside_the_agent_and_channel_range():
    """N <= 32 (several envs per wave), N > 64 (one env per workgroup) and C > 8 (uint16 masks) are not record-only
    steps: no table image."""
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    rec = _lib.EnvOut(None, None, 16, None, None, 16)
    for N, C in ((32, 8), (16, 4), (9, 8)):
        d, _keep = _desc(N, C, 14)
        assert _lds(lib, d, rec) == 0 and _lds(lib, d, rec, packed=1) == 0
    d, _keep = _desc(65, 8, 14)
    assert _lds(lib, d, rec) == 4 * 80            # the LARGE path's channel counters
    d, _keep = _desc(64, 16, 14)
    assert _lds(lib, d, rec) == 0
    d, _keep = _desc(64, 3, 7, kind=1)            # channel selection: its own carve
    assert _lds(lib, d, None) == 4 * ((8 * 34 + 3) & ~3)  # 8 envs per 512-lane workgroup


def test_refusals_are_unchanged():
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    ref = ctypes.byref
    w = ctypes.c_void_p(16)
    assert lib.d2d_env_step_lds_bytes(None, None, None, 0) == -1 and b"desc" in lib.d2d_last_error()
    ok, _keep = _desc(64, 8, 14)
    pst = _lib.EnvPackedState(w, w)
    ust = _lib.EnvState(w, w, w, w, None, None)
    # the steps themselves: NULL actions, NULL state, a misaligned record, before any HIP call
    assert lib.d2d_env_step_packed(ref(ok), ref(pst), None, None, None, 1, 0, None) == -1
    assert b"actions" in lib.d2d_last_error()
    assert lib.d2d_env_step(ref(ok), ref(ust), None, None, None, 1, 0, None) == -1 and b"actions" in lib.d2d_last_error()
    assert lib.d2d_env_step_packed(ref(ok), None, w, None, None, 1, 0, None) == -1
    assert b"packed state" in lib.d2d_last_error()
    assert lib.d2d_env_step(ref(ok), None, w, None, None, 1, 0, None) == -1 and b"state buffers" in lib.d2d_last_error()
    bad_rec = _lib.EnvOut(None, None, None, None, None, 24)
    for rc in (lib.d2d_env_step_packed(ref(ok), ref(pst), w, None, ref(bad_rec), 1, 0, None),
               lib.d2d_env_step(ref(ok), ref(ust), w, None, ref(bad_rec), 1, 0, None), _lds(lib, ok, bad_rec)):
        assert rc == -1 and b"aligned" in lib.d2d_last_error()
    # packed eligibility (a full row, C > 8), for the step and the query alike
    for d, word in ((_desc(64, 8, 8)[0], b"max_deadline"), (_desc(64, 8, 16)[0], b"max_deadline"),
                    (_desc(64, 16, 14)[0], b"n_channels")):
        assert lib.d2d_env_step_packed(ref(d), ref(pst), w, None, None, 1, 0, None) == -2
        assert word in lib.d2d_last_error()
        assert _lds(lib, d, None, packed=1) == -2 and word in lib.d2d_last_error()
    big, _keep2 = _desc(2000, 8, 7)
    assert lib.d2d_env_step(ref(big), ref(ust), w, None, None, 1, 0, None) == -2 and _lds(lib, big) == -2
    assert lib.d2d_abi_version() == 15


@pytest.mark.parametrize("traffic", ["heterogeneous", "aperiodic"])
def test_control_run_stays_inside_byte_cells_and_16_bit_counters(traffic):
    """The parameters of the GPU file on the C oracle, two 12-slot episodes at N = 50, C = 5, E = 5: no buffer cell
    near 255 and no counter near 65,536 (so the packed batches stay packed), Poisson draws beyond the four staged
    CDF entries do occur, and so do slots with flips forced by threshold 2^32."""
    from oracle.c_oracle import COracle
    p = tables_params(50, 5, [7, 14], True, traffic)
    c = COracle("comb", p, n_envs=5, seed=21)
    top = 0
    step = 0
    for _ep in range(2):
        c.reset(rng_step=step)
        step += 1
        for _t in range(L):
            ac = c.sample_actions(step, p=0.3)
            before = c.chan.copy()
            c.step(ac, rng_step=step + 1)
            step += 2
            top = max(top, int(c.buf.max()))
            flipped = before != c.chan
            sw = np.broadcast_to(p["channel_switch"], flipped.shape)
            assert flipped[sw == 1.0].all() and not flipped[sw == 0.0].any()
            assert int(c.buf.max()) < 128 and int(c.recv.max()) < 4096 and int(c.disc.max()) < 4096
    assert top >= 8  # a draw of at least 4 passed the staged head, many times over at lambda = 20
