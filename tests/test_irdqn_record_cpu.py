"""Host-side checks of iRDQN on the compact obs record and of its carried acting state (csrc/rdqn_kernels.hip
d2d_rdqn_q_ex / d2d_rdqn_grad_ex / d2d_rdqn_carry_floats, d2dhip/rdqn.py CarryState, d2dhip/record.py encode) that need
no GPU: the additive ABI, the argument refusals before any HIP call, the record encoder, and the tag logic that decides
whether a launch may carry the previous launch's hidden state."""
import ctypes

import pytest

torch = pytest.importorskip("torch")


def _lib_and_desc():
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    w = ctypes.c_void_p(16)
    mk = lambda N=2, F=12, H=100, A=4, rows=14, ep=0: _lib.RdqnDesc(N, 3, F, H, A, rows, ep, 0, *([w] * 10), 0, 0, None)  # noqa
    return lib, _lib, w, mk


def test_additive_abi():
    lib, _lib, w, mk = _lib_and_desc()
    for fn in ("d2d_rdqn_q_ex", "d2d_rdqn_grad_ex", "d2d_rdqn_carry_floats"):
        assert hasattr(lib, fn) and fn in _lib.EXPORTED, fn
    assert lib.d2d_abi_version() == 15
    assert ctypes.sizeof(_lib.RdqnDesc) == 8 * 4 + 10 * 8 + 2 * 8 + 8
    for N, B, H in ((2, 17, 100), (3, 1, 16)):
        want = N * 16 * -(-B // 16) * 16 * -(-H // 16)
        assert lib.d2d_rdqn_carry_floats(ctypes.byref(mk(N=N, H=H)), B) == want
    assert lib.d2d_rdqn_carry_floats(ctypes.byref(mk(N=2, H=100)), 17) == 2 * 32 * 112
    assert lib.d2d_rdqn_carry_floats(ctypes.byref(mk(H=129)), 17) == -1
    assert lib.d2d_rdqn_carry_floats(ctypes.byref(mk()), -1) == -1
    assert lib.d2d_rdqn_carry_floats(None, 1) == -1


def test_argument_refusals_before_any_hip_call():
    lib, _lib, w, mk = _lib_and_desc()
    odd = ctypes.c_void_p(24)                                            # 8-byte aligned only
    F32, U8 = _lib.D2D_OBS_F32, _lib.D2D_OBS_U8

    def q(obs=w, fmt=F32, sgn=None, shift=0, hc=None, cin=0):
        return lib.d2d_rdqn_q_ex(ctypes.byref(mk()), obs, fmt, sgn, w, 1, shift, 0, 0.0, None, 1, None, None, 0, hc,
                                 cin, w, None, w, None)

    def g(obs=w, fmt=F32, sgn=None):
        d = mk()
        ws = lib.d2d_rdqn_grad_workspace(ctypes.byref(d), 33, 5)
        return lib.d2d_rdqn_grad_ex(ctypes.byref(d), obs, fmt, sgn, w, 33, 5, w, w, w, w, 0.4, 0, *([w] * 12), ws, None)

    err = lib.d2d_last_error
    for call in (q, g):
        assert call(fmt=7) == -1 and b"obs_format" in err()
        assert call(fmt=U8) == -1 and b"obs_signed" in err()
        assert call(obs=odd, fmt=U8, sgn=w) == -1 and b"obs record" in err() and b"aligned" in err()
    assert b"d2d_rdqn_grad" in err()                                      # the entry point is named too
    assert q(cin=1) == -1 and b"hcarry" in err() and b"carry_in" in err()
    assert q(cin=1, hc=w, shift=1) == -1 and b"row_shift" in err()
    assert q(hc=odd) == -1 and b"hcarry" in err() and b"aligned" in err()
    assert q(hc=odd, cin=1) == -1 and b"hcarry" in err()
    # the old entry points still refuse what they refused
    assert lib.d2d_rdqn_q(ctypes.byref(mk()), w, w, 1, 2, 0, 0.0, None, 1, None, None, 0, w, None, w, None) == -1
    assert lib.d2d_rdqn_q(ctypes.byref(mk(H=144)), w, w, 1, 0, 0, 0.0, None, 1, None, None, 0, w, None, w, None) == -2


def random_record(lead, N, F, seed, garbage=False):
    """(ObsRecord, signed bool [N][F]): random bytes over the full uint8 / int8 range, per-agent int8 masks that differ
    (a signed column >= 32 where F allows); garbage: random bytes after column F instead of zeros."""
    from d2dhip import _lib
    from d2dhip.record import ObsRecord
    g = torch.Generator().manual_seed(seed)
    R = _lib.record_bytes(F)
    neg = torch.rand(N, F, generator=g) < 0.4
    neg[0, 0], neg[N - 1, F - 1] = True, True                            # F - 1 >= 32 for F in {46, 63}
    neg[0, 1], neg[0, 2], neg[0, F - 1] = False, False, False
    words = torch.zeros(N, R // 32, dtype=torch.int64)
    for k in range(N):
        for c in range(F):
            if neg[k, c]:
                words[k, c // 32] |= 1 << (c % 32)
    signed = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    data = torch.randint(0, 256, tuple(lead) + (N, R), generator=g).to(torch.uint8)
    data[..., 0, 0], data[..., 0, 1], data[..., 0, 2] = 127, 255, 0      # the ends of both ranges, somewhere
    data[..., N - 1, F - 1] = 128                                        # int8 -128
    data[..., F] = 1
    if not garbage:
        data[..., F + 1:] = 0
    else:
        data[..., F] = torch.randint(2, 256, tuple(lead) + (N,), generator=g).to(torch.uint8)
    return ObsRecord(data, F, signed), neg


@pytest.mark.parametrize("F", [5, 31, 32, 63])
def test_encode_inverts_decode(F):
    from d2dhip import record
    rec, neg = random_record((4, 2), 3, F, seed=F)
    x = rec.decode()
    assert x.shape == (4, 2, 3, F) and x.dtype == torch.float32
    assert x[..., neg].min() == -128 and x[..., ~neg].max() == 255 and x[..., ~neg].min() == 0
    assert not torch.equal(rec.signed[0], rec.signed[2])                 # per-agent masks differ
    if F > 32:
        assert neg[2, F - 1] and F - 1 >= 32                              # a signed column in the second word
    enc = record.encode(x, rec.signed)
    assert torch.equal(enc.data, rec.data) and torch.equal(enc.decode(), x)
    assert torch.all(enc.data[..., F] == 1) and torch.all(enc.data[..., F + 1:] == 0)
    # into a dirty `out`
    out = record.ObsRecord(torch.full_like(rec.data, 77), F, rec.signed)
    assert record.encode(x, rec.signed, out=out) is out and torch.equal(out.data, rec.data)
    # refusals: a fraction, above uint8, below int8, above int8 on a signed column, below 0 on an unsigned one
    for k, c, v in ((1, 3, 0.5), (0, F - 1, 256.0), (0, 0, -129.0), (0, 0, 128.0),
                    (0, F - 1, -1.0)):
        bad = x.clone()
        bad[1, 1, k, c] = v
        with pytest.raises(ValueError, match="obs record holds integers"):
            record.encode(bad, rec.signed)
    with pytest.raises(ValueError, match="out must be"):
        record.encode(x[0], rec.signed, out=out)


def test_carry_state_tag_logic():
    """CarryState.advance is the whole decision (q_values launches with carry_in = its return value): it carries only
    for (row + 1, S + 1, S >= 2) on the same ring / B / samples / parameter versions."""
    from d2dhip import rdqn
    N, F, H, A, E = 2, 5, 16, 2, 3
    p = {n: torch.zeros(s) for n, s in (("w_ih", (N, 3 * H, F)), ("w_hh", (N, 3 * H, H)), ("b_ih", (N, 3 * H)),
                                        ("b_hh", (N, 3 * H)), ("w1", (N, H, H)), ("b1", (N, H)), ("w2", (N, H, H)),
                                        ("b2", (N, H)), ("w3", (N, A, H)), ("b3", (N, A)))}
    ring, other = torch.zeros(9, E, N, F), torch.zeros(9, E, N, F)
    rec, _ = random_record((9, E), N, F, seed=0)
    s, s2 = torch.zeros(E, 3, dtype=torch.int32), torch.zeros(E - 1, 3, dtype=torch.int32)
    st = rdqn.CarryState()
    st.h = torch.zeros(4)                                                # stands for the scratch q_values allocates
    adv = lambda row, S, ring_=ring, s_=s, shift=0, ep=0: st.advance(p, ring_, s_, ep, shift, row, S)  # noqa: E731
    L = 5
    got = [adv(t, min(t + 1, L)) for t in range(8)]                      # an episode: prefix windows, then sliding ones
    assert got == [False, True, True, True, True, False, False, False]
    assert (st.carried, st.recomputed) == (4, 4)
    assert adv(0, 1) is False and adv(1, 2) is True
    assert adv(3, 4) is False                                            # a skipped slot
    assert adv(4, 5) is True
    assert adv(5, 5) is False and adv(6, 5) is False                     # sliding windows: S did not grow
    assert adv(7, 6) is True                                             # one more row on the same start: an extension
    assert adv(0, 1) is False and adv(1, 2, ring_=other) is False        # another ring
    assert adv(2, 3, ring_=other) is True and adv(3, 4, ring_=rec) is False   # ... and another format
    assert adv(4, 5, ring_=rec) is True
    assert adv(0, 1) is False and adv(1, 2, s_=s2) is False              # a changed B (another samples tensor)
    assert adv(2, 3, s_=s2) is True and adv(3, 4, s_=s2.clone()) is False    # same values, not the same tensor
    assert adv(0, 1) is False and adv(1, 2) is True
    p["w2"][1, 0, 0] += 1.0                                              # an in-place parameter write
    assert adv(2, 3) is False and adv(3, 4) is True
    p["b3"] = p["b3"].clone()                                            # other storage
    assert adv(4, 5) is False
    assert adv(0, 1) is False and adv(1, 2, shift=1) is False and adv(2, 3) is False   # row_shift never carries
    assert adv(3, 4) is True and adv(4, 5, ep=6) is False                # another ring geometry
    st.reset()
    assert adv(5, 6) is False and adv(6, 7) is True
    st.h = None                                                          # no scratch yet: nothing to carry
    assert adv(7, 8) is False
    with pytest.raises(ValueError, match="row= and window="):
        st.advance(p, ring, s, 0, 0, None, 3)


def test_learner_switches():
    from algorithms.irdqn import iRDQN
    import inspect
    sig = inspect.signature(iRDQN.__init__)
    assert sig.parameters["replay_record"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["replay_record"].default is None
    assert list(sig.parameters)[-2:] == ["early_stopping", "replay_record"]
    assert isinstance(iRDQN.replay_record, bool) and isinstance(iRDQN.carry_state, bool)
    ln = iRDQN.__new__(iRDQN)
    ln.carry_state = False
    assert ln._carry(object(), "train") is None
    ln.carry_state = True
    b = object()
    assert ln._carry(b, "train") is ln._carry(b, "train") is not ln._carry(b, "test")
