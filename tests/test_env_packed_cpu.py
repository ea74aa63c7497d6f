"""CPU-side checks of the packed per-agent state of the combinatorial env (d2d_env_packed_state, added on top
of ABI v15): the new entry points refuse bad arguments before any HIP call, the ctypes struct matches the
header, and the bit layout (mask in the top byte of the last row word, received | discarded << 16) is
restated in numpy against a hand-written row."""
import ctypes

import numpy as np


def _descs():
    from d2dhip import _lib
    w = ctypes.c_void_p(16)
    kinds, period, offs = np.zeros(64, np.uint8), np.ones(64), np.zeros(64)
    host = (kinds, period, offs)  # kept alive by the caller

    def comb(N, C, D, kind=0):
        F = D + 2 * C if kind == 0 else D + C + 1
        return _lib.EnvDesc(kind, N, C, D, F, 100, 100, 1, 0, 0, w, w, kinds.ctypes.data, period.ctypes.data,
                            offs.ctypes.data, None, None, w)
    return comb, w, host


def test_packed_entry_points_validate_arguments_without_gpu():
    """NULL state, ineligible shapes (D2D_EUNSUPPORTED with a message) and misaligned records are refused before
    any HIP call, so this runs on a GPU-less host."""
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    comb, w, _host = _descs()
    ok = comb(64, 8, 14)
    pst = _lib.EnvPackedState(w, w)
    ust = _lib.EnvState(w, w, w, w, None, None)
    ref = ctypes.byref
    # NULL desc
    assert lib.d2d_env_step_packed(None, None, None, None, None, 1, 0, None) == -1 and b"desc" in lib.d2d_last_error()
    assert lib.d2d_env_state_pack(None, None, None, None) == -1 and b"desc" in lib.d2d_last_error()
    # NULL state, or a NULL member
    for bad in (None, ref(_lib.EnvPackedState(None, w)), ref(_lib.EnvPackedState(w, None))):
        assert lib.d2d_env_reset_packed(ref(ok), bad, None, None, 0, None) == -1
        assert b"packed state" in lib.d2d_last_error()
        assert lib.d2d_env_step_packed(ref(ok), bad, w, None, None, 1, 0, None) == -1
        assert b"packed state" in lib.d2d_last_error()
        assert lib.d2d_env_state_pack(ref(ok), ref(ust), bad, None) == -1 and b"non-NULL" in lib.d2d_last_error()
        assert lib.d2d_env_state_unpack(ref(ok), bad, ref(ust), None) == -1 and b"non-NULL" in lib.d2d_last_error()
    assert lib.d2d_env_state_pack(ref(ok), None, ref(pst), None) == -1
    assert lib.d2d_env_state_unpack(ref(ok), ref(pst), ref(_lib.EnvState(w, None, w, w, None, None)), None) == -1
    # the step needs actions
    assert lib.d2d_env_step_packed(ref(ok), ref(pst), None, None, None, 1, 0, None) == -1
    assert b"actions" in lib.d2d_last_error()
    # ineligible: a full row (D = 8, 16 with C = 8), C > 8 (left unpacked), another env kind
    for d, word in ((comb(6, 8, 8), b"max_deadline"), (comb(6, 8, 16), b"max_deadline"), (comb(6, 8, 4), b"max_deadline"),
                    (comb(6, 8, 12), b"max_deadline"), (comb(6, 16, 14), b"n_channels"), (comb(6, 32, 7), b"n_channels"),
                    (comb(4, 3, 7, kind=1), b"combinatorial")):
        for rc in (lib.d2d_env_reset_packed(ref(d), ref(pst), None, None, 0, None),
                   lib.d2d_env_step_packed(ref(d), ref(pst), w, None, None, 1, 0, None),
                   lib.d2d_env_state_pack(ref(d), ref(ust), ref(pst), None),
                   lib.d2d_env_state_unpack(ref(d), ref(pst), ref(ust), None)):
            assert rc == -2
            assert word in lib.d2d_last_error(), lib.d2d_last_error()
    # misaligned record
    bad_rec = _lib.EnvOut(None, None, None, None, None, 24)
    assert lib.d2d_env_reset_packed(ref(ok), ref(pst), None, ref(bad_rec), 0, None) == -1
    assert b"aligned" in lib.d2d_last_error()
    assert lib.d2d_env_step_packed(ref(ok), ref(pst), w, None, ref(bad_rec), 1, 0, None) == -1
    assert b"aligned" in lib.d2d_last_error()
    # the ABI version did not move
    assert lib.d2d_abi_version() == 15


def test_packed_struct_size_and_eligibility_mirror():
    from d2dhip import _lib
    from d2dhip.envbatch import packed_eligible
    from d2dhip.spec import EnvSpec
    assert ctypes.sizeof(_lib.EnvPackedState) == 2 * 8

    def spec(N, C, d):
        return EnvSpec("comb", N, C, d, [0.5] * N, 2, [1] * N, [0] * N, 10, "aperiodic", [], True, None)
    assert packed_eligible(spec(4, 8, [7, 14, 3, 14]))      # 14 + 1 <= 16
    assert packed_eligible(spec(4, 8, [7] * 4))             # 7 + 1 <= 8
    assert packed_eligible(spec(3, 4, [3] * 3))             # DW = 1
    assert not packed_eligible(spec(4, 8, [8] * 4))         # the row is full
    assert not packed_eligible(spec(4, 8, [16] * 4))
    assert not packed_eligible(spec(4, 16, [14] * 4))       # C > 8 stays unpacked


def _pack_np(buf, chan, recv, disc):
    """numpy restatement of d2d_env_state_pack: buf uint32 [..][DW], chan uint8, recv / disc uint32."""
    rows = buf.copy()
    rows[..., -1] = (rows[..., -1] & np.uint32(0x00FFFFFF)) | (chan.astype(np.uint32) << np.uint32(24))
    return rows, (recv & np.uint32(0xFFFF)) | (disc << np.uint32(16))


def _unpack_np(rows, counters):
    buf = rows.copy()
    buf[..., -1] &= np.uint32(0x00FFFFFF)
    return buf, (rows[..., -1] >> np.uint32(24)).astype(np.uint8), counters & np.uint32(0xFFFF), counters >> np.uint32(16)


def test_packed_bit_layout_against_hand_written_row():
    # D = 14 (DW = 4): cells 0..13 hold 1..14, the mask 0xA5 sits in byte 15, byte 14 stays zero
    cells = np.zeros(16, dtype=np.uint8)
    cells[:14] = np.arange(1, 15)
    buf = cells.view("<u4").reshape(1, 4).copy()
    rows, cnt = _pack_np(buf, np.array([0xA5], np.uint8), np.array([300], np.uint32), np.array([7], np.uint32))
    assert rows.tolist() == [[0x04030201, 0x08070605, 0x0C0B0A09, 0xA5000E0D]]
    assert cnt.tolist() == [300 | (7 << 16)] == [0x0007012C]
    b2, h2, r2, d2 = _unpack_np(rows, cnt)
    assert np.array_equal(b2, buf) and h2.tolist() == [0xA5] and r2.tolist() == [300] and d2.tolist() == [7]
    # D = 3 (DW = 1): the mask in the top byte of the only word
    buf1 = np.array([[0x00030201]], dtype=np.uint32)
    rows1, cnt1 = _pack_np(buf1, np.array([0x0F], np.uint8), np.array([65535], np.uint32), np.array([65535], np.uint32))
    assert rows1.tolist() == [[0x0F030201]] and cnt1.tolist() == [0xFFFFFFFF]
    b3, h3, r3, d3 = _unpack_np(rows1, cnt1)
    assert np.array_equal(b3, buf1) and h3.tolist() == [0x0F] and r3.tolist() == [65535] and d3.tolist() == [65535]
    # all-zero state is the same in both layouts
    z = np.zeros((2, 4), np.uint32)
    rz, cz = _pack_np(z, np.zeros(2, np.uint8), np.zeros(2, np.uint32), np.zeros(2, np.uint32))
    assert not rz.any() and not cz.any()
