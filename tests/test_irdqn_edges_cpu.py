"""The input sets of tests/test_irdqn_edges_gpu.py (tests/irdqn_cases.py), checked on the CPU against the float64
oracle of tests/irdqn_oracle.py, and the iRDQN C ABI's sizes and empty batches on a GPU-less host.

- The table reaches every hidden tile count HT = 1 .. 8 and every input tile count IT = 1 .. 4 of the kernels, HT = 1
  and HT = 8 at all four IT, the ragged last tiles and all four (F % 4 == 0, H % 4 == 0) combinations that choose
  between 16-byte and masked scalar fragment loads.
- Every set meets the conditions under which the GPU file needs one strict branch.  torch float32 autograd lies within
  2e-5 max|g64| + 1e-7 of float64 for every *block* of every gradient tensor (irdqn_cases.blocks: each gate, each head
  layer, the rows of the last hidden tile and the rest apart) and both losses; no head-relu pre-activation of either
  layer lies within 2 (H + 2) 2^-24 (|b| + sum |w| |v|) of zero; |delta| falls on both sides of 1 where B >= 16; `done`
  is both set and clear (B >= 2); the unused input columns of the ring and of W_ih are exactly zero; at most 1 % of
  the float64 greedy decisions are within 1e-5 of a tie.  These are conditions on the reference alone, not
  measurements of a kernel; a set that misses one takes the next seed (irdqn_cases.BUMP).
- d2d_rdqn_grad_workspace and d2d_rdqn_carry_floats equal their layouts' sums at a ragged (H, F, B, L); an empty batch
  is D2D_OK for the Q entry and D2D_EINVAL for the gradient entry, before any HIP call."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

import irdqn_cases as C  # noqa: E402

CASES = C.all_cases()


def test_case_table_is_consistent():
    ids = [C.cid(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        assert 1 <= c.H <= 128 and 1 <= c.F <= 63 and 1 <= c.A <= 16 and 1 <= c.L <= 256
        assert c.L < 64 or c.B <= 2, "long windows: two samples (the reference's cost)"
    reached = {C.tiles(c) for c in CASES}
    assert {ht for ht, _ in reached} == set(range(1, 9)) and {it for _, it in reached} == {1, 2, 3, 4}
    assert reached >= {(ht, it) for ht in (1, 8) for it in (1, 2, 3, 4)}
    assert {C.tiles(c) for c in C.MATRIX} == {(1, 1), (1, 2), (1, 3), (1, 4), (8, 1), (8, 2), (8, 3), (8, 4),
                                             (2, 1), (3, 2), (4, 3), (5, 4), (6, 1), (7, 2)}
    assert {c.H % 16 for c in CASES} >= {0, 1, 2, 15} and {c.F % 16 for c in CASES} >= {0, 1, 15}
    assert {c.H - 16 * (C.tiles(c)[0] - 1) for c in C.RAGGED_H} >= {1, 2, 4, 10, 15}
    assert {(c.F % 4 == 0, c.H % 4 == 0) for c in CASES} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(c.H % 4 == 0, C.tiles(c)[0] > 4) for c in C.RAGGED_H} >= {(False, False), (False, True)}
    assert {c.A for c in C.RAGGED_A} == {1, 2, 3, 5, 9, 15, 16} and {c.B for c in C.BATCH} == {1, 15, 16, 33, 48}
    assert {c.L for c in C.WINDOW} == {1, 2, 64, 65, 256}
    assert C.UNALIGNED in CASES and C.INVALID in CASES and C.BASE in CASES
    assert set(C.BUMP) <= set(ids), "a bump for a set that is not in the table"
    for c in CASES:            # every window list the description promises
        r = C.ref(c)
        if c.ep:
            assert [s[1] for s in r.samples[:6]] == [4, 7, 9, 17, 2, 0]
        elif c.L > 1:
            assert r.samples[0][1] - c.L + 1 < 0, "no window wraps the ring"
        if c.B >= 3:
            assert {s[2] for s in r.qsamples} == {1, 2, c.L}


@pytest.mark.parametrize("c", CASES, ids=C.cid)
def test_input_set_conditions(c):
    worst = C.conditions(c)
    print(f"  torch fp32 at {worst:.3f} of the tightest block's gradient tolerance")


@pytest.mark.parametrize("name", sorted(C.BUMP))
def test_bump_is_the_first_that_meets_the_conditions(name):
    c = next(c for c in CASES if C.cid(c) == name)
    assert c.bump == C.BUMP[name] and C.first_bump(c._replace(bump=0), limit=c.bump + 1) == c.bump


@pytest.mark.parametrize("loss", C.LOSSES)
def test_single_sample_and_excluded_action_references(loss):
    """The two references the GPU file builds beside the sets' own meet the block condition too: the base set's
    samples launched alone, and the A = 5 set with excluded and two-bit action masks."""
    r = C.ref(C.BASE)
    worst = 0.0
    refs = [(C.BASE, C.single(r, b), None) for b in C.SINGLES]
    ri = C.ref(C.INVALID)
    masks, act, weight = C.invalid_actions(ri)
    assert int((weight == 0).sum()) == 5 and bool(((masks >> act) & 1)[weight == 1].all())
    refs.append((C.INVALID, (ri.samples, act, ri.reward, ri.done, ri.qt), weight))
    for c, inputs, w in refs:
        rr = C.ref(c)
        with C.one_thread():
            g64, l64, _ = C.td_ref(c, rr.p, rr.ring, *inputs, loss, torch.float64, weight=w)
            g32, l32, _ = C.td_ref(c, rr.p, rr.ring, *inputs, loss, torch.float32, weight=w)
        for label, name, idx in C.blocks(c):
            tol = C.block_tol(g64[name][idx])
            band = (g32[name][idx] - g64[name][idx]).abs().max().item()
            worst = max(worst, band / tol)
            assert band <= tol, (label, band, tol)
    print(f"  torch fp32 at {worst:.3f} of the tightest block's gradient tolerance")


def _desc(_lib, N=2, E=3, F=30, H=50, A=8, rows=7):
    w = ctypes.c_void_p(16)
    return _lib.RdqnDesc(N, E, F, H, A, rows, 0, 0, *([w] * 10), 0, 0, None)


@pytest.mark.parametrize("shape", [(2, 50, 30, 17, 3), (3, 113, 49, 33, 65), (1, 1, 1, 1, 1), (2, 128, 63, 48, 256)],
                         ids=lambda s: "N%d-H%d-F%d-B%d-L%d" % s)
def test_workspace_and_carry_sizes_at_ragged_shapes(shape):
    """x [L][Bp][IW] + h [L + 1][Bp][HW] + gates [L][Bp][4 HW] + y1, y2, d1, d2 [Bp][HW] + dq [Bp][16] + one loss per
    tile, per agent; the carried h image [N][tiles][HT][64] f32x4"""
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    N, H, F, B, L = shape
    nt = -(-B // 16)
    Bp, HW, IW = 16 * nt, 16 * -(-H // 16), 16 * -(-F // 16)
    want = N * (L * Bp * IW + (L + 1) * Bp * HW + L * Bp * 4 * HW + 4 * Bp * HW + Bp * 16 + nt)
    d = _desc(_lib, N=N, F=F, H=H)
    assert lib.d2d_rdqn_grad_workspace(ctypes.byref(d), B, L) == want
    assert lib.d2d_rdqn_carry_floats(ctypes.byref(d), B) == N * nt * (HW // 16) * 64 * 4 == N * Bp * HW
    assert lib.d2d_rdqn_grad_workspace(ctypes.byref(d), B, 0) == -1
    assert lib.d2d_rdqn_carry_floats(ctypes.byref(d), 0) == 0
    assert lib.d2d_rdqn_grad_workspace(ctypes.byref(d), 0, L) == 0


def test_empty_batch_before_any_hip_call():
    import d2dhip
    from d2dhip import _lib
    lib = d2dhip.load()
    w = ctypes.c_void_p(16)
    d = _desc(_lib)
    for hc in (None, w):
        rc = lib.d2d_rdqn_q_ex(ctypes.byref(d), w, _lib.D2D_OBS_F32, None, w, 0, 0, _lib.D2D_RDQN_EPS, 0.5, w, 1, None,
                               None, 0, hc, 0, w, w, w, None)
        assert rc == 0
    ws = lib.d2d_rdqn_grad_workspace(ctypes.byref(d), 16, 3)
    for entry, head in ((lib.d2d_rdqn_grad_ex, (w, _lib.D2D_OBS_F32, None)), (lib.d2d_rdqn_grad, (w,))):
        rc = entry(ctypes.byref(d), *head, w, 0, 3, w, w, w, w, 0.4, 0, *([w] * 12), ws, None)
        assert rc == -1 and b"B < 1" in lib.d2d_last_error()
