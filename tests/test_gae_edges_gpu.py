"""csrc/gae_kernels.hip against float64 at every edge (pytest -m gpu).  The reference is tests/gae_scan_oracle.py, a
float64 restatement of the ABI contract, itself pinned on the CPU by tests/test_gae_scan_oracle_cpu.py.

Bars, and where each comes from:

* raw scan -- bit equality of adv and ret with scan_ref(...).astype(float32), for all six entry points
  (d2d_gae_scan, d2d_gae_scan_tce, d2d_gae_scan_moments with outputs in both layouts, d2d_gae_scan_normalized with
  mean0 = mean1 = NULL in both layouts).  The library is built with -ffp-contract=off and the kernels evaluate the
  recursion in scan_ref's operation order, one IEEE float64 operation at a time, so there is nothing left to differ.
  "Close to exact arithmetic" would be the wrong bar: a long-double recursion differs from float64 by 1 fp32 ulp in
  0.15 % of the elements (exact ties), see the CPU file.
* moments -- n exact; sum within rtol 1e-12, M2 within rtol 1e-11, both plus 1e-9 absolute, of float64 two-pass
  statistics of the stored fp32 outputs: the bars of tests/test_gae_gpu.py::test_gae_scan_moments_fused_stats, taken
  from that test and not from what the kernel returns.  MODE 0 (with outputs) and MODE 1 (moments only) agree bit for
  bit with each other and run to run (fixed-order combines, no atomics).
* statistics -- d2d_colstats_finalize through moments_stats / two_pass_column_stats: mean and 1 / std within rtol
  1e-12 of stats_ref for ddof 0 and 1 (float64 sums of at most 4.5 M terms of one sign scale are good to ~1e-13),
  the gate equal.
* normalised outputs -- the device's mean, 1 / std and gate are read back and the output is bit-equal to
  norm_ref(raw reference, mean, scale): nrm() is two float64 operations and one rounding with nothing to contract.
  The same for d2d_normalize_pair, d2d_normalize_columns and d2d_normalize_columns_tce.
* shards against one process -- 1 fp32 ulp plus scale_c 2^-40 (|mean_c| + 1), derived at
  test_sharded_protocol_equals_one_process.
* d2d_colstats / d2d_colstats_tce -- rtol 1e-12 plus 1e-9 absolute against float64 sums, bitwise reproducible.

Not reached: the n >= 2^31 branch of normalize_pair_kernel<false> (64-bit `j % cols`), which needs 8 GiB per tensor.

Every test prints its worst deviations as one JSON line (pytest -s); DESIGN.md section 6.5 quotes them.
"""
import functools
import json

import numpy as np
import pytest

import gae_scan_oracle as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda"
NAN = float("nan")
RTOL_SUM, RTOL_M2, ATOL_MOM, RTOL_STAT = 1e-12, 1e-11, 1e-9, 1e-12
ENTRY_POINTS = ["scan", "scan_tce", "moments0", "moments1", "normalized0", "normalized1"]
NORM_SHAPES = [(2, 5, 3), (7, 257, 3), (13, 5, 64), (37, 300, 4)]
WHICH = {"both": (True, True), "adv": (True, False), "ret": (False, True)}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm GPU")
    from d2dhip import _lib
    return _lib.require_gpu()


def check(rc, what):
    from d2dhip import _lib
    _lib.check(rc, what)


def stream():
    from d2dhip import _lib
    return _lib.stream_ptr()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def tce(x):
    """[T][E][cols] <-> [T][cols][E], always a copy (.contiguous() alone returns the same memory when E or cols is 1)"""
    return x.permute(0, 2, 1).clone(memory_format=torch.contiguous_format)


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ptr(t):
    return None if t is None else t.data_ptr()


def describe(x, ref):
    """how a device fp32 tensor differs from its reference (both in the same layout)"""
    a, b = x.cpu().numpy(), ref.cpu().numpy()
    ne = a.view(np.uint32) != b.view(np.uint32)
    i = tuple(int(k) for k in np.argwhere(ne)[0])
    with np.errstate(invalid="ignore"):
        ulps = int(G.ulp_distance(a, b)[ne].max())
    return f"{int(ne.sum())} of {ne.size} differ, first at {i}: {a[i]!r} != {b[i]!r}, max {ulps} ulp"


class Batch:
    """one shape's inputs on the host ([T][E][cols]) and on the device in both layouts"""

    def __init__(self, T, E, cols, seed=0, offset_column=False, val=None, rews=None, done_np=None):
        self.T, self.E, self.cols = T, E, cols
        if val is None:
            val, rews = G.inputs(T, E, cols, seed, offset_column)
        self.val_np, self.rew_np = val, rews
        v = dev(val)
        self.val = {0: v, 1: tce(v)}
        self.rew = {}
        for rk, r in rews.items():
            d = dev(r)
            self.rew[rk] = {0: d, 1: d if r.ndim == 2 else tce(d)}
        self.done_np = {dk: G.dones(dk, T) for dk in G.DONE_KINDS} if done_np is None else done_np
        self.done = {dk: dev(d) for dk, d in self.done_np.items()}

    def shard(self, a, b):
        return Batch(self.T, b - a, self.cols, val=self.val_np[:, a:b],
                     rews={k: r[:, a:b] for k, r in self.rew_np.items()}, done_np=self.done_np)

    def args(self, lay, rk, dk, gamma, lam, ls):
        r = self.rew[rk][lay]
        return (self.T, self.E, self.cols, 1 if r.dim() == 2 else self.cols, r.data_ptr(), self.val[lay].data_ptr(),
                self.done[dk].data_ptr(), float(gamma), float(lam), int(ls))

    def ref32(self, rk, dk, gamma, lam, ls):
        return G.scan_ref32(self.rew_np[rk], self.val_np, self.done_np[dk], gamma, lam, ls)

    def out(self, lay):
        return torch.full_like(self.val[lay], NAN)   # an element the kernel leaves out stays NaN


def ep_scan(lib, B, lay, args):
    adv, ret = B.out(lay), B.out(lay)
    fn = lib.d2d_gae_scan_tce if lay else lib.d2d_gae_scan
    check(fn(*args, adv.data_ptr(), ret.data_ptr(), stream()), "d2d_gae_scan")
    return adv, ret


def ep_moments(lib, B, lay, args, outputs=True):
    adv, ret = (B.out(lay), B.out(lay)) if outputs else (None, None)
    mom = torch.full((2, 3, B.cols), NAN, dtype=torch.float64, device=DEV)
    ws = torch.full((int(lib.d2d_gae_moments_workspace(B.E, B.cols, lay)),), NAN, dtype=torch.float64, device=DEV)
    check(lib.d2d_gae_scan_moments(*args, lay, ptr(adv), ptr(ret), mom.data_ptr(), ws.data_ptr(), ws.numel(), stream()),
          "d2d_gae_scan_moments")
    return adv, ret, mom


def ep_normalized(lib, B, lay, args, st0=None, st1=None):
    adv, ret = B.out(lay), B.out(lay)
    a0 = [t.data_ptr() for t in st0] if st0 is not None else [None] * 3
    a1 = [t.data_ptr() for t in st1] if st1 is not None else [None] * 3
    check(lib.d2d_gae_scan_normalized(*args, lay, adv.data_ptr(), *a0, ret.data_ptr(), *a1, stream()),
          "d2d_gae_scan_normalized")
    return adv, ret


def raw_outputs(lib, B, rk, dk, gamma, lam, ls, names=ENTRY_POINTS):
    """(entry point, layout, adv, ret) of every entry point that can write raw outputs"""
    for name in names:
        lay = 1 if name in ("scan_tce", "moments1", "normalized1") else 0
        args = B.args(lay, rk, dk, gamma, lam, ls)
        if name.startswith("scan"):
            adv, ret = ep_scan(lib, B, lay, args)
        elif name.startswith("moments"):
            adv, ret, _ = ep_moments(lib, B, lay, args)
        else:
            adv, ret = ep_normalized(lib, B, lay, args)
        yield name, lay, adv, ret


def both_layouts(x32):
    d = dev(x32)
    return {0: d, 1: tce(d)}


# ---------------------------------------------------------------- 2. the raw scan
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.shape_id)
def test_raw_scan_is_bitwise_scan_ref(lib, shape):
    """All six entry points, every (gamma, lam) x dones x last_shard x reward kind of the grid: adv and ret are
    bit-equal to scan_ref(...).astype(float32).  Bar from -ffp-contract=off and the identical operation order."""
    B = Batch(*shape)
    bad = []
    for (gamma, lam, dk, ls, rk) in G.settings():
        a32, r32 = B.ref32(rk, dk, gamma, lam, ls)
        ra, rr = both_layouts(a32), both_layouts(r32)
        for name, lay, adv, ret in raw_outputs(lib, B, rk, dk, gamma, lam, ls):
            for what, x, ref in (("adv", adv, ra[lay]), ("ret", ret, rr[lay])):
                if not same(x, ref):
                    bad.append(f"{name} {what} gamma={gamma} lam={lam} dones={dk} last_shard={ls} rewards={rk}: "
                               + describe(x, ref))
    assert not bad, f"{len(bad)} mismatches, first: " + "\n".join(bad[:6])


@pytest.mark.parametrize("shape", G.SHAPES, ids=G.shape_id)
def test_last_shard_changes_one_element_and_one_env(lib, shape):
    """Canary: with last_shard = 1 element (T-1, E-1, c) is fl32(r - v); ret does not change and no env but E-1
    changes between last_shard 0 and 1."""
    T, E, cols = shape
    B = Batch(*shape, seed=2)
    for rk in G.REWARD_KINDS:
        r_last = B.rew_np[rk][T - 1, E - 1] if rk == "percol" else np.full(cols, B.rew_np[rk][T - 1, E - 1])
        want = dev((r_last.astype(np.float64) - B.val_np[T - 1, E - 1]).astype(np.float32))
        for (gamma, lam) in G.GAMMA_LAM[:3]:
            for dk in G.DONE_KINDS:
                off = dict((n, (l, a, r)) for n, l, a, r in raw_outputs(lib, B, rk, dk, gamma, lam, 0))
                for name, lay, adv, ret in raw_outputs(lib, B, rk, dk, gamma, lam, 1):
                    where = f"{name} gamma={gamma} dones={dk} rewards={rk}"
                    _, adv0, ret0 = off[name]
                    assert same(ret, ret0), where
                    a1, a0 = (tce(adv), tce(adv0)) if lay else (adv, adv0)   # [T][E][cols]
                    assert same(a1[:, :E - 1], a0[:, :E - 1]), where
                    assert same(a1[T - 1, E - 1], want), where
                    assert not bool(torch.isnan(a1).any()), where


@pytest.mark.parametrize("shape", [(2, 5, 3), (5, 33, 5), (7, 257, 3), (13, 5, 64), (6, 3, 300)], ids=G.shape_id)
def test_envs_are_independent_when_the_last_slot_is_not_done(lib, shape):
    """Canary for the dones[T-1] = 0 contract: every env is its own sequence with zero bootstrap, so env e's outputs
    do not depend on env e+1's inputs.  Every second env is perturbed; the others keep their bits."""
    T, E, cols = shape
    val, rews = G.inputs(T, E, cols, seed=3)
    open_end = G.dones("bern", T)
    open_end[T - 1] = 0
    done_np = {"none": G.dones("none", T), "open": open_end}
    B = Batch(T, E, cols, val=val, rews=rews, done_np=done_np)
    for parity in (0, 1):
        hit = np.arange(E) % 2 == parity
        val2 = val.copy()
        val2[:, hit] = val2[:, hit] * -2 + 5
        rews2 = {k: r.copy() for k, r in rews.items()}
        for r in rews2.values():
            r[:, hit] += np.float32(1.5)
        B2 = Batch(T, E, cols, val=val2, rews=rews2, done_np=done_np)
        keep = dev(np.flatnonzero(~hit))
        touched = dev(np.flatnonzero(hit))
        for rk in G.REWARD_KINDS:
            for dk in done_np:
                for ls in (0, 1):
                    one = list(raw_outputs(lib, B, rk, dk, 0.9, 0.95, ls))
                    two = list(raw_outputs(lib, B2, rk, dk, 0.9, 0.95, ls))
                    for (name, lay, a1, r1), (_, _, a2, r2) in zip(one, two):
                        dim = 2 if lay else 1
                        for x1, x2 in ((a1, a2), (r1, r2)):
                            assert same(x1.index_select(dim, keep), x2.index_select(dim, keep)), (name, rk, dk, ls)
                            if len(touched):   # the perturbation is seen at all
                                assert not same(x1.index_select(dim, touched), x2.index_select(dim, touched))


# ---------------------------------------------------------------- 3. moments and statistics
class Worst(dict):
    def see(self, key, value):
        value = float(value)
        if value == value:
            self[key] = max(self.get(key, 0.0), value)


def rel(a, b):
    """max |a - b| / |b| over the finite, nonzero entries of b"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = np.isfinite(b) & (b != 0)
    return float((np.abs(a[ok] - b[ok]) / np.abs(b[ok])).max()) if ok.any() else 0.0


def check_moments(mom, ref_moments, where, worst):
    """mom [3][cols] of the device against moments_ref (float64 two-pass statistics) of the reference output"""
    n, s, m2 = ref_moments
    m = mom.cpu().numpy()
    assert (m[0] == n).all(), where
    np.testing.assert_allclose(m[1], s, rtol=RTOL_SUM, atol=ATOL_MOM, err_msg=where)
    np.testing.assert_allclose(m[2], m2, rtol=RTOL_M2, atol=ATOL_MOM, err_msg=where)
    worst.see("sum_bar_used", (np.abs(m[1] - s) / (ATOL_MOM + RTOL_SUM * np.abs(s))).max())
    worst.see("m2_bar_used", (np.abs(m[2] - m2) / (ATOL_MOM + RTOL_M2 * np.abs(m2))).max())
    worst.see("sum_rel", rel(m[1], s))
    worst.see("m2_rel", rel(m[2], m2))


def check_stats(st, x32, ddof, n, where, worst, ref_moments=None):
    """device (mean, scale, gate) against stats_ref of x32: rtol 1e-12, the gate equal; returns them on the host"""
    mean, scale, gate = (t.cpu().numpy() for t in st)
    rmean, rscale, rgate = G.stats_ref(x32, ddof, n, ref_moments)
    assert int(gate[0]) == rgate, where
    np.testing.assert_allclose(mean, rmean, rtol=RTOL_STAT, atol=0, err_msg=where)
    np.testing.assert_allclose(scale, rscale, rtol=RTOL_STAT, atol=0, err_msg=where)
    worst.see("mean_rel", rel(mean, rmean))
    worst.see("scale_rel", rel(scale, rscale))
    return mean, scale, int(gate[0])


@pytest.mark.parametrize("shape", G.SHAPES + [(1, 300, 5)], ids=G.shape_id)
def test_moments_and_statistics_against_float64(lib, shape):
    """d2d_gae_scan_moments with outputs (MODE 0) and without (MODE 1), both layouts, per-column rewards whose last
    column has offset 1e4 (SeqMom shifts every thread's sums by its first element, which is what keeps M2 of such a
    column at float64 level): n exact, sum rtol 1e-12, M2 rtol 1e-11, + 1e-9 absolute (the bars of
    test_gae_gpu.py::test_gae_scan_moments_fused_stats) against float64 two-pass statistics of the reference's fp32
    outputs; the four moment sets (two modes, two runs) bit-equal; mean / scale of d2d_colstats_finalize through
    moments_stats within rtol 1e-12 of stats_ref for ddof 0 and 1, gate equal."""
    from d2dhip.gae import moments_stats
    T, E, cols = shape
    B = Batch(T, E, cols, seed=4, offset_column=True)
    worst = Worst()
    for (gamma, lam) in G.GAMMA_LAM:
        for dk in G.DONE_KINDS:
            for ls in (0, 1):
                x32 = B.ref32("percol", dk, gamma, lam, ls)
                ref_mom = [G.moments_ref(x) for x in x32]
                ref_dev = [dev(x) for x in x32]
                for lay in (0, 1):
                    where = f"layout={lay} gamma={gamma} lam={lam} dones={dk} last_shard={ls}"
                    args = B.args(lay, "percol", dk, gamma, lam, ls)
                    adv, ret, m0 = ep_moments(lib, B, lay, args)
                    m1 = ep_moments(lib, B, lay, args, outputs=False)[2]
                    m0b = ep_moments(lib, B, lay, args)[2]
                    m1b = ep_moments(lib, B, lay, args, outputs=False)[2]
                    assert torch.equal(m0, m1) and torch.equal(m0, m0b) and torch.equal(m0, m1b), where
                    for k, (x, ref) in enumerate(zip((adv, ret), x32)):
                        assert same(tce(x) if lay else x, ref_dev[k]), where
                        check_moments(m0[k], ref_mom[k], where, worst)
                        for ddof in (0, 1):
                            check_stats(moments_stats(m0[k], ddof, T * E), ref, ddof, T * E, where + f" ddof={ddof}",
                                        worst, ref_mom[k])
    print(json.dumps({"gae_moments": dict(shape=G.shape_id(shape), **worst)}))


# ---------------------------------------------------------------- 4. normalised outputs
def device_stats(lib, B, lay, args, n, worst, refs, where):
    """what gae_returns computes inside: the moments-only scan and moments_stats (adv ddof 0, ret ddof 1); checked
    against stats_ref of the reference's outputs and read back"""
    from d2dhip.gae import moments_stats
    mom = ep_moments(lib, B, lay, args, outputs=False)[2]
    st = [moments_stats(mom[0], 0, n), moments_stats(mom[1], 1, n)]
    host = [check_stats(st[k], refs[k], k, n, where, worst) for k in (0, 1)]
    return st, host


def expected(x32, host, on):
    mean, scale, gate = host
    return G.norm_ref(x32, mean, scale) if (on and gate) else x32


def call_normalize_pair(lib, T, E, cols, lay, x0, st0, x1, st1):
    a0 = [ptr(x0)] + ([t.data_ptr() for t in st0] if x0 is not None else [None] * 3)
    a1 = [ptr(x1)] + ([t.data_ptr() for t in st1] if x1 is not None else [None] * 3)
    check(lib.d2d_normalize_pair(T, E, cols, lay, *a0, *a1, stream()), "d2d_normalize_pair")


@pytest.mark.parametrize("which", list(WHICH))
@pytest.mark.parametrize("layout", ["tec", "tce"])
@pytest.mark.parametrize("shape", NORM_SHAPES, ids=G.shape_id)
def test_normalised_outputs_are_bitwise_norm_ref(lib, shape, layout, which):
    """gae_returns (moments-only scan, statistics, d2d_gae_scan_normalized) and d2d_normalize_pair on the raw
    reference, normalising both outputs or one: with the device's mean, 1 / std and gate read back, the output is
    bit-equal to norm_ref(raw reference, mean, scale) -- nrm() is two float64 operations, nothing to contract -- and
    the device statistics are within rtol 1e-12 of stats_ref (the statistics bar of the moments test)."""
    from d2dhip.gae import gae_returns
    T, E, cols = shape
    lay = 1 if layout == "tce" else 0
    na, nr = WHICH[which]
    B = Batch(T, E, cols, seed=5)
    worst = Worst()
    for (gamma, lam, dk, ls, rk) in G.settings():
        where = f"gamma={gamma} lam={lam} dones={dk} last_shard={ls} rewards={rk}"
        refs = B.ref32(rk, dk, gamma, lam, ls)
        st, host = device_stats(lib, B, lay, B.args(lay, rk, dk, gamma, lam, ls), T * E, worst, refs, where)
        want = [both_layouts(expected(refs[0], host[0], na))[lay], both_layouts(expected(refs[1], host[1], nr))[lay]]
        adv, ret = gae_returns(B.rew[rk][lay], B.val[lay], B.done[dk], gamma, lam, normalize_adv=na, normalize_ret=nr,
                               last_shard=bool(ls), layout=layout)
        assert same(adv, want[0]), "gae_returns adv " + where + ": " + describe(adv, want[0])
        assert same(ret, want[1]), "gae_returns ret " + where + ": " + describe(ret, want[1])
        x0 = both_layouts(refs[0])[lay] if na else None
        x1 = both_layouts(refs[1])[lay] if nr else None
        call_normalize_pair(lib, T, E, cols, lay, x0, st[0], x1, st[1])
        if na:
            assert same(x0, want[0]), "normalize_pair x0 " + where + ": " + describe(x0, want[0])
        if nr:
            assert same(x1, want[1]), "normalize_pair x1 " + where + ": " + describe(x1, want[1])
    print(json.dumps({"gae_normalised": dict(shape=G.shape_id(shape), layout=layout, which=which, **worst)}))


def given_stats(cols, seed):
    rng = np.random.default_rng(seed)
    mean, scale = rng.standard_normal(cols) * 2 + 0.5, rng.random(cols) * 3 + 0.25
    return mean, scale


@pytest.mark.parametrize("lay,T,E,cols", [(1, 300, 4, 300), (1, 300, 3, 300), (0, 5, 7, 3), (0, 3, 5, 2), (0, 1, 1, 3),
                                          (0, 6, 3, 300), (1, 3, 1030, 2)])
def test_normalize_pair_at_the_shapes_nothing_else_reaches(lib, lay, T, E, cols):
    """d2d_normalize_pair with given statistics, x0 only, x1 only and both, every gate combination: bit-equal to
    norm_ref (or untouched).  Layout 1 with T cols = 90,000 > 65,535 rows (the row loop over gridDim.y) on the float4
    path (E = 4) and the scalar path (E = 3); layout 0 with cols in {2, 3} (the `cu % cols` wrap of a float4's four
    columns) and n % 4 in {1, 2, 3} (the tail; n = 3 is a tail alone)."""
    rng = np.random.default_rng([T, E, cols])
    x_np = [(rng.standard_normal((T, E, cols)) * 3 + 1).astype(np.float32) for _ in range(2)]
    stats_np = [given_stats(cols, 10), given_stats(cols, 11)]
    for g0, g1 in ((1, 1), (0, 1), (1, 0), (0, 0)):
        st = [(dev(m), dev(s), dev(np.array([g], dtype=np.int32))) for (m, s), g in zip(stats_np, (g0, g1))]
        want = [both_layouts(G.norm_ref(x, m, s) if g else x)[lay] for x, (m, s), g in zip(x_np, stats_np, (g0, g1))]
        for use0, use1 in ((True, True), (True, False), (False, True)):
            x = [both_layouts(x_np[0])[lay], both_layouts(x_np[1])[lay]]
            call_normalize_pair(lib, T, E, cols, lay, x[0] if use0 else None, st[0], x[1] if use1 else None, st[1])
            for k, used in enumerate((use0, use1)):
                ref = want[k] if used else both_layouts(x_np[k])[lay]
                assert same(x[k], ref), f"x{k} gates=({g0}, {g1}) used=({use0}, {use1}): " + describe(x[k], ref)


@pytest.mark.parametrize("T,E,cols", [(1, 1, 1), (5, 255, 3), (37, 300, 4), (1025, 257, 3), (300, 130, 64)])
def test_normalize_columns_entry_points(lib, T, E, cols):
    """d2d_normalize_columns on [rows = T E][cols] and d2d_normalize_columns_tce on [T][cols][E] with given
    statistics: bit-equal to norm_ref with the gate open, untouched with it closed.  300 x 130 x 64 = 2.5 M elements
    is more than the 8192 x 256 threads of the launch, so the grid-stride loop runs."""
    rng = np.random.default_rng([T, E, cols, 1])
    x_np = (rng.standard_normal((T, E, cols)) * 3 + 1).astype(np.float32)
    mean, scale = given_stats(cols, 12)
    for g in (1, 0):
        st = (dev(mean), dev(scale), dev(np.array([g], dtype=np.int32)))
        want = both_layouts(G.norm_ref(x_np, mean, scale) if g else x_np)
        x = both_layouts(x_np)
        check(lib.d2d_normalize_columns(T * E, cols, x[0].data_ptr(), *[t.data_ptr() for t in st], stream()),
              "d2d_normalize_columns")
        assert same(x[0], want[0]), f"gate={g}: " + describe(x[0], want[0])
        check(lib.d2d_normalize_columns_tce(T, cols, E, x[1].data_ptr(), *[t.data_ptr() for t in st], stream()),
              "d2d_normalize_columns_tce")
        assert same(x[1], want[1]), f"tce gate={g}: " + describe(x[1], want[1])


def constant_column_batch(T, E, cols, seed):
    """gamma = 0 inputs whose column 1 of BOTH outputs is the nonzero constant 0.1f: the per-column reward is 0.1f
    everywhere, so ret = r = 0.1f and adv = (r - v) + v = 0.1f (r - v is exact in float64 for fp32 r and v of these
    magnitudes); the value under the one element last_shard rewrites to r - v is 0, so that it stays 0.1f too."""
    val, rews = G.inputs(T, E, cols, seed)
    rews = {"percol": rews["percol"]}
    rews["percol"][..., 1] = np.float32(0.1)
    val[T - 1, E - 1, 1] = 0.0
    return Batch(T, E, cols, val=val, rews=rews)


@pytest.mark.parametrize("layout", ["tec", "tce"])
def test_constant_nonzero_column_keeps_the_gate_closed(lib, layout):
    """Quirk Q2 with a constant column that is not zero (0.1f; the existing gate test uses zeros, where a wrong
    shift or a wrong mean still gives M2 = 0): E = 600 spans 3 (layout 1) resp. 10 (layout 0) blocks.  Every
    `which`, last_shard 0 and 1: the outputs are bit-equal to the raw ones.  Without the constant column the same
    call does normalise (the test would notice a gate that is always closed)."""
    from d2dhip.gae import gae_returns
    T, E, cols = 9, 600, 3
    lay = 1 if layout == "tce" else 0
    B = constant_column_batch(T, E, cols, seed=6)
    C = Batch(T, E, cols, seed=6)
    for dk in ("last", "bern"):
        for ls in (0, 1):
            a32, r32 = B.ref32("percol", dk, 0.0, 0.5, ls)
            k = np.float32(0.1)
            assert (a32[..., 1] == k).all() and (r32[..., 1] == k).all() and G.stats_ref(a32, 0)[2] == 0
            raw = [both_layouts(a32)[lay], both_layouts(r32)[lay]]
            for which, (na, nr) in WHICH.items():
                adv, ret = gae_returns(B.rew["percol"][lay], B.val[lay], B.done[dk], 0.0, 0.5, normalize_adv=na,
                                       normalize_ret=nr, last_shard=bool(ls), layout=layout)
                assert same(adv, raw[0]) and same(ret, raw[1]), (dk, ls, which)
            adv, ret = gae_returns(C.rew["percol"][lay], C.val[lay], C.done[dk], 0.0, 0.5, last_shard=bool(ls),
                                   layout=layout)
            c32 = C.ref32("percol", dk, 0.0, 0.5, ls)
            assert not same(adv, both_layouts(c32[0])[lay]) and not same(ret, both_layouts(c32[1])[lay])


# ---------------------------------------------------------------- 5. the cross-rank protocol in one process
SHARDINGS = [(130, 170), (1, 299), (7, 256, 37)]


def sharded_stats(lib, shards, lay, rk, dk, gamma, lam, n_total):
    """two_pass_column_stats over the shards' moments: every shard runs the moments-only scan (last_shard on the
    last one only) and builds its colsum with moments_colsum(m, True); adding the shards' vectors is the all-reduce;
    finalize is d2d_colstats_finalize with n = the whole batch's rows.  Returns [(mean, scale, gate)] for adv, ret."""
    from d2dhip.gae import moments_colsum, two_pass_column_stats
    moms = [ep_moments(lib, S, lay, S.args(lay, rk, dk, gamma, lam, int(S is shards[-1])), outputs=False)[2]
            for S in shards]
    cols = shards[0].cols
    out = []
    for k, ddof in ((0, 0), (1, 1)):
        parts = [moments_colsum(m[k], True) for m in moms]
        mean = torch.full((cols,), NAN, dtype=torch.float64, device=DEV)
        scale = torch.full((cols,), NAN, dtype=torch.float64, device=DEV)
        gate = torch.zeros(1, dtype=torch.int32, device=DEV)

        def colsum(center):
            return functools.reduce(torch.add, [p(center) for p in parts])

        def finalize(s1, m2):
            check(lib.d2d_colstats_finalize(cols, s1.data_ptr(), ptr(m2), float(n_total), ddof, mean.data_ptr(),
                                            None if m2 is None else scale.data_ptr(),
                                            None if m2 is None else gate.data_ptr(), stream()), "d2d_colstats_finalize")
            return mean, scale, gate

        out.append(two_pass_column_stats(colsum, finalize, None))
    return out


def sharded_outputs(lib, shards, lay, rk, dk, gamma, lam, st):
    outs = [ep_normalized(lib, S, lay, S.args(lay, rk, dk, gamma, lam, int(S is shards[-1])), st[0], st[1])
            for S in shards]
    dim = 2 if lay else 1
    return torch.cat([o[0] for o in outs], dim), torch.cat([o[1] for o in outs], dim)


def split(B, sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    assert edges[-1] == B.E
    return [B.shard(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("layout", ["tec", "tce"])
@pytest.mark.parametrize("sizes", SHARDINGS, ids=lambda s: "+".join(map(str, s)))
def test_sharded_protocol_equals_one_process(lib, sizes, layout):
    """E = 300 envs split into env shards, no torch.distributed: the data-parallel statistics protocol run by hand.

    * the sharded mean / scale are within rtol 1e-12 of stats_ref of the WHOLE batch and the gate is equal (the
      statistics bar of the moments test);
    * every shard's d2d_gae_scan_normalized output, concatenated, is bit-equal to norm_ref(raw reference, the
      read-back statistics);
    * against one-process gae_returns on the whole batch: |out' - out| <= 1 fp32 ulp + scale_c 2^-40 (|mean_c| + 1).
      Not bitwise: Chan's combination runs over other partials in another order, so mean' and scale' differ from
      mean and scale in their last float64 bits.  The test asserts |mean' - mean| <= 2^-40 (|mean| + 1) and
      |scale' - scale| <= 2^-40 scale on the read-back values.  Then with y = (x - mean) scale before rounding,
      y' - y = (mean - mean') scale' + (x - mean)(scale' - scale); the first term is at most scale 2^-40 (|mean| + 1),
      the second at most |y| 2^-40, which is 2^-16 of an fp32 ulp of y; and two values that close round to fp32
      numbers at most one ulp further apart than they are.
    """
    from d2dhip.gae import gae_returns, moments_stats
    T, E, cols = 11, 300, 5
    lay = 1 if layout == "tce" else 0
    B = Batch(T, E, cols, seed=7, offset_column=True)
    shards = split(B, sizes)
    n = T * E
    worst = Worst()
    for (gamma, lam, dk, _, rk) in [s for s in G.settings() if s[3] == 1]:
        where = f"gamma={gamma} lam={lam} dones={dk} rewards={rk}"
        refs = B.ref32(rk, dk, gamma, lam, 1)
        st = sharded_stats(lib, shards, lay, rk, dk, gamma, lam, n)
        host = [check_stats(st[k], refs[k], k, n, where, worst) for k in (0, 1)]
        adv, ret = sharded_outputs(lib, shards, lay, rk, dk, gamma, lam, st)
        for k, x in enumerate((adv, ret)):
            want = both_layouts(expected(refs[k], host[k], True))[lay]
            assert same(x, want), f"output {k} " + where + ": " + describe(x, want)
        # one process, whole batch
        mom = ep_moments(lib, B, lay, B.args(lay, rk, dk, gamma, lam, 1), outputs=False)[2]
        one = [tuple(t.cpu().numpy() for t in moments_stats(mom[k], k, n)) for k in (0, 1)]
        adv1, ret1 = gae_returns(B.rew[rk][lay], B.val[lay], B.done[dk], gamma, lam, layout=layout)
        for k, (x, x1) in enumerate(((adv, adv1), (ret, ret1))):
            mean, scale, gate = host[k]
            mean1, scale1, gate1 = one[k]
            assert gate == int(gate1[0]) == 1, where
            assert (np.abs(mean - mean1) <= 2.0 ** -40 * (np.abs(mean1) + 1)).all(), where
            assert (np.abs(scale - scale1) <= 2.0 ** -40 * scale1).all(), where
            worst.see("mean_vs_one_process_rel", rel(mean, mean1))
            worst.see("scale_vs_one_process_rel", rel(scale, scale1))
            a = (tce(x) if lay else x).cpu().numpy()        # [T][E][cols]
            b = (tce(x1) if lay else x1).cpu().numpy()
            ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
            bound = ulp.astype(np.float64) + scale1 * 2.0 ** -40 * (np.abs(mean1) + 1)
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            assert (d <= bound).all(), f"output {k} " + where + f": worst {float((d / bound).max())} of the bound"
            worst.see("out_vs_one_process_ulps", G.ulp_distance(a, b).max())
            worst.see("out_vs_one_process_differ", float((d > 0).mean()))
            worst.see("out_bound_used", (d / bound).max())
    print(json.dumps({"gae_sharded": dict(sizes=list(sizes), layout=layout, **worst)}))


@pytest.mark.parametrize("layout", ["tec", "tce"])
@pytest.mark.parametrize("sizes", SHARDINGS, ids=lambda s: "+".join(map(str, s)))
def test_sharded_gate_stays_closed_on_a_constant_nonzero_column(lib, sizes, layout):
    """The constant 0.1f column across shards: every shard's local mean is k exactly and n k is exact in float64, so
    the all-reduced mean is k, n_loc (mean_loc - mean)^2 = 0 on every shard, M2 = 0 and the gate stays closed for
    adv and ret: the sharded outputs are bit-equal to the raw reference."""
    T, E, cols = 9, 300, 3
    lay = 1 if layout == "tce" else 0
    B = constant_column_batch(T, E, cols, seed=8)
    shards = split(B, sizes)
    for dk in ("last", "bern"):
        refs = B.ref32("percol", dk, 0.0, 0.5, 1)
        st = sharded_stats(lib, shards, lay, "percol", dk, 0.0, 0.5, T * E)
        for k in (0, 1):
            mean, scale, gate = (t.cpu().numpy() for t in st[k])
            assert int(gate[0]) == 0 and mean[1] == np.float64(np.float32(0.1)) and np.isinf(scale[1]), (dk, k)
        adv, ret = sharded_outputs(lib, shards, lay, "percol", dk, 0.0, 0.5, st)
        assert same(adv, both_layouts(refs[0])[lay]) and same(ret, both_layouts(refs[1])[lay]), dk


# ---------------------------------------------------------------- 6. d2d_colstats, d2d_colstats_tce, normalize_columns_
def colstat_input(shape, seed):
    """fp32 [..., cols], every column of one sign scale (mean 3, spread 2), column 0 with offset 1e4"""
    rng = np.random.default_rng([seed] + list(shape))
    x = (rng.standard_normal(shape) * 2 + 3).astype(np.float32)
    x[..., 0] += np.float32(G.OFFSET)
    return x


def check_colstats(run, x_np, where, worst):
    """run(center or None) -> device float64 [cols]; against float64 column sums, twice for reproducibility"""
    xc = G.columns(x_np)
    cols = xc.shape[0]
    center_np = xc.mean(1) + np.random.default_rng(cols).standard_normal(cols) * 0.1
    for center, ref in ((None, xc.sum(1)), (dev(center_np), ((xc - center_np[:, None]) ** 2).sum(1))):
        a, b = run(center), run(center)
        assert torch.equal(a, b), where
        got = a.cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-9, err_msg=where)
        worst.see("sum_rel" if center is None else "sq_rel", rel(got, ref))


@pytest.mark.parametrize("cols", [1, 3, 64, 65, 300])
def test_colstats_against_float64(lib, cols):
    """d2d_colstats, center NULL (sums) and given (sums of squared deviations): rtol 1e-12 + 1e-9 absolute against
    float64 column sums, bitwise reproducible.  rows = 1, 15, one less and one more than the 16 rlanes rows of one
    row block, and at cols = 64 rows = 70,000: 1094 row blocks capped at 1024, so the row stride loop runs."""
    ct = 1
    while ct < cols and ct < 64:
        ct <<= 1
    rlanes = 256 // ct
    worst = Worst()
    for rows in [1, 15, 16 * rlanes - 1, 16 * rlanes + 1] + ([70000] if cols == 64 else []):
        x_np = colstat_input((rows, cols), 20)
        x = dev(x_np)
        ws = torch.full((int(lib.d2d_colstats_workspace(rows, cols)),), NAN, dtype=torch.float64, device=DEV)

        def run(center):
            out = torch.full((cols,), NAN, dtype=torch.float64, device=DEV)
            check(lib.d2d_colstats(rows, cols, x.data_ptr(), ptr(center), ws.data_ptr(), out.data_ptr(), stream()),
                  "d2d_colstats")
            return out

        check_colstats(run, x_np, f"rows={rows} cols={cols}", worst)
    print(json.dumps({"colstats": dict(cols=cols, **worst)}))


@pytest.mark.parametrize("cols", [1, 3])
@pytest.mark.parametrize("T", [1, 5, 1025])
def test_colstats_tce_against_float64(lib, T, cols):
    """d2d_colstats_tce on [T][cols][E], E = 1, 255, 257 (one lane, one short of and one past a 256-lane pass),
    T = 1025 being more than the 1024 slot blocks: the same bars."""
    worst = Worst()
    for E in (1, 255, 257):
        x_np = colstat_input((T, E, cols), 21)
        x = tce(dev(x_np))
        ws = torch.full((int(lib.d2d_colstats_workspace(T * E, cols)),), NAN, dtype=torch.float64, device=DEV)

        def run(center):
            out = torch.full((cols,), NAN, dtype=torch.float64, device=DEV)
            check(lib.d2d_colstats_tce(T, cols, E, x.data_ptr(), ptr(center), ws.data_ptr(), out.data_ptr(), stream()),
                  "d2d_colstats_tce")
            return out

        check_colstats(run, x_np, f"T={T} E={E} cols={cols}", worst)
    print(json.dumps({"colstats_tce": dict(T=T, cols=cols, **worst)}))


@pytest.mark.parametrize("constant", [False, True], ids=["spread", "constant-column"])
@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("layout", ["rows", "tce"])
def test_normalize_columns_end_to_end(lib, layout, ddof, constant):
    """gae.normalize_columns_, plain and tce=: it returns the gate of stats_ref; with the gate open x is bit-equal to
    norm_ref(x, mean, scale) for the device's statistics (the same d2d_colstats / d2d_colstats_finalize calls made
    again and read back; they are reproducible), which are within rtol 1e-12 of stats_ref; with one constant
    (nonzero) column the gate is closed and x keeps its bits."""
    from d2dhip.gae import normalize_columns_, two_pass_column_stats
    T, E, cols = 7, 143, 5
    x_np = colstat_input((T, E, cols), 22)
    if constant:
        x_np[..., 2] = np.float32(0.1)
    is_tce = layout == "tce"
    x = tce(dev(x_np)) if is_tce else dev(x_np).view(T * E, cols)
    rows = T * E
    ws = torch.full((int(lib.d2d_colstats_workspace(rows, cols)),), NAN, dtype=torch.float64, device=DEV)
    st = (torch.full((cols,), NAN, dtype=torch.float64, device=DEV),
          torch.full((cols,), NAN, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))

    def colsum(center):
        out = torch.full((cols,), NAN, dtype=torch.float64, device=DEV)
        if is_tce:
            check(lib.d2d_colstats_tce(T, cols, E, x.data_ptr(), ptr(center), ws.data_ptr(), out.data_ptr(), stream()),
                  "d2d_colstats_tce")
        else:
            check(lib.d2d_colstats(rows, cols, x.data_ptr(), ptr(center), ws.data_ptr(), out.data_ptr(), stream()),
                  "d2d_colstats")
        return out

    def finalize(s1, m2):
        check(lib.d2d_colstats_finalize(cols, s1.data_ptr(), ptr(m2), float(rows), ddof, st[0].data_ptr(),
                                        None if m2 is None else st[1].data_ptr(),
                                        None if m2 is None else st[2].data_ptr(), stream()), "d2d_colstats_finalize")
        return st

    two_pass_column_stats(colsum, finalize, None)
    worst = Worst()
    mean, scale, gate = check_stats(st, x_np, ddof, rows, f"{layout} ddof={ddof}", worst)
    assert gate == (0 if constant else 1)
    got_gate = normalize_columns_(x, ddof, tce=(T, cols, E) if is_tce else None)
    assert int(got_gate.item()) == gate
    want = dev(G.norm_ref(x_np, mean, scale) if gate else x_np)
    want = tce(want) if is_tce else want.view(rows, cols)
    assert same(x, want), describe(x, want)
    print(json.dumps({"normalize_columns_": dict(layout=layout, ddof=ddof, constant=constant, **worst)}))
