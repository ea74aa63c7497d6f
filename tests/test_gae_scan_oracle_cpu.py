"""The reference of tests/test_gae_edges_gpu.py, checked on the CPU (tests/gae_scan_oracle.py).

- Pinned to the existing oracle: with dones[-1] = 1 and last_shard = 1 the ABI contract (independent envs) IS the
  reference's env-major concatenated sequence, so scan_ref normalised with stats_ref gives
  oracle.gae_oracle.gae_returns_batched within 1e-6 (adv differs by one fp32 rounding before the normalisation: the
  kernels normalise the stored fp32 values, compute_gae the float64 ones), and reproduces
  tests/golden/gae_returns.npz at that file's bar, 1e-5.
- With dones[-1] = 0 the two differ by O(1) in normalised units: the contract is not the concatenation there.
- Independent precision check: scan_ref in np.longdouble (64-bit mantissa) against scan_ref in float64, both rounded
  to fp32, over the (gamma, lam) x dones x last_shard x rewards grid of the GPU file.  Bar: at most 1 fp32 ulp
  apart, or closer than float64_floor (values that cancel to near 0 carry the float64 recursion's absolute error,
  which is many ulps of a tiny value).  Measured: see test_float64_scan_is_within_one_ulp_of_long_double.  The
  elements that differ are exact fp32 ties of the float64 value, which gamma in {0, 0.5, 1} produce.  That is why the
  GPU bar is bit equality with the same-order float64 restatement and not "close to exact arithmetic".
"""
import json
import os

import numpy as np
import pytest

import gae_scan_oracle as G
from conftest import GOLDEN
from oracle.gae_oracle import gae_returns_batched

# the shapes of the grid up to 44,400 elements (the two 258-partial shapes add no new arithmetic)
CPU_SHAPES = [s for s in G.SHAPES if s[0] * s[1] * s[2] <= 50000]


def normalised(rew, val, done, gamma, lam, last_shard):
    adv, ret = G.scan_ref32(rew, val, done, gamma, lam, last_shard)
    out = []
    for x, ddof in ((adv, 0), (ret, 1)):
        mean, scale, gate = G.stats_ref(x, ddof)
        out.append(G.norm_ref(x, mean, scale) if gate else x)
    return out


@pytest.mark.parametrize("T,E,cols", [(40, 9, 4), (7, 257, 3), (37, 300, 4)])
@pytest.mark.parametrize("gamma,lam", [(0.6, 0.97), (0.99, 0.95), (0.5, 1.0)])
@pytest.mark.parametrize("rk", G.REWARD_KINDS)
def test_scan_ref_is_the_batched_oracle_when_the_last_slot_is_done(T, E, cols, gamma, lam, rk):
    val, rews = G.inputs(T, E, cols, seed=1)
    for dk in ("last", "bern"):
        done = G.dones(dk, T)
        done[-1] = 1
        adv, ret = normalised(rews[rk], val, done, gamma, lam, 1)
        adv_o, ret_o = gae_returns_batched(rews[rk], val, done, gamma, lam)
        np.testing.assert_allclose(adv, adv_o, rtol=0, atol=1e-6)
        np.testing.assert_allclose(ret, ret_o, rtol=0, atol=1e-6)


def test_contract_is_not_the_concatenation_when_the_last_slot_is_not_done():
    """dones[T-1] = 0: the kernels (and scan_ref) still start every env at zero bootstrap; the reference's
    concatenated sequence would carry env e+1's first step into env e's last.  The difference is O(1)."""
    T, E, cols = 40, 9, 4
    val, rews = G.inputs(T, E, cols, seed=1)
    done = G.dones("none", T)
    adv, ret = normalised(rews["bcast"], val, done, 0.6, 0.97, 1)
    adv_o, ret_o = gae_returns_batched(rews["bcast"], val, done, 0.6, 0.97)
    assert max(np.abs(adv - adv_o).max(), np.abs(ret - ret_o).max()) > 0.5


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "gae_returns.npz"))


@pytest.mark.parametrize("case", ["small", "mid", "big"])
@pytest.mark.parametrize("gamma", [0.6, 0.99])
def test_scan_ref_reproduces_the_golden_vectors(z, case, gamma):
    rew, val, done = z[f"{case}_rew"], z[f"{case}_val"], z[f"{case}_done"]
    adv, ret = normalised(rew[:, None, :], val[:, None, :], done, gamma, 0.97, 1)   # one env, N agent columns
    np.testing.assert_allclose(adv[:, 0], z[f"{case}_g{gamma}_adv"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(ret[:, 0], z[f"{case}_g{gamma}_ret"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("case,gamma", [("zerostd", 0.9), ("alldone", 0.8)])
def test_scan_ref_reproduces_the_golden_edge_cases(z, case, gamma):
    rew, val, done = z[f"{case}_rew"], z[f"{case}_val"], z[f"{case}_done"]
    adv, ret = normalised(rew[:, None, :], val[:, None, :], done, gamma, 0.97, 1)
    np.testing.assert_allclose(adv[:, 0], z[f"{case}_adv"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(ret[:, 0], z[f"{case}_ret"], rtol=0, atol=1e-5)


def test_last_shard_touches_one_element_and_one_env():
    T, E, cols = 7, 5, 3
    val, rews = G.inputs(T, E, cols)
    for rk in G.REWARD_KINDS:
        a0, r0 = G.scan_ref32(rews[rk], val, G.dones("bern", T), 0.9, 0.95, 0)
        a1, r1 = G.scan_ref32(rews[rk], val, G.dones("bern", T), 0.9, 0.95, 1)
        assert G.same_bits(r0, r1) and G.same_bits(a0[:, :E - 1], a1[:, :E - 1])
        r_last = rews[rk][T - 1, E - 1] if rk == "percol" else np.full(cols, rews[rk][T - 1, E - 1])
        assert G.same_bits(a1[T - 1, E - 1], (r_last.astype(np.float64) - val[T - 1, E - 1]).astype(np.float32))


def test_helpers():
    x = np.array([1.0, -1.0, 0.0, 1e-45, 3.0], dtype=np.float32)
    y = np.array([np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0, -1e-45, 3.0], dtype=np.float32)
    assert G.ulp_distance(x, y).tolist() == [1, 0, 0, 2, 0]
    assert not G.same_bits(x, y) and G.same_bits(x, x.copy())
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((50, 7, 3)) + 5).astype(np.float32)
    x[..., 1] = np.float32(0.1)
    for ddof in (0, 1):
        mean, scale, gate = G.stats_ref(x, ddof)
        assert gate == 0 and mean[1] == np.float64(np.float32(0.1)) and np.isinf(scale[1])
        x2 = x[..., [0, 2]]
        mean, scale, gate = G.stats_ref(x2, ddof)
        flat = x2.reshape(-1, 2).astype(np.float64)
        assert gate == 1
        np.testing.assert_allclose(mean, flat.mean(0), rtol=1e-14)
        np.testing.assert_allclose(scale, 1 / flat.std(0, ddof=ddof), rtol=1e-13)
        assert G.same_bits(G.norm_ref(x2, mean, scale), ((x2.astype(np.float64) - mean) * scale).astype(np.float32))


def test_float64_scan_is_within_one_ulp_of_long_double():
    """Measured on x86-64 (80-bit long double), 14,463,120 elements: 21,766 (0.15 %) differ, all by 1 ulp, none by
    more, none excused by the floor."""
    total = differ = worst = floored = 0
    for (T, E, cols) in CPU_SHAPES:
        val, rews = G.inputs(T, E, cols)
        for (gamma, lam, dk, ls, rk) in G.settings():
            done = G.dones(dk, T)
            floor = G.float64_floor(T, rews[rk], val)
            lo = G.scan_ref32(rews[rk], val, done, gamma, lam, ls)
            hi = G.scan_ref32(rews[rk], val, done, gamma, lam, ls, dtype=np.longdouble)
            for a, b in zip(lo, hi):
                d = G.ulp_distance(a, b)
                far = d > 1
                close = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= floor
                assert not (far & ~close).any(), (T, E, cols, gamma, lam, dk, ls, rk, int(d.max()))
                total += d.size
                differ += int((d > 0).sum())
                floored += int(far.sum())
                worst = max(worst, int(d.max()))
    print(json.dumps({"gae_long_double": {"elements": total, "differ": differ, "share": differ / total,
                                          "max_ulp": worst, "excused_by_floor": floored}}))
    assert total > 5_000_000
