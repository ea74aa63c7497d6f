"""TEST INFRASTRUCTURE ONLY -- float64 restatement of the GAE scan's ABI contract (include/d2d_hip.h,
csrc/gae_kernels.hip), shared by tests/test_gae_scan_oracle_cpu.py and tests/test_gae_edges_gpu.py.

oracle/gae_oracle.py restates the reference's compute_gae / discount_rewards on the env-major CONCATENATED
sequence.  This file restates what the kernels promise instead: every env of a [T][E][cols] batch is an
independent sequence that starts at t = T-1 with gae = R = v_next = 0, whatever dones[T-1] says, and with
`last_shard` the one element (T-1, E-1, .) has adv = r - v and restarts gae at 0.  The two agree when
dones[T-1] = 1 (tests/test_gae_scan_oracle_cpu.py pins that); with dones[T-1] = 0 they do not, and the
kernels follow this file.

The expressions are written in the kernels' operation order (which is the reference's, ippo.py:92-116), one
IEEE operation per numpy call, so a kernel built without FMA contraction rounds every step as scan_ref does:
the GPU tests ask for bit equality, not closeness.  References are numpy loops over T only, vectorised over
E and cols.
"""
import numpy as np

# ---------------------------------------------------------------- the grid of tests/test_gae_edges_gpu.py
# (T, E, cols): T < U = 4 (the moments kernel's prefetch depth); every T % 4; E across a 256-thread block; cols 3
# and 5 leave dead column lanes at ct = 4 and 8; ct = 64 with a partial env block; ct = 256 with two column blocks;
# several env blocks; and two shapes with 258 partials per column (layout 0 resp. 1), so that
# gae_moments_reduce_kernel's stride loop runs with a ragged end.
SHAPES = [(1, 3, 2), (2, 5, 3), (3, 7, 1), (4, 2, 2), (5, 33, 5), (7, 257, 3), (8, 1, 1), (13, 5, 64), (6, 3, 300),
          (37, 300, 4), (5, 1030, 64), (3, 65800, 2)]
GAMMA_LAM = [(0.6, 0.97), (0.99, 0.95), (1.0, 1.0), (0.0, 0.5), (0.9, 0.0), (0.5, 1.0)]
DONE_KINDS = ["last", "none", "all", "alt", "bern"]
REWARD_KINDS = ["bcast", "percol"]
OFFSET = 1e4  # the large-offset column of the moments tests


def shape_id(s):
    return "T%d-E%d-c%d" % tuple(s)


def dones(kind, T):
    """uint8 [T]: last only / none / all / every second slot from t = 0 / Bernoulli(0.4), fixed seed."""
    d = np.zeros(T, dtype=np.uint8)
    if kind == "last":
        d[T - 1] = 1
    elif kind == "all":
        d[:] = 1
    elif kind == "alt":
        d[0::2] = 1
    elif kind == "bern":
        d[:] = np.random.default_rng(1234 + T).random(T) < 0.4
    elif kind != "none":
        raise ValueError(kind)
    return d


def inputs(T, E, cols, seed=0, offset_column=False):
    """values randn * 3 + 1 [T][E][cols]; rewards broadcast [T][E] integers 0..4 ("bcast") and per-column
    non-integer fp32 ("percol").  offset_column: the last reward column is OFFSET + randn, so with gamma = 0 the
    last column of adv and ret has offset 1e4 and unit spread (and a far larger spread at gamma > 0)."""
    rng = np.random.default_rng([seed, T, E, cols])
    val = (rng.standard_normal((T, E, cols)) * 3 + 1).astype(np.float32)
    bcast = rng.integers(0, 5, size=(T, E)).astype(np.float32)
    percol = (rng.random((T, E, cols)) * 4 + 0.1 * rng.standard_normal((T, E, cols))).astype(np.float32)
    if offset_column:
        percol[..., -1] = (OFFSET + rng.standard_normal((T, E))).astype(np.float32)
    return val, {"bcast": bcast, "percol": percol}


def settings():
    """every (gamma, lam, done kind, last_shard, reward kind) of the grid"""
    return [(g, l, dk, ls, rk) for (g, l) in GAMMA_LAM for dk in DONE_KINDS for ls in (0, 1) for rk in REWARD_KINDS]


# ---------------------------------------------------------------- the scan
def scan_ref(rew, val, done, gamma, lam, last_shard, dtype=np.float64):
    """Raw (adv, ret) [T][E][cols] in `dtype` (np.float64: the kernels' arithmetic; np.longdouble: the
    precision check).  rew [T][E] (broadcast over columns) or [T][E][cols]; val [T][E][cols]; done [T]."""
    v = np.asarray(val).astype(dtype)
    T, E, cols = v.shape
    r = np.asarray(rew).astype(dtype)
    if r.ndim == 2:
        r = np.broadcast_to(r[:, :, None], (T, E, cols))
    gamma, lam = dtype(gamma), dtype(lam)
    adv = np.empty((T, E, cols), dtype=dtype)
    ret = np.empty((T, E, cols), dtype=dtype)
    gae = np.zeros((E, cols), dtype=dtype)
    R = np.zeros((E, cols), dtype=dtype)
    v_next = np.zeros((E, cols), dtype=dtype)
    for t in range(T - 1, -1, -1):
        nd = dtype(0.0 if done[t] else 1.0)
        R = r[t] + R * gamma * nd
        delta = r[t] + gamma * v_next * nd - v[t]
        gae = delta + gamma * lam * nd * gae
        a = gae + v[t]
        if t == T - 1 and last_shard:
            a[E - 1] = r[t, E - 1] - v[t, E - 1]
            gae[E - 1] = 0
        adv[t] = a
        ret[t] = R
        v_next = v[t]
    return adv, ret


def scan_ref32(rew, val, done, gamma, lam, last_shard, dtype=np.float64):
    adv, ret = scan_ref(rew, val, done, gamma, lam, last_shard, dtype)
    return adv.astype(np.float32), ret.astype(np.float32)


def float64_floor(T, rew, val):
    """Absolute size below which a float64 recursion of T steps cannot be told from exact arithmetic: every step
    adds a rounding of at most 2^-53 times the running magnitude, the running magnitude is at most
    T (max|r| + 2 max|V|) (gamma = lam = 1: gae sums T deltas), so T steps leave at most
    T^2 2^-53 (max|r| + 2 max|V|); 2^-50 gives a factor 8 for the additions inside a step."""
    return float(T) ** 2 * 2.0 ** -50 * (float(np.abs(rew).max()) + 2 * float(np.abs(val).max()))


# ---------------------------------------------------------------- normalisation and statistics
def columns(x32):
    """[..., cols] -> contiguous float64 [cols][rows]: numpy sums a contiguous axis pairwise"""
    x = np.asarray(x32)
    return np.ascontiguousarray(x.reshape(-1, x.shape[-1]).T, dtype=np.float64)


def moments_ref(x32):
    """float64 two-pass (n, sum, M2 = sum of squared deviations from the mean) per column of x32 [..., cols]"""
    xc = columns(x32)
    n = xc.shape[1]
    s = xc.sum(1)
    m2 = ((xc - (s / n)[:, None]) ** 2).sum(1)
    return float(n), s, m2


def stats_ref(x32, ddof, n=None, moments=None):
    """float64 two-pass (mean, 1 / std, gate) per column of x32 [..., cols] as d2d_colstats_finalize defines them:
    mean = sum / n, std = sqrt(M2 / (n - ddof)), gate = every column's std > 0.  n defaults to the row count;
    moments: moments_ref(x32) if the caller has it already."""
    rows, s, m2 = moments_ref(x32) if moments is None else moments
    n = rows if n is None else float(n)
    mean = s / n
    if n != rows:
        m2 = ((columns(x32) - mean[:, None]) ** 2).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(m2 / (n - ddof))
        scale = 1.0 / sd
    return mean, scale, int(bool((sd > 0).all()))


def norm_ref(x32, mean, scale):
    """nrm of csrc/gae_kernels.hip: two float64 operations and one rounding, columns last"""
    return ((np.asarray(x32).astype(np.float64) - mean) * scale).astype(np.float32)


# ---------------------------------------------------------------- fp32 distances
def ulp_distance(a32, b32):
    """number of fp32 values between a and b (0 = the same bits up to the sign of zero), int64"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a32) - key(b32))


def same_bits(a32, b32):
    a = np.ascontiguousarray(a32, dtype=np.float32).view(np.uint32)
    b = np.ascontiguousarray(b32, dtype=np.float32).view(np.uint32)
    return a.shape == b.shape and bool((a == b).all())
