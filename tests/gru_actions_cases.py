"""TEST INFRASTRUCTURE ONLY.  The input sets of the categorical GRU head with 17..32 ids (the second action tile of
csrc/gru_kernels.hip), shared by tests/test_gru_actions_cpu.py -- which asserts on the CPU the conditions that make
every GPU comparison strict -- and tests/test_gru_actions_gpu.py.  Everything else is tests/gru_oracle.py's: the case
tuple, the seeds, the observations, the float64 / float32 references.

The output layer is scaled by 0.15 instead of gru_oracle's 0.3: with 25..32 ids the wider logits push probabilities
below P_LO = 1e-3 in most seeds.  Each case names its seed bump (the first seed, from 0 up, that meets every condition
of tests/test_gru_actions_cpu.py at that scale)."""
import gru_oracle as O

OUT_SCALE = 0.15


def acase(F, H, A, bump=0, **kw):
    return O.case("softmax", F, H, A=A, **kw)._replace(bump=bump)


# (1) the instance matrix: A in {17 (one id in tile 1), 25 (a ragged lane group), 32 (a full tile)} x (H, F) reaching
# HT in {1, 2, 4} and IT in {1, 2, 3, 4}; the value = the seed bump
MATRIX_HF = ((64, 24), (50, 30), (16, 12), (32, 47), (64, 63))
MATRIX_A = (17, 25, 32)
MATRIX_BUMP = {(64, 24): (3, 0, 1), (50, 30): (0, 2, 3), (16, 12): (0, 0, 0), (32, 47): (0, 1, 0), (64, 63): (2, 0, 2)}
MATRIX = [acase(F, H, A, MATRIX_BUMP[(H, F)][j]) for (H, F) in MATRIX_HF for j, A in enumerate(MATRIX_A)]
# (2) the input branches: the categorical env's 1/n ACK column, fractional inputs everywhere
INPUTS = [acase(24, 64, 17, 0, frac="column"), acase(40, 50, 20, 0, frac="all")]
# (3) windows and batch edges: the driver's window (history_len 10), L = 1, the LDS padding table's last window, one env,
# a full tile, two tiles and one env
DRIVER = acase(24, 64, 17, 1, L=10, ep=12, T=12)
WINDOWS = [DRIVER, acase(30, 50, 17, 1, L=1), acase(30, 50, 32, 0, L=64, ep=6, T=6, E=3)]
BATCH = [acase(30, 50, 32, 0, E=1), acase(30, 50, 17, 0, E=16), acase(30, 50, 31, 0, E=33)]
# the sets of the slot-range, carried-state and workspace tests (members of the matrix)
A17, A32 = MATRIX[3], MATRIX[5]          # H = 50, F = 30 (HT = 4, IT = 2): A = 17 and A = 32
# the sampler against the host Philox: 200 envs, every slot of one launch (sample index = slot * E + env)
SAMPLER = [acase(30, 50, 17, 0, E=200, ep=5, T=5), acase(30, 50, 32, 0, E=200, ep=5, T=5)]
RNG = dict(seed=1234, env_base=77, rng_step=5)
CDF_EDGE = 1e-6             # u tot within this of a CDF entry: the id may fall either way


def all_cases():
    seen, out = set(), []
    for c in MATRIX + INPUTS + WINDOWS + BATCH:
        if O.cid(c) not in seen:
            seen.add(O.cid(c))
            out.append(c)
    return out


class Ref(O.Ref):
    """gru_oracle.Ref with the output layer scaled by OUT_SCALE"""

    def __init__(self, c):
        super().__init__(c)
        s = O.case_seed(c)
        self.p, self.dims = O.make_net(c.N, c.F, c.H, c.A, s, c.dims, out_scale=OUT_SCALE)


_REFS = {}


def ref(c):
    key = (O.cid(c), c.bump)
    if key not in _REFS:
        _REFS[key] = Ref(c)
    return _REFS[key]


def sampler_reference(r):
    """(ids [N][T * E], near [N][T * E]) of a sampling launch over all T unpadded slots with RNG: word 0 of the Philox
    block at counter (env_base + slot * E + env, agent, rng_step, stream 3 | 0); u = (w >> 8) 2^-24; the id =
    min(#{cdf <= u tot}, A - 1) on the float64 probabilities; near: u tot within CDF_EDGE of a CDF entry."""
    import numpy as np
    from oracle import philox
    c = r.c
    p = r.out(False).reshape(c.N, c.T * c.E, c.A).numpy()
    envs = np.arange(c.T * c.E, dtype=np.uint64) + np.uint64(RNG["env_base"])
    agents = np.arange(c.N, dtype=np.uint64)
    w = philox.words(envs[None, :], agents[:, None], RNG["rng_step"], 3, 1, RNG["seed"])[..., 0]
    u = (w >> np.uint64(8)).astype(np.float64) / 16777216.0
    cdf = np.cumsum(p, -1)
    ut = (u * cdf[..., -1])[..., None]
    ids = np.minimum((cdf <= ut).sum(-1), c.A - 1)
    return ids, (np.abs(ut - cdf) < CDF_EDGE).any(-1)
