"""The actor gradient for 17..32 action ids (d2d_ppo_actor_grad_actions; csrc/mlp_actions_kernels.hip
ppo_actions_grad_kernel, actions_reduce_kernel) against the float64 autograd oracle of tests/mlp_oracle.py, by the
criterion of tests/test_update_edges_gpu.py, whose guarded buffers and comparisons it imports.  Per agent
and tensor (w1, b1, w2, b2):

    |g - g64| <= envelope + max(2e-5, 4 excess32) max|g64[k]| + 1e-7

(envelope: the relu-flip envelope of ambiguous (sample, unit) pairs; excess32: torch fp32's own excess on the CPU).
Every launch writes interior views between sentinels with a workspace of exactly d2d_ppo_actions_workspace floats --
which the test also holds to the restated grid rule --; logp_old / weight rotate through the three layouts the learners
use; stats are held to the oracle; w1 columns past an agent's in_dims are exactly zero; a second launch gives the same
bits.

Input sets (mlp_actions_cases.update_input_sets; tests/test_mlp_actions_cpu.py checks their conditioning, and that
every id -- 16 and A - 1 included -- is used): the nine shapes at N = 5, T = 3, E = 45 on integer and fractional inputs
(heterogeneous in_dims); the (T, E) edges of mlp_oracle.UPD_TE at N in {1, 5} for two shapes; N = 256 at (25, 70),
where by the grid rule G = 1 and each of the 4 waves sums 31 or 32 tiles; clips 0.1 and 0.2; empty batches."""
import ctypes

import pytest

import mlp_actions_cases as C
import mlp_oracle as O
import test_update_edges_gpu as U
from test_update_edges_gpu import (BETA, CLIP, GUARD, LAYOUTS, SENT, _bits, _inputs_intact, check_actor, lay_samples,
                                   same_bits)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class Ref(U.Ref):
    """test_update_edges_gpu.Ref on the input sets of mlp_actions_cases"""

    def __init__(self, **kw):
        self.inp = C.update_inputs(**kw)
        i = self.inp
        self.kind, self.F, self.H, self.A = i["shape"]
        self.N, self.T, self.E, self.B = i["N"], i["T"], i["E"], i["T"] * i["E"]
        self.obs_flat = i["obs"].view(self.B, self.N, self.F)
        self._cache = {}
        self._dev = {}


class Launch(U.Launch):
    """The outputs of one launch between sentinels, and the workspace: exactly d2d_ppo_actions_workspace floats,
    which equal the restated grid rule."""

    def __init__(self, r):
        from d2dhip import _lib
        lib = _lib.require_gpu()
        assert _lib.mlp_actions(r.F, r.H, r.A, 1), "every shape of this file runs on the new entry points"
        self.bufs, self.grads = {}, {}
        for name, t in r.inp["actor"].items():
            self.bufs[name], self.grads[name] = self._guarded(t.numel(), t.shape)
        self.bufs["stats"], self.stats = self._guarded(2 * r.N, (r.N, 2))
        self.need = int(lib.d2d_ppo_actions_workspace(r.N, r.T, r.E, r.F, r.H, r.A))
        assert self.need == C.workspace_floats(r.N, r.T, r.E, r.F, r.H, r.A)
        self.bufs["workspace"], self.ws = self._guarded(self.need, (self.need,))


def run_actor(r, lay=0, clip=CLIP, beta=BETA, scale=None):
    from d2dhip.update import actor_grads
    obuf, obs = r.dev("f32")
    abuf, acts = r.dev("acts")
    assert acts.dtype == torch.uint8
    lbuf, lo = lay_samples(r.inp["logp_old"], r.T, r.E, LAYOUTS[lay % 3])
    wbuf, w = lay_samples(r.inp["W"], r.T, r.E, LAYOUTS[(lay + 1) % 3])
    ins = {n: (b, _bits(b).clone()) for n, b in (("obs", obuf), ("actions", abuf), ("logp_old", lbuf), ("weight", wbuf))}
    L = Launch(r)
    actor_grads(r.dev("actor"), obs, acts, lo, w, r.kind, clip=clip, beta=beta, scale=scale, grads=L.grads,
                stats=L.stats, workspace=L)
    out = L.finish()
    _inputs_intact(ins)
    return out


def checked(r, tag, lay=0, twice=True, **kw):
    a = run_actor(r, lay, **kw)
    check_actor(a, r, f"{tag} actor", **kw)
    if twice:
        same_bits(a, run_actor(r, lay + 1, **kw), f"{tag} actor: second run")
    return a


@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_shape_sweep(shape):
    dims = C.sweep_dims(shape)
    lay = C.SHAPES.index(shape)
    for mode in ("int", "frac"):
        r = Ref(shape=shape, dims=dims, mode=mode, **C.SWEEP)
        ids = set(r.inp["acts"].reshape(-1).tolist())
        assert ids == set(range(shape[3])) and 16 in ids, "every id is used"
        checked(r, f"{C.SID(shape)} {mode}", lay)
        if mode == "int":
            checked(r, f"{C.SID(shape)} {mode} clip 0.2", lay + 1, twice=False, clip=0.2)


@pytest.mark.parametrize("T,E", O.UPD_TE, ids=[f"T{T}-E{E}" for T, E in O.UPD_TE])
@pytest.mark.parametrize("N", C.EDGE_N)
@pytest.mark.parametrize("shape", C.EDGE_SHAPES, ids=[C.SID(s) for s in C.EDGE_SHAPES])
def test_batch_edges(shape, N, T, E):
    r = Ref(shape=shape, N=N, T=T, E=E)
    checked(r, f"{C.SID(shape)} N{N} T{T} E{E}", O.UPD_TE.index((T, E)))


def test_several_tiles_per_wave():
    """N = 256: one workgroup per agent (G = 1 by the grid rule, which the workspace size exposes), so each of its 4
    waves sums n_tiles / 4 >= 31 tiles of mixed exact / fractional inputs"""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    shape, T, E, mode = C.TILE_CASE
    r = Ref(shape=shape, N=C.TILE_N, T=T, E=E, mode=mode)
    x = r.inp["obs"]
    assert bool((x != x.round()).any()), "fractional values"
    n_tiles = T * ((E + 15) // 16)
    P = r.H * r.F + r.H + r.A * r.H + r.A + 2
    G = C.actions_blocks(r.N, n_tiles)
    assert int(lib.d2d_ppo_actions_workspace(r.N, T, E, r.F, r.H, r.A)) == 4 * G * r.N * P
    assert G == 1 and n_tiles >= 8 * G, (n_tiles, G)
    checked(r, f"{C.SID(shape)} T{T} E{E} {mode}", 0)


@pytest.mark.parametrize("T,E,N", [(0, 45, 5), (3, 0, 5), (3, 45, 0), (0, 0, 0)])
def test_empty_batches(T, E, N):
    """With no sample (T = 0 or E = 0) the outputs are all zero; with no agent (N = 0) there is no output.
    d2d_ppo_actions_workspace asks for 0 floats, and nothing outside the outputs is written."""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    F, H, A = 24, 64, 17
    assert lib.d2d_ppo_actions_workspace(N, T, E, F, H, A) == 0
    zeros = torch.zeros(65536, device="cuda")                  # stands for every input: never read
    p = ctypes.c_void_p(zeros.data_ptr())
    st = (ctypes.c_int64 * 3)(E * N, N, 1)
    sizes = {"w1": N * H * F, "b1": N * H, "w2": N * A * H, "b2": N * A, "stats": N * 2, "workspace": 0}
    bufs = {k: torch.full((16384 + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda") for k in sizes}
    q = {k: ctypes.c_void_p(b[GUARD:].data_ptr()) for k, b in bufs.items()}
    desc = _lib.MlpDesc(N, E, F, H, A, 1, p, p, p, p, None, None, None, None, 0, 0)
    rc = lib.d2d_ppo_actor_grad_actions(desc, T, p, p, p, st, p, st, 0.1, 0.05, 1.0, q["w1"], q["b1"], q["w2"],
                                        q["b2"], q["stats"], q["workspace"], 0, _lib.stream_ptr())
    assert rc == 0, lib.d2d_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        n = sizes[k]
        assert bool((b[GUARD:GUARD + n] == 0).all()), f"{k}: not zero"
        rest = b.clone()
        rest[GUARD:GUARD + n] = SENT
        assert bool((rest == SENT).all()), f"{k}: written outside"
