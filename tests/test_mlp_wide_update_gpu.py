"""The wide PPO-update kernels (d2d_ppo_actor_grad_wide, d2d_ppo_critic_grad_wide; csrc/mlp_wide_kernels.hip
ppo_wide_grad_kernel: hidden 65..128 with obs_dim 32..63) against the float64 autograd oracle of tests/mlp_oracle.py,
by the criterion of tests/test_update_edges_gpu.py, whose references, guarded buffers and comparisons it
imports.  Per agent and tensor:

    |g - g64| <= envelope + max(2e-5, 4 excess32) max|g64[k]| + 1e-7

(envelope: the relu-flip envelope of ambiguous (sample, unit) pairs; excess32: torch fp32's own excess on the CPU).
Every launch writes interior views between sentinels with a workspace of exactly d2d_ppo_wide_workspace floats;
logp_old / weight / returns / values rotate through the three layouts the learners use ([T][E][N], [N][E*T]
env-major, strided); stats and values are held to the oracle; a second launch gives the same bits; the record (64-byte
rows) gives the bits of fp32 rows on integer obs.

Input sets (mlp_wide_cases.update_input_sets; tests/test_mlp_wide_cpu.py checks their conditioning): the eight shapes
at N = 5, T = 3, E = 45 as integer, fractional and record inputs (two of them with heterogeneous in_dims); the (T, E)
edges of mlp_oracle.UPD_TE at N in {1, 5} for two shapes; N = 256 at (25, 70) and (75, 9), modes "int" and "mixed",
where every wave takes several 16-sample tiles; a saturated case; empty batches.  d2dhip.update routes to the wide entry
points only for callers that pass wide=True, as the learners do: its default stays d2d_ppo_actor_grad's envelope
(tests/test_update_gpu.py::test_update_rejects_bad_shapes), and test_default_call_keeps_the_narrow_envelope holds both."""
import ctypes

import pytest

import mlp_oracle as O
import mlp_wide_cases as C
import test_update_edges_gpu as U
from test_update_edges_gpu import (BETA, CLIP, GUARD, LAYOUTS, SENT, _bits, _inputs_intact, check_actor, check_critic,
                                   lay_samples, lay_values, same_bits)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class Launch(U.Launch):
    """The outputs of one launch between sentinels, and the workspace: exactly d2d_ppo_wide_workspace floats."""

    def __init__(self, r, critic):
        from d2dhip import _lib
        lib = _lib.require_gpu()
        assert _lib.mlp_wide(r.F, r.H), "every shape of this file runs on the wide entry points"
        net = r.inp["critic" if critic else "actor"]
        self.bufs, self.grads = {}, {}
        for name, t in net.items():
            self.bufs[name], self.grads[name] = self._guarded(t.numel(), t.shape)
        self.bufs["stats"], self.stats = self._guarded(2 * r.N, (r.N, 2))
        self.need = int(lib.d2d_ppo_wide_workspace(r.N, r.T, r.E, r.F, r.H, 1 if critic else r.A))
        self.bufs["workspace"], self.ws = self._guarded(self.need, (self.need,))


def run_actor(r, fmt, lay=0, clip=CLIP, beta=BETA, scale=None):
    from d2dhip.update import actor_grads
    obuf, obs = r.dev(fmt)
    abuf, acts = r.dev("acts")
    lbuf, lo = lay_samples(r.inp["logp_old"], r.T, r.E, LAYOUTS[lay % 3])
    wbuf, w = lay_samples(r.inp["W"], r.T, r.E, LAYOUTS[(lay + 1) % 3])
    ins = {n: (b, _bits(b).clone()) for n, b in (("obs", obuf), ("actions", abuf), ("logp_old", lbuf), ("weight", wbuf))}
    L = Launch(r, False)
    actor_grads(r.dev("actor"), obs, acts, lo, w, r.kind, clip=clip, beta=beta, scale=scale, grads=L.grads,
                stats=L.stats, workspace=L, wide=True)
    out = L.finish()
    _inputs_intact(ins)
    return out


def run_critic(r, fmt, lay=0, scale=None, values=None):
    from d2dhip.update import critic_grads
    obuf, obs = r.dev(fmt)
    rbuf, R = lay_samples(r.inp["R"], r.T, r.E, LAYOUTS[lay % 3])
    ins = {n: (b, _bits(b).clone()) for n, b in (("obs", obuf), ("returns", rbuf))}
    L = Launch(r, True)
    if values is not None:
        vbuf, vview, sel = lay_values(r.N, r.T, r.E, values)
    critic_grads(r.dev("critic"), obs, R, scale=scale, grads=L.grads, stats=L.stats, workspace=L,
                 values=None if values is None else vview, wide=True)
    out = L.finish()
    _inputs_intact(ins)
    if values is not None:
        v = vview.contiguous().cpu()
        assert not bool((_bits(v) == SENT).any()) and not bool(v.isnan().any()), "values: a sample was never written"
        rest = vbuf.clone()
        rest[sel] = SENT
        assert bool((rest == SENT).all()), "values: written outside (t, e < E, k)"
        out["values"] = (v.view(r.N, r.E, r.T).permute(0, 2, 1) if values == "env" else v.permute(2, 0, 1)).reshape(r.N, r.B)
    return out


def actor_formats(r_int, r_frac, tag, lay=0, twice=True):
    """fp32 integer, fp32 fractional (r_frac, or None) and the record: each against the oracle and bit for bit equal
    on repeat; the record bit for bit the fp32 integer run"""
    a = run_actor(r_int, "f32", lay)
    check_actor(a, r_int, f"{tag} actor f32")
    b = run_actor(r_int, "rec", lay + 1)
    check_actor(b, r_int, f"{tag} actor rec")
    same_bits(a, b, f"{tag} actor: record against fp32 rows")
    if twice:
        same_bits(a, run_actor(r_int, "f32", lay + 2), f"{tag} actor f32: second run")
        same_bits(b, run_actor(r_int, "rec", lay), f"{tag} actor rec: second run")
    if r_frac is not None:
        c = run_actor(r_frac, "f32", lay + 2)
        check_actor(c, r_frac, f"{tag} actor frac")
        if twice:
            same_bits(c, run_actor(r_frac, "f32", lay), f"{tag} actor frac: second run")


def critic_formats(r_int, r_frac, tag, lay=0, twice=True):
    """the same for the critic; every checked run also writes values, and equals bit for bit a run that does not"""
    a = run_critic(r_int, "f32", lay, values="tne")
    check_critic(a, r_int, f"{tag} critic f32")
    b = run_critic(r_int, "rec", lay + 1, values="env")
    check_critic(b, r_int, f"{tag} critic rec")
    same_bits(a, b, f"{tag} critic: record against fp32 rows")
    plain = run_critic(r_int, "f32", lay + 2)
    same_bits(plain, {k: a[k] for k in plain}, f"{tag} critic f32: values = None")
    if twice:
        same_bits(plain, run_critic(r_int, "rec", lay), f"{tag} critic rec: values = None, second run")
    if r_frac is not None:
        c = run_critic(r_frac, "f32", lay + 2, values="env")
        check_critic(c, r_frac, f"{tag} critic frac")
        plain = run_critic(r_frac, "f32", lay)
        same_bits(plain, {k: c[k] for k in plain}, f"{tag} critic frac: values = None")


# ---- (a) the shape sweep

@pytest.mark.parametrize("shape", C.SHAPES, ids=C.IDS)
def test_shape_sweep(shape):
    dims = C.HET.get(shape)
    ri = U.Ref(shape=shape, dims=dims, mode="int", **O.UPD_SWEEP)
    rf = U.Ref(shape=shape, dims=dims, mode="frac", **O.UPD_SWEEP)
    lay = C.SHAPES.index(shape)
    actor_formats(ri, rf, C.SID(shape), lay)
    critic_formats(ri, rf, C.SID(shape), lay)


# ---- (b) batch edges

@pytest.mark.parametrize("T,E", O.UPD_TE, ids=[f"T{T}-E{E}" for T, E in O.UPD_TE])
@pytest.mark.parametrize("N", O.UPD_EDGE_N)
@pytest.mark.parametrize("shape", C.EDGE_SHAPES, ids=[C.SID(s) for s in C.EDGE_SHAPES])
def test_batch_edges(shape, N, T, E):
    r = U.Ref(shape=shape, N=N, T=T, E=E)
    tag = f"{C.SID(shape)} N{N} T{T} E{E}"
    actor_formats(r, None, tag, O.UPD_TE.index((T, E)), twice=False)
    critic_formats(r, None, tag, O.UPD_TE.index((T, E)), twice=False)


# ---- (c) several tiles per wave

def assert_several_tiles_per_wave(r, critic):
    """The grid rule (mlp_wide_cases.wide_blocks restates csrc/mlp_wide_kernels.hip): G workgroups of 4 waves per
    agent, wave w takes the 16-sample tiles w, w + 4 G, ...; the workspace is one partial of P floats per wave and
    agent, which exposes G.  With n_tiles >= 8 G every wave sums at least two tiles."""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    A = 1 if critic else r.A
    P = r.H * r.F + r.H + A * r.H + A + 2
    n_tiles = r.T * ((r.E + 15) // 16)
    G = C.wide_blocks(r.N, n_tiles)
    assert int(lib.d2d_ppo_wide_workspace(r.N, r.T, r.E, r.F, r.H, A)) == 4 * G * r.N * P
    assert n_tiles >= 8 * G, (n_tiles, G)


@pytest.mark.parametrize("shape,T,E,mode", C.TILE_CASES, ids=[f"{C.SID(s)}-T{T}-E{E}-{m}" for s, T, E, m in C.TILE_CASES])
def test_several_tiles_per_wave(shape, T, E, mode):
    r = U.Ref(shape=shape, N=C.TILE_N, T=T, E=E, mode=mode)
    tag = f"{C.SID(shape)} T{T} E{E} {mode}"
    if mode == "mixed":
        x = r.inp["obs"]
        assert bool((x != x.round()).any()), "fractional values"
    assert_several_tiles_per_wave(r, False)
    a = run_actor(r, "f32", 0)
    check_actor(a, r, f"{tag} actor f32")
    if mode == "int":
        same_bits(a, run_actor(r, "rec", 1), f"{tag} actor: record against fp32 rows")
    else:
        same_bits(a, run_actor(r, "f32", 2), f"{tag} actor f32: second run")
    assert_several_tiles_per_wave(r, True)
    c = run_critic(r, "f32", 2, values="tne")
    check_critic(c, r, f"{tag} critic f32")
    if mode == "int":
        d = run_critic(r, "rec", 0)
        same_bits(d, {k: c[k] for k in d}, f"{tag} critic: record (values = None) against fp32 rows")
    else:
        d = run_critic(r, "f32", 1, values="env")
        same_bits(d, c, f"{tag} critic f32: second run")


# ---- (d) the clamp, the opt-in, empty batches

def test_default_call_keeps_the_narrow_envelope():
    """actor_grads / critic_grads without wide=True refuse a wide shape as before, and write nothing"""
    from d2dhip.update import actor_grads, critic_grads
    r = U.Ref(shape=("comb", 40, 96, 3), N=2, T=1, E=8)
    _, obs = r.dev("f32")
    _, acts = r.dev("acts")
    _, lo = lay_samples(r.inp["logp_old"], r.T, r.E, "tne")
    L = Launch(r, False)
    with pytest.raises(NotImplementedError):
        actor_grads(r.dev("actor"), obs, acts, lo, lo, r.kind, grads=L.grads, stats=L.stats)
    Lc = Launch(r, True)
    with pytest.raises(NotImplementedError):
        critic_grads(r.dev("critic"), obs, lo, grads=Lc.grads, stats=Lc.stats)
    torch.cuda.synchronize()
    for launch in (L, Lc):
        for name, buf in launch.bufs.items():
            assert bool((buf == SENT).all()), f"{name}: written by a refused call"



@pytest.mark.parametrize("shape", C.SATURATED, ids=[C.SID(s) for s in C.SATURATED])
def test_saturated_probabilities(shape):
    """b2[:, 0] += 40: every sample's probabilities past action 0 are far below EPS = 2^-23, where the clamp stops the
    log-prob's gradient; held to the oracle with the same clamp under the same formula."""
    r = U.Ref(shape=shape, dims=C.HET.get(shape), saturated=True, **O.UPD_SWEEP)
    assert r.actor()[0]["probs"][..., 1:].max().item() < O.EPS
    actor_formats(r, None, f"saturated {C.SID(shape)}", 0)


@pytest.mark.parametrize("T,E,N", [(0, 45, 5), (3, 0, 5), (3, 45, 0), (0, 0, 0)])
@pytest.mark.parametrize("record", [False, True], ids=["f32", "rec"])
def test_empty_batches(T, E, N, record):
    """With no sample (T = 0 or E = 0) the outputs are all zero; with no agent (N = 0) there is no output.
    d2d_ppo_wide_workspace asks for 0 floats, and nothing outside the outputs is written."""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    F, H, A = 33, 65, 4                                        # N * P = 12,565 floats at N = 5
    assert lib.d2d_ppo_wide_workspace(N, T, E, F, H, A) == 0
    zeros = torch.zeros(65536, device="cuda")                  # stands for every input: never read
    p = ctypes.c_void_p(zeros.data_ptr())
    st = (ctypes.c_int64 * 3)(E * N, N, 1)
    for critic in (False, True):
        a = 1 if critic else A
        sizes = {"w1": N * H * F, "b1": N * H, "w2": N * a * H, "b2": N * a, "stats": N * 2, "workspace": 0, "values": 0}
        bufs = {k: torch.full((16384 + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda") for k in sizes}
        q = {k: ctypes.c_void_p(b[GUARD:].data_ptr()) for k, b in bufs.items()}
        desc = _lib.MlpDesc(N, E, F, H, a, 1, p, p, p, p, None, None, None, None, 0, 0)
        desc.obs_format = _lib.D2D_OBS_U8 if record else _lib.D2D_OBS_F32
        desc.obs_signed = p if record else None
        if critic:
            rc = lib.d2d_ppo_critic_grad_wide(desc, T, p, p, st, 1.0, q["w1"], q["b1"], q["w2"], q["b2"], q["stats"],
                                              q["workspace"], 0, q["values"], st, _lib.stream_ptr())
        else:
            rc = lib.d2d_ppo_actor_grad_wide(desc, T, p, p, p, st, p, st, 0.1, 0.05, 1.0, q["w1"], q["b1"], q["w2"],
                                             q["b2"], q["stats"], q["workspace"], 0, _lib.stream_ptr())
        assert rc == 0, lib.d2d_last_error()
        torch.cuda.synchronize()
        for k, b in bufs.items():
            n = sizes[k]
            assert bool((b[GUARD:GUARD + n] == 0).all()), f"{k}: not zero"
            rest = b.clone()
            rest[GUARD:GUARD + n] = SENT
            assert bool((rest == SENT).all()), f"{k}: written outside"
