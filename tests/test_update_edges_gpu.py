"""The fused PPO-update kernels (csrc/update_kernels.hip: ppo_actor_grad_kernel<KC, HT, KIND, PAIR, U8, AFIX>,
ppo_critic_grad_t_kernel<KC, HT, U8>, ppo_critic_grad_kernel<KC, HT, U8>, update_reduce_kernel; ppo_epilogue.h) against
the float64 gradient oracle of tests/mlp_oracle.py, at every instance the dispatch can select and at the edges of the
per-wave tile loop.  Inputs come from mlp_oracle.update_inputs (CPU, a seed per case; nonzero biases);
tests/test_update_oracle_cpu.py pins the oracle to torch autograd and checks on the reference alone that every input
set is well conditioned.  Its worst figures over all input sets: ambiguous-pair share 9.8e-4 (one pair of the 1,024
of a one-agent, 16-sample set), units with an envelope 6.1 %, torch fp32's own excess over the envelope 4.0e-6 of
max|g64[k]| (caps 1e-3, 10 %, 2e-5).  The whole file takes 22 s on an MI355X (the slowest test 3.9 s).

Criterion, per agent k and tensor, elementwise: |g - g64| <= envelope + max(2e-5, 4 excess32) max|g64[k]| + 1e-7,
envelope = the relu-flip envelope (zero but for w1 / b1), excess32 = the float32 oracle's own excess over the envelope
on the CPU (the rule of test_grads_on_large_rollout_vs_float64, per agent).  Loss, entropy and surrogate sums: rtol 1e-5,
atol 1e-4 against float64.  w1 columns past an agent's in_dims are exactly zero; two runs of a case agree bit for bit;
on integer inputs the record run equals the fp32 run bit for bit.  Values: |v - v64| <= max(1e-5 |v64| + 1e-5,
2 |v32 - v64|), and the gradients and stats of that run are bitwise those of a run with values = None.

Every launch goes through Launch: obs is an interior view of a NaN-filled buffer (the record: 0xFF bytes); logp_old,
weight and returns are views into NaN-filled storage in three layouts ([T][E][N]; env-major [N][E*T]; the
permute(1, 2, 0) of an [N][T][E + 3] tensor cut to E, whose samples past E are NaN inside the tensor's extent); every
gradient tensor, stats and the actions sit between sentinels (float bits 0x7FC0A5A5); the workspace is exactly
d2d_ppo_workspace(...) floats inside a sentinel-filled buffer; values is a strided view of a sentinel-filled buffer that
covers every env of the last 32-env tile.  Afterwards every input is bit-intact, every sentinel outside the outputs is
intact, and no sentinel is left inside an output.

Kernel instances and the cases that run them (KC = 2 when F + 1 > 32; HT = 2 / 4 / 8 for H <= 32 / 64 / 128; fp32 rows
and the record, U8, are two instances each; on the record A == 8 is the AFIX = 8 instance, on fp32 rows the PAIR one):
  actor (KC, HT)  comb A < 8     comb A == 8    comb A > 8     chsel A < 8    chsel A == 8   chsel A > 8
    (1, 2)        F15-H32-A4     F5-H20-A8      F10-H16-A16    F2-H17-A2      F9-H16-A8      F7-H32-A12
    (1, 4)        F18-H40-A5     F30-H64-A8     F24-H48-A13    F12-H33-A4     F12-H33-A8     F20-H40-A11
    (1, 8)        F9-H80-A6      F22-H96-A8     F31-H128-A9    F31-H65-A5     F14-H120-A8    F23-H100-A16
    (2, 2)        F35-H24-A2     F63-H17-A8     F40-H30-A12    F47-H20-A3     F52-H32-A8     F33-H32-A10
    (2, 4)        F50-H50-A7     F38-H64-A8     F32-H33-A16    F36-H64-A4     F60-H36-A8     F46-H64-A9
  (test_instance_sweep: fp32 integer, fp32 fractional -- the !XE body -- and the record; also comb F1-H1-A1, F3-H32-A3)
  critic, hidden on rows ppo_critic_grad_t_kernel (1, 2), (1, 4), (2, 2), (2, 4): every shape of that (KC, HT) above,
  by default; critic, sample on rows ppo_critic_grad_kernel (1, 8): the (1, 8) shapes by default; (1, 2), (1, 4),
  (2, 2), (2, 4): the same shapes under D2D_OPT_CRITIC_GRAD_ROWS (test_instance_sweep, three formats each).
  Several tiles per wave, the TileStride carry and mixed exact / fractional tiles: test_several_tiles_per_wave and
  test_mixed_exact_and_fractional_tiles (mlp_oracle.UPD_TILE_CASES / UPD_MIXED_CASES), one actor shape per (KC, HT)
  and kind, both critic kernels per (KC, HT).

Kernel faults these tests found, all fixed in update_kernels.hip:
- ppo_actor_grad_kernel<2, 2, 1, true, true> (chsel, A < 8, the record, F >= 32, H <= 32; test_instance_sweep
  [chsel-F47-H20-A3]) returned dW1 and db1 of hidden units 16 .. 31, input columns 32 .. 47, up to 400 x max|g| off:
  the compiler had placed the first dW1 MFMA of that tile one VALU instruction behind the inline-asm v_pk_mul_lo_u16
  that writes the first dword of its A operand (two wait states are needed; the compiler pads no asm statement), so
  the MFMA read the dword's previous content.  The asm helpers' results now pass mfma_operand_pad (s_nop 1) before
  an MFMA reads them, in the actor and both critic kernels.
- With T = 0 or E = 0, d2d_ppo_actor_grad / d2d_ppo_critic_grad_values zeroed N * P floats of a workspace for which
  d2d_ppo_workspace asks 0 floats (a write past the caller's buffer); they now zero the outputs themselves.
- dW2 = relu(h)^T dZ ran on two-way bf16 splits as (h_h + h_m) z_h + h_h z_m, with zeros in the four k-slots beside z_m:
  at 17 samples whose terms cancel to a seventh of their absolute sum (test_batch_edges[chsel-F2-H17-A2-5-T1-E17],
  agent 3) the dropped h_m z_m term and the split residuals left dW2 at 3.0e-5 of max|g64[k]|, over the bar.  The
  slots now carry z_m, (h_h + h_m)(z_h + z_m), in the same two MFMAs: 1.8e-5 there.  w2 stays the tensor nearest the
  bar (1.9e-5 at the same shape, T2 E64; the critic's b1 1.8e-5 at T3 E1): what remains is the residual of the
  two-way splits, <= 2 x 2^-18 of every |h z| term."""
import ctypes
import functools

import pytest

import mlp_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 256                 # sentinel elements on each side of every output
OBS_PAD = 256               # NaN floats (record: 0xFF bytes) on each side of the obs
SENT = 0x7FC0A5A5           # a NaN that no arithmetic produces
CLIP, BETA = 0.1, 0.05
LAYOUTS = ("tne", "env", "strided")
SID = lambda s: f"{s[0]}-F{s[1]}-H{s[2]}-A{s[3]}"  # noqa: E731


def kc_ht(shape):
    _, F, H, _ = shape
    ht = (H + 15) // 16
    return (1 if F + 1 <= 32 else 2), (2 if ht <= 2 else 4 if ht <= 4 else 8)


@pytest.fixture
def rows_option():
    """sets D2D_OPT_CRITIC_GRAD_ROWS on request and restores the default"""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    yield lambda on: lib.d2d_set_option(_lib.D2D_OPT_CRITIC_GRAD_ROWS, 1 if on else 0)
    lib.d2d_set_option(_lib.D2D_OPT_CRITIC_GRAD_ROWS, 0)


# ---- the reference, computed once per input set and shared (never modified)

class Ref:
    def __init__(self, **kw):
        self.inp = O.update_inputs(**kw)
        i = self.inp
        self.kind, self.F, self.H, self.A = i["shape"]
        self.N, self.T, self.E, self.B = i["N"], i["T"], i["E"], i["T"] * i["E"]
        self.obs_flat = i["obs"].view(self.B, self.N, self.F)
        self._cache = {}
        self._dev = {}

    @staticmethod
    def _excess(r64, r32):
        return {n: O.grad_excess(r32["grads"][n], r64["grads"][n], r64["env"][n]) for n in r64["grads"]}

    def actor(self, clip=CLIP, beta=BETA, scale=None):
        """(float64 oracle, torch-fp32 excess per tensor [N]) of the actor loss"""
        scale = 1.0 / self.B if scale is None else scale
        key = ("actor", clip, beta, scale)
        if key not in self._cache:
            i = self.inp
            args = (i["actor"], self.obs_flat, self.kind, i["acts"], i["logp_old"], i["W"], clip, beta, scale)
            r64 = O.actor_grad_oracle(*args)
            self._cache[key] = (r64, self._excess(r64, O.actor_grad_oracle(*args, torch.float32)))
        return self._cache[key]

    def critic(self, scale=None):
        """(float64 oracle, excess32, |v32 - v64|) of the critic loss"""
        scale = 1.0 / self.B if scale is None else scale
        key = ("critic", scale)
        if key not in self._cache:
            i = self.inp
            r64 = O.critic_grad_oracle(i["critic"], self.obs_flat, i["R"], scale)
            r32 = O.critic_grad_oracle(i["critic"], self.obs_flat, i["R"], scale, torch.float32)
            self._cache[key] = (r64, self._excess(r64, r32), (r32["v"].double() - r64["v"]).abs())
        return self._cache[key]

    def dev(self, what):
        """device copies shared by the runs of this input set: the nets, the obs in both formats, the actions"""
        if what not in self._dev:
            i = self.inp
            if what in ("actor", "critic"):
                self._dev[what] = {k: v.cuda().contiguous() for k, v in i[what].items()}
            elif what == "f32":
                self._dev[what] = pad_obs(i["obs"])
            elif what == "rec":
                self._dev[what] = pad_record(i["obs"])
            elif what == "acts":
                self._dev[what] = pad_actions(self)
        return self._dev[what]


@functools.lru_cache(maxsize=2)
def _ref(shape, N, T, E, dims, mode, saturated):
    return Ref(shape=shape, N=N, T=T, E=E, dims=None if dims is None else list(dims), mode=mode, saturated=saturated)


def ref(shape, N, T, E, dims=None, mode="int", saturated=False):
    return _ref(shape, N, T, E, None if dims is None else tuple(dims), mode, saturated)


# ---- guarded buffers

def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def pad_obs(obs):
    n = obs.numel()
    buf = torch.full((n + 2 * OBS_PAD,), float("nan"), device="cuda")
    view = buf[OBS_PAD:OBS_PAD + n].view(obs.shape)
    view.copy_(obs)
    return buf, view


def pad_record(obs):
    from d2dhip.record import ObsRecord
    rec = O.to_record(obs)
    n = rec.data.numel()
    buf = torch.full((n + 2 * OBS_PAD,), 0xFF, dtype=torch.uint8, device="cuda")
    view = buf[OBS_PAD:OBS_PAD + n].view(rec.data.shape)
    view.copy_(rec.data)
    return buf, ObsRecord(view, rec.obs_dim, rec.signed)


def pad_actions(r):
    """the kernel's [T][E][N] masks / ids between 0xFF bytes"""
    from d2dhip.envbatch import pack_masks_torch
    acts = r.inp["acts"]
    if r.kind == "comb":
        a = pack_masks_torch(acts.view(r.N, r.T, r.E, r.A).permute(1, 2, 0, 3)).contiguous()
    else:
        a = acts.view(r.N, r.T, r.E).permute(1, 2, 0).to(torch.uint8).contiguous()
    raw = a.view(torch.uint8).reshape(-1)
    buf = torch.full((raw.numel() + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + raw.numel()].copy_(raw)
    return buf, buf[GUARD:GUARD + raw.numel()].view(a.dtype).view(a.shape)


def lay_samples(x, T, E, layout):
    """per-sample values [N][B] (b = t * E + e, CPU) as the kernel's argument in one of LAYOUTS -> (storage, view)"""
    N = x.shape[0]
    tne = x.view(N, T, E).permute(1, 2, 0)
    if layout == "strided":
        buf = torch.full((N, T, E + 3), float("nan"), device="cuda")
        view = buf[:, :, :E].permute(1, 2, 0)
        view.copy_(tne)
        return buf, view
    buf = torch.full((T * E * N + 2 * GUARD,), float("nan"), device="cuda")
    inner = buf[GUARD:GUARD + T * E * N]
    if layout == "tne":
        view = inner.view(T, E, N)
        view.copy_(tne)
    else:
        view = inner.view(N, E * T)                       # sample e * T + t
        view.copy_(x.view(N, T, E).permute(0, 2, 1).reshape(N, E * T))
    return buf, view


def lay_values(N, T, E, layout):
    """the values argument: a strided view of a sentinel-filled buffer that holds every env of the last 32-env tile,
    -> (storage int32, view float32, the view's positions in the storage)"""
    Ep = 32 * ((E + 31) // 32)
    if layout == "env":
        buf = torch.full((N, Ep * T + 5), SENT, dtype=torch.int32, device="cuda")
        sel = (slice(None), slice(0, E * T))
    else:
        buf = torch.full((T, Ep, N + 2), SENT, dtype=torch.int32, device="cuda")
        sel = (slice(None), slice(0, E), slice(1, N + 1))
    return buf, buf.view(torch.float32)[sel], sel


class Launch:
    """The outputs of one launch between sentinels, and the workspace: exactly d2d_ppo_workspace floats."""

    def __init__(self, r, critic):
        from d2dhip import _lib
        lib = _lib.require_gpu()
        net = r.inp["critic" if critic else "actor"]
        self.bufs, self.grads = {}, {}
        for name, t in net.items():
            self.bufs[name], self.grads[name] = self._guarded(t.numel(), t.shape)
        self.bufs["stats"], self.stats = self._guarded(2 * r.N, (r.N, 2))
        self.need = int(lib.d2d_ppo_workspace(r.N, r.T, r.E, r.F, r.H, 1 if critic else r.A))
        self.bufs["workspace"], self.ws = self._guarded(self.need, (self.need,))

    @staticmethod
    def _guarded(n, shape):
        buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda")
        return buf, buf[GUARD:GUARD + n].view(torch.float32).view(shape)

    def get(self, floats, device):
        assert floats == self.need
        return self.ws

    def finish(self):
        torch.cuda.synchronize()
        for name, buf in self.bufs.items():
            assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all()), f"{name}: written outside"
            if name != "workspace":
                assert not bool((buf[GUARD:-GUARD] == SENT).any()), f"{name}: an element was never written"
        out = {k: v.cpu() for k, v in self.grads.items()}
        out["stats"] = self.stats.cpu()
        for k, v in out.items():
            assert not bool(v.isnan().any()), f"{k}: NaN"
        return out


def _inputs_intact(pairs):
    for name, (buf, before) in pairs.items():
        assert torch.equal(_bits(buf), before), f"{name} was modified"


def run_actor(r, fmt, lay=0, clip=CLIP, beta=BETA, scale=None):
    """d2d_ppo_actor_grad on guarded buffers -> {w1, b1, w2, b2, stats} (CPU).  lay: which layouts logp_old / weight
    take (rotating)."""
    from d2dhip.update import actor_grads
    obuf, obs = r.dev(fmt)
    abuf, acts = r.dev("acts")
    lbuf, lo = lay_samples(r.inp["logp_old"], r.T, r.E, LAYOUTS[lay % 3])
    wbuf, w = lay_samples(r.inp["W"], r.T, r.E, LAYOUTS[(lay + 1) % 3])
    ins = {n: (b, _bits(b).clone()) for n, b in (("obs", obuf), ("actions", abuf), ("logp_old", lbuf), ("weight", wbuf))}
    L = Launch(r, False)
    actor_grads(r.dev("actor"), obs, acts, lo, w, r.kind, clip=clip, beta=beta, scale=scale, grads=L.grads,
                stats=L.stats, workspace=L)
    out = L.finish()
    _inputs_intact(ins)
    return out


def run_critic(r, fmt, lay=0, scale=None, values=None):
    """d2d_ppo_critic_grad_values on guarded buffers -> {w1, b1, w2, b2, stats[, values [N][B]]} (CPU).
    values: None or a layout of lay_values."""
    from d2dhip.update import critic_grads
    obuf, obs = r.dev(fmt)
    rbuf, R = lay_samples(r.inp["R"], r.T, r.E, LAYOUTS[lay % 3])
    ins = {n: (b, _bits(b).clone()) for n, b in (("obs", obuf), ("returns", rbuf))}
    L = Launch(r, True)
    if values is not None:
        vbuf, vview, sel = lay_values(r.N, r.T, r.E, values)
    critic_grads(r.dev("critic"), obs, R, scale=scale, grads=L.grads, stats=L.stats, workspace=L,
                 values=None if values is None else vview)
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


# ---- comparisons

def same_bits(a, b, what):
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs"


def check_grads(got, r64, exc32, dims, tag):
    line = []
    for name, g64 in r64["grads"].items():
        N = g64.shape[0]
        one = (N,) + (1,) * (g64.dim() - 1)
        top = g64.abs().reshape(N, -1).max(1).values
        band = torch.maximum(torch.full_like(top, 2e-5), 4 * exc32[name])
        err = (got[name].double() - g64).abs()
        over = (err - r64["env"][name]).clamp(min=0).reshape(N, -1).max(1).values
        k = int((over / top.clamp(min=1e-300) * (top > 0)).argmax())
        line.append(f"{name} {over[k].item() / max(top[k].item(), 1e-300):.1e} of max|g64| {top[k].item():.1e} (agent {k}, "
                    f"band {band[k].item():.1e})")
        bad = err > r64["env"][name] + (band * top).view(one) + 1e-7
        assert not bool(bad.any()), (tag, name, int(bad.sum()), err[bad].max().item(), line[-1])
    print(f"GRAD {tag}: " + "; ".join(line))
    for k, d in enumerate(dims or []):
        assert bool((got["w1"][k, :, d:] == 0).all()), (tag, "w1 columns past in_dims", k)


def check_actor(got, r, tag, **kw):
    r64, exc32 = r.actor(**kw)
    check_grads(got, r64, exc32, r.inp["dims"], tag)
    st = got["stats"].double()
    assert torch.allclose(st[:, 0], r64["surr"], rtol=1e-5, atol=1e-4), (tag, "surrogate", st[:, 0], r64["surr"])
    assert torch.allclose(st[:, 1], r64["ent"], rtol=1e-5, atol=1e-4), (tag, "entropy", st[:, 1], r64["ent"])


def check_critic(got, r, tag, **kw):
    r64, exc32, v_band = r.critic(**kw)
    check_grads(got, r64, exc32, r.inp["dims"], tag)
    st = got["stats"].double()
    assert torch.allclose(st[:, 0], r64["loss"], rtol=1e-5, atol=1e-4), (tag, "loss", st[:, 0], r64["loss"])
    assert bool((got["stats"][:, 1] == 0).all())
    if "values" in got:
        err = (got["values"].double() - r64["v"]).abs()
        bad = err > torch.maximum(1e-5 * r64["v"].abs() + 1e-5, 2 * v_band)
        assert not bool(bad.any()), (tag, "values", int(bad.sum()), err[bad].max().item())


def actor_formats(r_int, r_frac, tag, lay=0, twice=True, **kw):
    """fp32 integer, fp32 fractional (r_frac, or None) and the record: each against the oracle and bit for bit equal
    on repeat; the record bit for bit the fp32 integer run"""
    a = run_actor(r_int, "f32", lay, **kw)
    check_actor(a, r_int, f"{tag} actor f32", **kw)
    b = run_actor(r_int, "rec", lay + 1, **kw)
    check_actor(b, r_int, f"{tag} actor rec", **kw)
    same_bits(a, b, f"{tag} actor: record against fp32 rows")
    if twice:
        same_bits(a, run_actor(r_int, "f32", lay + 2, **kw), f"{tag} actor f32: second run")
        same_bits(b, run_actor(r_int, "rec", lay, **kw), f"{tag} actor rec: second run")
    if r_frac is not None:
        c = run_actor(r_frac, "f32", lay + 2, **kw)
        check_actor(c, r_frac, f"{tag} actor frac", **kw)
        if twice:
            same_bits(c, run_actor(r_frac, "f32", lay, **kw), f"{tag} actor frac: second run")


def critic_formats(r_int, r_frac, tag, lay=0, twice=True, **kw):
    """the same for the critic; every checked run also writes values, and equals bit for bit a run that does not"""
    a = run_critic(r_int, "f32", lay, values="tne", **kw)
    check_critic(a, r_int, f"{tag} critic f32", **kw)
    b = run_critic(r_int, "rec", lay + 1, values="env", **kw)
    check_critic(b, r_int, f"{tag} critic rec", **kw)
    same_bits(a, b, f"{tag} critic: record against fp32 rows")
    plain = run_critic(r_int, "f32", lay + 2, **kw)
    same_bits(plain, {k: a[k] for k in plain}, f"{tag} critic f32: values = None")
    if twice:
        same_bits(plain, run_critic(r_int, "rec", lay, **kw), f"{tag} critic rec: values = None, second run")
    if r_frac is not None:
        c = run_critic(r_frac, "f32", lay + 2, values="env", **kw)
        check_critic(c, r_frac, f"{tag} critic frac", **kw)
        plain = run_critic(r_frac, "f32", lay, **kw)
        same_bits(plain, {k: c[k] for k in plain}, f"{tag} critic frac: values = None")


# ---- (a) the instance sweep

@pytest.mark.parametrize("shape", O.UPD_SHAPES, ids=[SID(s) for s in O.UPD_SHAPES])
def test_instance_sweep(shape, rows_option):
    dims = O.upd_dims(shape[1])
    ri = ref(shape, dims=dims, mode="int", **O.UPD_SWEEP)
    rf = Ref(shape=shape, dims=dims, mode="frac", **O.UPD_SWEEP)
    tag = SID(shape)
    lay = O.UPD_SHAPES.index(shape)
    actor_formats(ri, rf, tag, lay)
    critic_formats(ri, rf, tag, lay)
    if kc_ht(shape)[1] <= 4:
        rows_option(True)
        critic_formats(ri, rf, tag + " rows", lay + 1)


# ---- (b) batch edges and argument variants

@pytest.mark.parametrize("T,E", O.UPD_TE, ids=[f"T{T}-E{E}" for T, E in O.UPD_TE])
@pytest.mark.parametrize("N", O.UPD_EDGE_N)
@pytest.mark.parametrize("shape", O.UPD_EDGE_SHAPES, ids=[SID(s) for s in O.UPD_EDGE_SHAPES])
def test_batch_edges(shape, N, T, E):
    r = Ref(shape=shape, N=N, T=T, E=E)
    tag = f"{SID(shape)} N{N} T{T} E{E}"
    actor_formats(r, None, tag, O.UPD_TE.index((T, E)), twice=False)
    critic_formats(r, None, tag, O.UPD_TE.index((T, E)), twice=False)


@pytest.mark.parametrize("variant", ["beta0", "clip02", "scale"])
@pytest.mark.parametrize("shape", O.UPD_EDGE_SHAPES[:2], ids=[SID(s) for s in O.UPD_EDGE_SHAPES[:2]])
def test_argument_variants(shape, variant):
    r = ref(shape, 5, 5, 65)
    kw = {"beta0": dict(beta=0.0), "clip02": dict(clip=0.2), "scale": dict(scale=0.37 / r.B)}[variant]
    actor_formats(r, None, f"{SID(shape)} {variant}", 0, twice=False, **kw)
    base = run_actor(r, "f32")
    assert not torch.equal(base["w2"], run_actor(r, "f32", **kw)["w2"]), "the argument is ignored"
    if variant == "scale":
        critic_formats(r, None, f"{SID(shape)} {variant}", 1, twice=False, **kw)


# ---- (c) several tiles per wave, (d) mixed exact / fractional tiles

def tiles_per_wave_bound(r, critic):
    """G is not exposed: the workspace holds G_bound >= G partials of N * P floats, and a wave of the 4 G per agent
    computes at least two tiles when n_tiles >= 8 G_bound"""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    A = 1 if critic else r.A
    P = r.H * r.F + r.H + A * r.H + A + 2
    g_bound = int(lib.d2d_ppo_workspace(r.N, r.T, r.E, r.F, r.H, A)) // (r.N * P)
    n_tiles = r.T * ((r.E + 31) // 32)
    assert g_bound >= 1 and n_tiles >= 8 * g_bound, (n_tiles, g_bound)


def tile_case(r, tag, rows_option, record, critic=True):
    tiles_per_wave_bound(r, False)
    a = run_actor(r, "f32", 0)
    check_actor(a, r, f"{tag} actor f32")
    if record:
        same_bits(a, run_actor(r, "rec", 1), f"{tag} actor: record against fp32 rows")
    else:
        same_bits(a, run_actor(r, "f32", 2), f"{tag} actor f32: second run")
    if not critic:
        return
    tiles_per_wave_bound(r, True)
    for rows in ((False, True) if kc_ht(r.inp["shape"])[1] <= 4 else (False,)):
        rows_option(rows)
        t = f"{tag} critic{' rows' if rows else ''}"
        c = run_critic(r, "f32", 2, values="tne")
        check_critic(c, r, t + " f32")
        if record:
            d = run_critic(r, "rec", 0)
            same_bits(d, {k: c[k] for k in d}, t + ": record (values = None) against fp32 rows")


TILE_IDS = [f"{SID(s)}-T{T}-E{E}" for s, T, E in O.UPD_TILE_CASES]


@pytest.mark.parametrize("shape,T,E", O.UPD_TILE_CASES, ids=TILE_IDS)
def test_several_tiles_per_wave(shape, T, E, rows_option):
    """N = 256: G workgroups per agent is the kernel's occupancy (at most 8), so each wave walks its tiles with
    TileStride::next at a stride of 4 G tiles -- with tiles_per_t = 3 never a multiple of it, the carry branch -- and
    accumulates them.  The critics run on the comb shapes (one per (KC, HT))."""
    r = ref(shape, O.UPD_TILE_N, T, E)
    tile_case(r, f"{SID(shape)} T{T} E{E}", rows_option, record=True, critic=shape[0] == "comb")


MIXED_IDS = [f"{m}-{SID(s)}-T{T}-E{E}" for s, T, E, m in O.UPD_MIXED_CASES]


@pytest.mark.parametrize("shape,T,E,mode", O.UPD_MIXED_CASES, ids=MIXED_IDS)
def test_mixed_exact_and_fractional_tiles(shape, T, E, mode, rows_option):
    """fp32 rows where each (slot, 32-env tile, agent) is bf16-exact or not by a hash of its indices (mode "mixed":
    1 / n values; 1/2 and 1/4 stay on the exact body), or where one element of the last real sample of a ragged tile
    is the only inexact value ("single"): a wave skips the tile in its first pass and re-stages it in its second."""
    r = ref(shape, O.UPD_TILE_N, T, E, mode=mode)
    if mode == "mixed":
        f = O.fractional_tiles(T, E, r.N)
        assert 0.4 < f.double().mean().item() < 0.6
        x = r.inp["obs"]
        low = (x.view(torch.int32) & 0xFFFF) != 0                                   # bf16-inexact elements
        per_tile = torch.stack([low[:, 32 * j:32 * j + 32].any(1).any(-1) for j in range(f.shape[1])], 1)
        assert torch.equal(per_tile, f), "the inexact tiles are the hashed ones"
        assert bool(((x != x.round()) & ~low).any()), "bf16-exact non-integers"
    tile_case(r, f"{mode} {SID(shape)} T{T} E{E}", rows_option, record=False)


# ---- (e) the clamp, empty batches

@pytest.mark.parametrize("shape", O.UPD_SATURATED, ids=[SID(s) for s in O.UPD_SATURATED])
def test_saturated_probabilities(shape):
    """b2[:, 0] += 40: every sample's probabilities past action 0 are far below EPS = 2^-23, where the clamp stops the
    log-prob's gradient; held to the oracle with the same clamp under the same formula (the escape may act)."""
    dims = O.upd_dims(shape[1])
    r = ref(shape, dims=dims, saturated=True, **O.UPD_SWEEP)
    assert r.actor()[0]["probs"][..., 1:].max().item() < O.EPS
    actor_formats(r, None, f"saturated {SID(shape)}", 0)


@pytest.mark.parametrize("T,E,N", [(0, 45, 5), (3, 0, 5), (3, 45, 0), (0, 0, 0)])
@pytest.mark.parametrize("record", [False, True], ids=["f32", "rec"])
def test_empty_batches(T, E, N, record):
    """include/d2d_hip.h: the outputs are overwritten with the gradients of scale * a sum over T * n_envs samples.  With
    no sample (T = 0 or E = 0) they are all zero; with no agent (N = 0) there is no output.  d2d_ppo_workspace asks for
    0 floats, and nothing outside the outputs is written."""
    from d2dhip import _lib
    lib = _lib.require_gpu()
    F, H, A = 12, 33, 4                                       # N * P = 2,835 floats at N = 5
    assert lib.d2d_ppo_workspace(N, T, E, F, H, A) == 0
    zeros = torch.zeros(65536, device="cuda")                  # stands for every input: never read
    p = ctypes.c_void_p(zeros.data_ptr())
    st = (ctypes.c_int64 * 3)(E * N, N, 1)
    for critic in (False, True):
        a = 1 if critic else A
        sizes = {"w1": N * H * F, "b1": N * H, "w2": N * a * H, "b2": N * a, "stats": N * 2, "workspace": 0, "values": 0}
        bufs = {k: torch.full((4096 + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda") for k in sizes}
        q = {k: ctypes.c_void_p(b[GUARD:].data_ptr()) for k, b in bufs.items()}
        desc = _lib.MlpDesc(N, E, F, H, a, 1, p, p, p, p, None, None, None, None, 0, 0)
        desc.obs_format = _lib.D2D_OBS_U8 if record else _lib.D2D_OBS_F32
        desc.obs_signed = p if record else None
        if critic:
            rc = lib.d2d_ppo_critic_grad_values(desc, T, p, p, st, 1.0, q["w1"], q["b1"], q["w2"], q["b2"], q["stats"],
                                                q["workspace"], 0, q["values"], st, _lib.stream_ptr())
        else:
            rc = lib.d2d_ppo_actor_grad(desc, T, p, p, p, st, p, st, 0.1, 0.05, 1.0, q["w1"], q["b1"], q["w2"], q["b2"],
                                        q["stats"], q["workspace"], 0, _lib.stream_ptr())
        assert rc == 0, lib.d2d_last_error()
        torch.cuda.synchronize()
        for k, b in bufs.items():
            n = sizes[k]
            assert bool((b[GUARD:GUARD + n] == 0).all()), f"{k}: not zero"
            assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), f"{k}: written outside"
