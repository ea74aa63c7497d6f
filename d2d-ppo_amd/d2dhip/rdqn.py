"""Python entry to the iRDQN kernels (C ABI d2d_rdqn_q / d2d_rdqn_grad, csrc/rdqn_kernels.hip): the reference's
RNN Q-network (algorithms/irdqn.py:58-86) and DQN.act / DQN.train_step (irdqn.py:133-160) for every agent at once,
windows gathered in-kernel from an observation ring -- fp32 rows or the env kernel's compact record (record.ObsRecord,
the same floats at 32 bytes per agent row) -- and, for the acting loop, a hidden state carried from slot to slot
(CarryState) instead of the window's recompute."""
import ctypes

import torch

from . import _lib
from .gru import _Workspace
from .record import ObsRecord, obs_arg

NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w1", "b1", "w2", "b2", "w3", "b3")
MODE = {"greedy": _lib.D2D_RDQN_GREEDY, "eps": _lib.D2D_RDQN_EPS, "forced": _lib.D2D_RDQN_FORCED}
LOSS = {"huber": _lib.D2D_RDQN_HUBER, "mse": _lib.D2D_RDQN_MSE}
MAX_HIDDEN, MAX_OBS, MAX_OUT, MAX_WINDOW = 128, 63, 16, 256


def check_envelope(F, H, A, L=1):
    """The kernels' shape limits, raised before any launch (the library checks them again)."""
    if H > MAX_HIDDEN or F > MAX_OBS or A > MAX_OUT or L > MAX_WINDOW:
        raise NotImplementedError(f"iRDQN kernels support hidden <= {MAX_HIDDEN}, obs_dim + 1 <= {MAX_OBS + 1}, "
                                  f"n_out <= {MAX_OUT}, window length <= {MAX_WINDOW} (got hidden {H}, obs_dim {F}, "
                                  f"n_out {A}, window {L})")


def desc(params, ring, ring_episode=0, seed=0, env_base=0, rng_offset=None):
    """d2d_rdqn_desc of agent-stacked params (NAMES) and the obs ring [rows][E][N][F] (float32 tensor or ObsRecord)."""
    p = params
    N, threeH, F = p["w_ih"].shape
    H, A = threeH // 3, p["w3"].shape[1]
    check_envelope(F, H, A)
    for n in NAMES:
        if p[n].dtype != torch.float32 or not p[n].is_contiguous():
            raise ValueError("iRDQN params must be contiguous float32")
    if isinstance(ring, ObsRecord):
        if not ring.is_contiguous() or len(ring.shape) != 4 or ring.shape[2:] != (N, F):
            raise ValueError("the obs record ring must be contiguous, logical shape [rows][E][N][F]")
    elif ring.dtype != torch.float32 or not ring.is_contiguous() or ring.dim() != 4 or ring.shape[2:] != (N, F):
        raise ValueError("the obs ring must be contiguous float32 [rows][E][N][F]")
    return _lib.RdqnDesc(N, ring.shape[1], F, H, A, ring.shape[0], int(ring_episode), 0,
                         *(p[n].data_ptr() for n in NAMES), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_base),
                         None if rng_offset is None else rng_offset)


def _samples(samples):
    if samples.dtype != torch.int32 or not samples.is_contiguous() or samples.dim() != 2 or samples.shape[1] != 3:
        raise ValueError("samples must be contiguous int32 [B][3] (env, last, window length)")
    return samples


def mask_dtype(A):
    return torch.uint8 if A <= 8 else torch.int16


class CarryState:
    """The acting loop's hidden state between d2d_rdqn_q_ex launches (the hcarry scratch) and a tag of the launch
    that left it there: the ring (data_ptr, obs format, ring_episode), the parameters (data_ptrs and the sum of their
    _version counters: an in-place write bumps it), B, the samples tensor, and the launch's `row` and `window`.
    q_values(..., carry=state, row=r, window=S) carries in only when the tag shows that this launch extends the
    previous one by exactly one row -- same ring, parameters, B and samples tensor, row == previous row + 1,
    S == previous S + 1, S >= 2, row_shift 0 -- and otherwise recomputes the window; either way it re-tags.
    `row` / `window` describe EVERY sample of the launch (samples[:, 1] == row, samples[:, 2] == window: the wrapper
    cannot read the device triples), samples[:, 0] must not change between the launches, and neither may the ring rows
    of the previous window.  Writes the version counters do not see (through a `.data` alias of a parameter) need
    reset()."""

    def __init__(self):
        self.h = None
        self.tag = None
        self.samples = None          # kept alive, compared by identity
        self.carried = 0             # launches that carried in / recomputed (tests, tools)
        self.recomputed = 0

    def reset(self):
        """Forget the carried state: the next launch recomputes."""
        self.tag = None
        self.samples = None

    @staticmethod
    def _key(params, ring, ring_episode, B):
        fmt = _lib.D2D_OBS_U8 if isinstance(ring, ObsRecord) else _lib.D2D_OBS_F32
        return (ring.data_ptr(), fmt, int(ring_episode), int(B), tuple(params[n].data_ptr() for n in NAMES),
                sum(int(getattr(params[n], "_version", 0)) for n in NAMES))

    def advance(self, params, ring, samples, ring_episode, row_shift, row, window):
        """Tag this launch; returns whether it may carry in."""
        if row is None or window is None:
            raise ValueError("q_values with a CarryState needs row= and window= (those of every sample)")
        key = self._key(params, ring, ring_episode, samples.shape[0])
        row, window = int(row), int(window)
        ok = (self.tag is not None and self.h is not None and int(row_shift) == 0 and samples is self.samples
              and self.tag == (key, row - 1, window - 1) and window >= 2)
        # a launch with row_shift != 0 leaves no state a later launch may extend
        self.tag = (key, row, window) if int(row_shift) == 0 else None
        self.samples = samples
        if ok:
            self.carried += 1
        else:
            self.recomputed += 1
        return ok

    def buffer(self, lib, d, B, device):
        n = lib.d2d_rdqn_carry_floats(ctypes.byref(d), B)
        if n < 0:
            raise ValueError("d2d_rdqn_carry_floats refused the desc")
        if self.h is None or self.h.numel() != n or self.h.device != device:
            self.h = torch.zeros(max(int(n), 4), dtype=torch.float32, device=device)
            self.tag = None
        return self.h


def q_values(params, ring, samples, ring_episode=0, row_shift=0, mode="greedy", eps=0.0, ready=True,
             explore_mask=None, explore_action=None, rng_step=0, seed=0, env_base=0, rng_offset=None,
             want_q=True, want_qmax=True, want_action=True, out=None, eps_rows=None, carry=None, row=None,
             window=None):
    """Q-values of the windows samples [B][3] (device int32: env, last, length) for every agent.
    Returns (q [N][B][A], qmax [N][B], action [B][N] one-hot channel masks), None where not wanted.
    mode 'greedy' / 'eps' (Philox, eps or per-sample eps_rows float32 [B], ready) / 'forced' (explore_mask,
    explore_action uint8 [B][N]).  ring: float32 [rows][E][N][F] or an ObsRecord of that logical shape.
    carry: a CarryState with row / window, the last row and the window length of every sample (see CarryState)."""
    lib = _lib.require_gpu()
    d = desc(params, ring, ring_episode, seed, env_base, rng_offset)
    s = _samples(samples)
    B, N, A, dev = s.shape[0], d.n_agents, d.n_out, ring.device
    out = out or {}
    q = out.get("q") if want_q else None
    qmax = out.get("qmax") if want_qmax else None
    act = out.get("action") if want_action else None
    if want_q and q is None:
        q = torch.empty((N, B, A), dtype=torch.float32, device=dev)
    if want_qmax and qmax is None:
        qmax = torch.empty((N, B), dtype=torch.float32, device=dev)
    if want_action and act is None:
        act = torch.empty((B, N), dtype=mask_dtype(A), device=dev)
    for t in (explore_mask, explore_action):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (B, N)):
            raise ValueError("explore_mask / explore_action must be contiguous uint8 [B][N]")
    if eps_rows is not None and (eps_rows.dtype != torch.float32 or not eps_rows.is_contiguous()
                                 or tuple(eps_rows.shape) != (B,)):
        raise ValueError("eps_rows must be contiguous float32 [B]")
    obs_p, fmt, sgn = obs_arg(ring)
    hc, carry_in = None, 0
    if carry is not None and B > 0:
        hc = carry.buffer(lib, d, B, dev)                                   # may drop the tag (a new size)
        carry_in = 1 if carry.advance(params, ring, s, ring_episode, row_shift, row, window) else 0
    rc = lib.d2d_rdqn_q_ex(ctypes.byref(d), obs_p, fmt, sgn, s.data_ptr(), B, int(row_shift), MODE[mode], float(eps),
                           _lib.ptr(eps_rows), 1 if ready else 0, _lib.ptr(explore_mask), _lib.ptr(explore_action),
                           int(rng_step) & 0xFFFFFFFF, _lib.ptr(hc), carry_in, _lib.ptr(q), _lib.ptr(qmax),
                           _lib.ptr(act), _lib.stream_ptr())
    if rc != 0 and carry is not None:
        carry.reset()
    _lib.check(rc, "d2d_rdqn_q_ex")
    return q, qmax, act


_ws = _Workspace()


def grads(params, ring, samples, L, action, reward, done, qmax_target, gamma, loss="huber", ring_episode=0,
          grads=None, loss_out=None):
    """One TD update's gradients (what autograd leaves in .grad after DQN.train_step's backward) and loss [N]:
    windows of exactly L steps ending at samples[:, 1]; action [B][N] one-hot masks, reward [B][N] float32,
    done [B] uint8 / bool, qmax_target [N][B] float32.  ring: float32 or ObsRecord, as in q_values."""
    lib = _lib.require_gpu()
    if callable(loss) or loss not in LOSS:
        raise NotImplementedError("the iRDQN gradient kernel implements loss 'huber' and 'mse'")
    d = desc(params, ring, ring_episode)
    check_envelope(d.obs_dim, d.hidden, d.n_out, L)
    s = _samples(samples)
    B, N, dev = s.shape[0], d.n_agents, ring.device
    if done.dtype == torch.bool:
        done = done.view(torch.uint8)
    ok = (action.dtype == mask_dtype(d.n_out) and tuple(action.shape) == (B, N) and action.is_contiguous()
          and reward.dtype == torch.float32 and tuple(reward.shape) == (B, N) and reward.is_contiguous()
          and done.dtype == torch.uint8 and tuple(done.shape) == (B,) and done.is_contiguous()
          and qmax_target.dtype == torch.float32 and tuple(qmax_target.shape) == (N, B) and qmax_target.is_contiguous())
    if not ok:
        raise ValueError("action [B][N] masks, reward [B][N] float32, done [B] uint8, qmax_target [N][B] float32, "
                         "all contiguous")
    grads = grads if grads is not None else {n: torch.empty_like(params[n]) for n in NAMES}
    if loss_out is None:
        loss_out = torch.empty((N,), dtype=torch.float32, device=dev)
    ws = _ws.get(lib.d2d_rdqn_grad_workspace(ctypes.byref(d), B, int(L)), dev)
    obs_p, fmt, sgn = obs_arg(ring)
    rc = lib.d2d_rdqn_grad_ex(ctypes.byref(d), obs_p, fmt, sgn, s.data_ptr(), B, int(L), action.data_ptr(),
                              reward.data_ptr(), done.data_ptr(), qmax_target.data_ptr(), float(gamma), LOSS[loss],
                              *(grads[n].data_ptr() for n in NAMES), loss_out.data_ptr(), ws.data_ptr(), ws.numel(),
                              _lib.stream_ptr())
    _lib.check(rc, "d2d_rdqn_grad_ex")
    return grads, loss_out
