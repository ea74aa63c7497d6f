"""Python entry to the iRDQN kernels (C ABI d2d_rdqn_q / d2d_rdqn_grad, csrc/rdqn_kernels.hip): the reference's
RNN Q-network (algorithms/irdqn.py:58-86) and DQN.act / DQN.train_step (irdqn.py:133-160) for every agent at once,
windows gathered in-kernel from an fp32 observation ring."""
import ctypes

import torch

from . import _lib
from .gru import _Workspace

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
    """d2d_rdqn_desc of agent-stacked params (NAMES) and the obs ring [rows][E][N][F]."""
    p = params
    N, threeH, F = p["w_ih"].shape
    H, A = threeH // 3, p["w3"].shape[1]
    check_envelope(F, H, A)
    for n in NAMES:
        if p[n].dtype != torch.float32 or not p[n].is_contiguous():
            raise ValueError("iRDQN params must be contiguous float32")
    if ring.dtype != torch.float32 or not ring.is_contiguous() or ring.dim() != 4 or ring.shape[2:] != (N, F):
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


def q_values(params, ring, samples, ring_episode=0, row_shift=0, mode="greedy", eps=0.0, ready=True,
             explore_mask=None, explore_action=None, rng_step=0, seed=0, env_base=0, rng_offset=None,
             want_q=True, want_qmax=True, want_action=True, out=None, eps_rows=None):
    """Q-values of the windows samples [B][3] (device int32: env, last, length) for every agent.
    Returns (q [N][B][A], qmax [N][B], action [B][N] one-hot channel masks), None where not wanted.
    mode 'greedy' / 'eps' (Philox, eps or per-sample eps_rows float32 [B], ready) / 'forced' (explore_mask,
    explore_action uint8 [B][N])."""
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
    rc = lib.d2d_rdqn_q(ctypes.byref(d), ring.data_ptr(), s.data_ptr(), B, int(row_shift), MODE[mode], float(eps),
                        _lib.ptr(eps_rows), 1 if ready else 0, _lib.ptr(explore_mask), _lib.ptr(explore_action),
                        int(rng_step) & 0xFFFFFFFF, _lib.ptr(q), _lib.ptr(qmax), _lib.ptr(act), _lib.stream_ptr())
    _lib.check(rc, "d2d_rdqn_q")
    return q, qmax, act


_ws = _Workspace()


def grads(params, ring, samples, L, action, reward, done, qmax_target, gamma, loss="huber", ring_episode=0,
          grads=None, loss_out=None):
    """One TD update's gradients (what autograd leaves in .grad after DQN.train_step's backward) and loss [N]:
    windows of exactly L steps ending at samples[:, 1]; action [B][N] one-hot masks, reward [B][N] float32,
    done [B] uint8 / bool, qmax_target [N][B] float32."""
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
    rc = lib.d2d_rdqn_grad(ctypes.byref(d), ring.data_ptr(), s.data_ptr(), B, int(L), action.data_ptr(),
                           reward.data_ptr(), done.data_ptr(), qmax_target.data_ptr(), float(gamma), LOSS[loss],
                           *(grads[n].data_ptr() for n in NAMES), loss_out.data_ptr(), ws.data_ptr(), ws.numel(),
                           _lib.stream_ptr())
    _lib.check(rc, "d2d_rdqn_grad")
    return grads, loss_out
