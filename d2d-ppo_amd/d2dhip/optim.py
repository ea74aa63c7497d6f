"""The optimizer step on the HIP kernel (C ABI d2d_adam_step, csrc/optim_kernels.hip): per-agent gradient-norm
clipping + Adam over agent-stacked tensors in one call.

Replaces torch.nn.utils.clip_grad_norm_ per agent + torch.optim.Adam.step() at its defaults (the reference's
ippo.py:204-215, d2d_ppo.py:209-212 and 443-446, irdqn.py:144-146).  The learners opt in with fused_optimizer=True;
their default is torch's Adam.
"""
import ctypes

import torch

from . import _lib

# the keys of torch.optim.Adam's param_groups this optimizer cannot honour unless they are at their defaults
_TORCH_DEFAULTS = {"weight_decay": 0, "amsgrad": False, "maximize": False, "decoupled_weight_decay": False}


class StackedAdam:
    """Adam (torch.optim.Adam's defaults: no amsgrad, no weight decay) over tensors whose leading axis is the agent
    axis, with torch.nn.utils.clip_grad_norm_(agent k's tensors, max_norm) per agent in front when max_norm is given.

    params: 1..16 contiguous fp32 CUDA tensors / nn.Parameters, [n_agents, ...] each; with n_agents = 1 (a plain
    nn.Module such as the central critic) whole tensors of any shape, one global norm.  Anything else: ValueError.
    State: exp_avg, exp_avg_sq per tensor and ONE device int64 step, so step() is capturable in torch.cuda.graph
    and replays advance the step.  state_dict() / load_state_dict() use torch.optim.Adam's layout."""

    def __init__(self, params, n_agents, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
        params = list(params)
        n_agents = int(n_agents)
        if n_agents < 1:
            raise ValueError(f"StackedAdam: n_agents {n_agents} < 1")
        if not 1 <= len(params) <= _lib.D2D_ADAM_MAX_TENSORS:
            raise ValueError(f"StackedAdam: {len(params)} tensors, the kernel's table holds 1..{_lib.D2D_ADAM_MAX_TENSORS}")
        for i, p in enumerate(params):
            self._check_tensor(p, f"params[{i}]")
            if n_agents > 1 and (p.dim() < 1 or p.shape[0] != n_agents):
                raise ValueError(f"StackedAdam: params[{i}] has shape {tuple(p.shape)}, its leading axis is not the "
                                 f"{n_agents} agents")
            if p.device != params[0].device:
                raise ValueError(f"StackedAdam: params[{i}] lives on {p.device}, params[0] on {params[0].device}")
        if not lr >= 0 or not eps >= 0 or not all(0 <= b < 1 for b in betas):
            raise ValueError(f"StackedAdam: lr {lr} and eps {eps} must be >= 0, betas {betas} in [0, 1)")
        self.params = params
        self.n_agents = n_agents
        self.max_norm = None if max_norm is None or max_norm <= 0 else float(max_norm)
        self.param_groups = [dict(params=params, lr=lr, betas=tuple(betas), eps=eps)]
        dev = params[0].device
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params]
        self.step_count = torch.zeros((), dtype=torch.int64, device=dev)
        self.grad_norm = torch.zeros(n_agents, dtype=torch.float32, device=dev) if self.max_norm else None
        d = self._desc = _lib.AdamDesc()
        d.n_agents, d.n_tensors = n_agents, len(params)
        for i, p in enumerate(params):
            t = d.tensors[i]
            t.param, t.exp_avg, t.exp_avg_sq = p.data_ptr(), self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr()
            t.grad = p.data_ptr()  # (a placeholder for the size query; step() sets the gradient's pointer)
            t.numel = p.numel() // n_agents
        d.max_norm = self.max_norm or 0.0
        d.step_dev = self.step_count.data_ptr()
        self._fill_scalars()
        need = int(_lib.load().d2d_adam_workspace(ctypes.byref(d)))
        if need < 0:
            _lib.check(-1, "d2d_adam_workspace")
        self._ws = torch.empty(need // 8, dtype=torch.float64, device=dev) if need else None

    @staticmethod
    def _check_tensor(p, what):
        if not isinstance(p, torch.Tensor):
            raise ValueError(f"StackedAdam: {what} is a {type(p).__name__}, not a tensor")
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"StackedAdam: {what} must be a contiguous fp32 CUDA tensor (got {p.dtype} on {p.device}, "
                             f"contiguous: {p.is_contiguous()})")

    def _fill_scalars(self):
        g, d = self.param_groups[0], self._desc
        d.lr, d.eps = float(g["lr"]), float(g["eps"])
        d.beta1, d.beta2 = float(g["betas"][0]), float(g["betas"][1])

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def step(self, grads=None):
        """One update from the tensors' .grad (or `grads`, one per tensor).  Returns the [n_agents] gradient norms
        before clipping (a buffer the next step overwrites) when max_norm is set, else None.  A missing gradient is
        an error, not a skipped tensor."""
        lib = _lib.require_gpu()
        d = self._desc
        for i, p in enumerate(self.params):
            g = p.grad if grads is None else grads[i]
            if g is None:
                raise ValueError(f"StackedAdam.step: params[{i}] has no gradient")
            self._check_tensor(g, f"the gradient of params[{i}]")
            if g.shape != p.shape or g.device != p.device:
                raise ValueError(f"StackedAdam.step: the gradient of params[{i}] has shape {tuple(g.shape)} on "
                                 f"{g.device}, the tensor {tuple(p.shape)} on {p.device}")
            d.tensors[i].grad = g.data_ptr()
        self._fill_scalars()  # (param_groups[0]['lr'] may be changed between steps, as with torch's optimizers)
        ws = self._ws
        _lib.check(lib.d2d_adam_step(ctypes.byref(d), None if ws is None else ws.data_ptr(),
                                     0 if ws is None else ws.numel() * 8,
                                     None if self.grad_norm is None else self.grad_norm.data_ptr(),
                                     _lib.stream_ptr()), "d2d_adam_step")
        return self.grad_norm

    # ------------------------------------------------------------ torch.optim.Adam's state layout
    @property
    def state(self):
        return {p: {"step": self.step_count, "exp_avg": m, "exp_avg_sq": v}
                for p, m, v in zip(self.params, self.exp_avg, self.exp_avg_sq)}

    def state_dict(self):
        """torch.optim.Adam's layout: state[i] = {step, exp_avg, exp_avg_sq} (step a CPU fp32 scalar, as torch keeps
        it), param_groups with the tensors' indices; it loads into a torch.optim.Adam over the same tensors."""
        g = self.param_groups[0]
        step = torch.tensor(float(self.step_count.item()), dtype=torch.float32)
        state = {i: {"step": step.clone(), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                 for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq))}
        group = dict(lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=0, amsgrad=False, maximize=False,
                     foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                     params=list(range(len(self.params))))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """From state_dict() or from a torch.optim.Adam over the same tensors (one param group, Adam's defaults for
        everything this optimizer does not have; tensors without state yet start from zero at step 0)."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError(f"StackedAdam.load_state_dict: expected one param group of {len(self.params)} tensors")
        g = groups[0]
        for key, default in _TORCH_DEFAULTS.items():
            if g.get(key, default) != default:
                raise ValueError(f"StackedAdam.load_state_dict: {key}={g[key]} is not supported")
        steps = set()
        with torch.no_grad():
            for i, idx in enumerate(g["params"]):
                st = sd["state"].get(idx)
                if st is None:
                    self.exp_avg[i].zero_()
                    self.exp_avg_sq[i].zero_()
                    steps.add(0)
                    continue
                if tuple(st["exp_avg"].shape) != tuple(self.params[i].shape):
                    raise ValueError(f"StackedAdam.load_state_dict: state {idx} has shape {tuple(st['exp_avg'].shape)}, "
                                     f"the tensor {tuple(self.params[i].shape)}")
                self.exp_avg[i].copy_(st["exp_avg"])          # in place: a captured graph keeps its pointers
                self.exp_avg_sq[i].copy_(st["exp_avg_sq"])
                steps.add(int(st["step"]))
            if len(steps) != 1:
                raise ValueError(f"StackedAdam.load_state_dict: the tensors are at different steps {sorted(steps)}")
            self.step_count.fill_(steps.pop())
        self.param_groups[0].update(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"])
        self._fill_scalars()
