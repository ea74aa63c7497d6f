"""The optimizer entry points (d2d_adam_step, d2d_adam_workspace; csrc/optim_kernels.hip) without a GPU: the float64
oracle of tests/optim_oracle.py against torch's own float64 Adam + clip_grad_norm_, the exports and struct layouts,
every argument refusal with its message (each check runs before any HIP call; the accepted calls use empty shapes, so
nothing is launched), and StackedAdam's refusals."""
import ctypes

import pytest
import torch

import optim_oracle as O


def test_oracle_is_torch_adam_with_clip_grad_norm_in_float64():
    """3 steps of torch.optim.Adam after clip_grad_norm_ per agent, float64 on the CPU, against the oracle carried
    from step to step: 1e-12 relative on every parameter, moment and norm, with and without clipping."""
    for name, N, max_norm, eps in (("mlp_tiny", 3, 0.5, 1e-8), ("rnn", 5, None, 1.5e-4), ("critic", 1, 20.0, 1e-8),
                                   ("rdqn", 3, 2.0, 1.5e-4)):
        shapes = O.tensor_shapes(name, N)
        p0, _, _, _ = O.random_state(shapes, 7)
        params = [torch.nn.Parameter(x.double().clone()) for x in p0]
        opt = torch.optim.Adam(params, lr=3e-3, eps=eps)
        p = [x.double() for x in p0]
        m = [torch.zeros_like(x) for x in p]
        v = [torch.zeros_like(x) for x in p]
        for t in (1, 2, 3):
            g = [x.double() * 10 ** (t - 2) for x in O.random_state(shapes, 100 + t)[1]]
            for prm, gi in zip(params, g):
                prm.grad = gi.clone()
            norms = []
            if max_norm is not None:
                for k in range(N):  # per agent: the views share the gradients' storage, so the clip is in place
                    views = [prm.detach()[k] if N > 1 else prm for prm in params]
                    for vw, prm in zip(views, params):
                        vw.grad = prm.grad[k] if N > 1 else prm.grad
                    norms.append(torch.nn.utils.clip_grad_norm_(views, max_norm))
            opt.step()
            r = O.clip_adam64(p, g, m, v, N, t, lr=3e-3, eps=eps, max_norm=max_norm)
            close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)  # noqa: E731
            for i, prm in enumerate(params):
                st = opt.state[prm]
                assert close(r["p"][i], prm.detach()), (name, t, i)
                assert close(r["m"][i], st["exp_avg"]) and close(r["v"][i], st["exp_avg_sq"]), (name, t, i)
                if max_norm is not None:
                    assert close(r["g"][i], prm.grad), (name, t, i)
            if max_norm is not None:
                assert close(r["norm"], torch.stack(norms)), (name, t)
                assert (r["norm"] > max_norm).any() or t == 1
            p, m, v = r["p"], r["m"], r["v"]


def _calls():
    from d2dhip import _lib
    lib = _lib.load()
    w = 16

    def desc(N=0, n_tensors=4, numel=(15, 5, 10, 2), ptrs=(w, w, w, w), lr=1e-3, b1=0.9, b2=0.999, eps=1e-8,
             max_norm=0.0, step=1, step_dev=None):
        d = _lib.AdamDesc()
        d.n_agents, d.n_tensors = N, n_tensors
        for i in range(min(max(n_tensors, 0), 16)):
            t = d.tensors[i]
            t.param, t.grad, t.exp_avg, t.exp_avg_sq = ptrs
            t.numel = numel[i % len(numel)]
        d.lr, d.beta1, d.beta2, d.eps, d.max_norm, d.step, d.step_dev = lr, b1, b2, eps, max_norm, step, step_dev
        return d

    def step(d, ws=None, ws_bytes=0, norm=None):
        return lib.d2d_adam_step(ctypes.byref(d) if d is not None else None, ws, ws_bytes, norm, None)

    return _lib, lib, desc, step


def test_exports_and_struct_layouts():
    _lib, lib, desc, step = _calls()
    for name in ("d2d_adam_step", "d2d_adam_workspace"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.d2d_abi_version() == 15                                   # additions on top of ABI v15
    assert _lib.D2D_ADAM_MAX_TENSORS == 16
    assert ctypes.sizeof(_lib.AdamTensor) == 4 * 8 + 8
    assert ctypes.sizeof(_lib.AdamDesc) == 2 * 4 + 16 * 40 + 5 * 8 + 8 + 8
    assert _lib.AdamDesc.tensors.offset == 8 and _lib.AdamDesc.lr.offset == 8 + 16 * 40
    from conftest import ROOT
    import os
    txt = open(os.path.join(ROOT, "include", "d2d_hip.h")).read()
    assert "#define D2D_ADAM_MAX_TENSORS 16" in txt


def test_empty_shapes_are_accepted_without_a_launch():
    _lib, lib, desc, step = _calls()
    assert step(desc(N=0)) == 0                                           # no agents
    assert step(desc(N=0, max_norm=20.0)) == 0
    assert step(desc(N=3, numel=(0,), ptrs=(None,) * 4)) == 0             # all numel = 0: the pointers may be NULL
    assert lib.d2d_adam_workspace(ctypes.byref(desc(N=0, max_norm=20.0))) == 0
    assert lib.d2d_adam_workspace(ctypes.byref(desc(N=3, numel=(0,), max_norm=20.0))) == 0


def test_workspace_size():
    """[n_agents][P] double partials + [n_agents] float coefficients, P = one partial per 4,096 elements of a slice;
    nothing without clipping."""
    _lib, lib, desc, step = _calls()
    ws = lambda **kw: lib.d2d_adam_workspace(ctypes.byref(desc(**kw)))  # noqa: E731
    assert ws(N=3) == 0 and ws(N=3, max_norm=-1.0) == 0
    assert ws(N=3, max_norm=20.0) == 3 * 4 * 8 + 3 * 4 + 4               # rounded up to 8 bytes
    assert ws(N=1, n_tensors=2, numel=(128 * 3848, 128), max_norm=20.0) == (121 + 1) * 8 + 8
    assert ws(N=64, n_tensors=1, numel=(4097,), max_norm=1.0) == 64 * 2 * 8 + 64 * 4


def test_entry_points_validate_arguments_without_gpu():
    _lib, lib, desc, step = _calls()
    err = lambda: lib.d2d_last_error()  # noqa: E731
    assert step(None) == -1 and b"NULL desc" in err()
    assert lib.d2d_adam_workspace(None) == -1 and b"NULL desc" in err()
    for n in (0, 17, -1):
        assert step(desc(n_tensors=n)) == -1 and b"n_tensors" in err() and b"[1, 16]" in err(), n
    assert step(desc(n_tensors=16)) == 0
    assert step(desc(N=-1)) == -1 and b"negative n_agents" in err()
    assert step(desc(numel=(15, -5))) == -1 and b"negative numel" in err()
    for missing in range(4):                                              # a NULL pointer of a non-empty tensor
        ptrs = [16, 16, 16, 16]
        ptrs[missing] = None
        assert step(desc(ptrs=tuple(ptrs))) == -1 and b"NULL" in err() and b"non-empty" in err(), missing
    assert step(desc(ptrs=(16, 18, 16, 16))) == -1 and b"4-byte aligned" in err()
    assert step(desc(step=0)) == -1 and b"step 0 < 1 without step_dev" in err()
    assert step(desc(step=-3)) == -1 and b"without step_dev" in err()
    assert step(desc(step=0, step_dev=16)) == 0                           # the device counter replaces it
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        assert step(desc(b1=bad)) == -1 and b"beta1" in err() and b"[0, 1)" in err(), bad
        assert step(desc(b2=bad)) == -1 and b"beta2" in err() and b"[0, 1)" in err(), bad
    assert step(desc(b1=0.0, b2=0.0)) == 0
    assert step(desc(eps=-1e-8)) == -1 and b"eps" in err() and b"< 0" in err()
    assert step(desc(lr=-1e-3)) == -1 and b"lr" in err() and b"< 0" in err()
    assert step(desc(lr=0.0, eps=0.0)) == 0
    # the workspace: refused before any launch, so real sizes with placeholder pointers are safe here
    d = desc(N=3, max_norm=20.0)
    need = lib.d2d_adam_workspace(ctypes.byref(d))
    assert need > 0
    assert step(d, ws=None, ws_bytes=need) == -1 and b"workspace" in err()
    assert step(d, ws=64, ws_bytes=need - 1) == -1 and b"workspace" in err() and b"too small" in err()
    assert step(d, ws=68, ws_bytes=need) == -1 and b"workspace" in err() and b"8-byte aligned" in err()
    # clipping runs one grid row per agent: more than 65,535 agents are refused by both entry points alike
    big = desc(N=65536, max_norm=20.0)
    assert step(big, ws=64, ws_bytes=1 << 40) == -2 and b"n_agents <= 65535" in err()
    assert lib.d2d_adam_workspace(ctypes.byref(big)) == -1 and b"n_agents <= 65535" in err()
    assert lib.d2d_adam_workspace(ctypes.byref(desc(N=65536))) == 0      # (no limit without clipping)
    # a refused desc has no workspace size
    assert lib.d2d_adam_workspace(ctypes.byref(desc(b1=1.0))) == -1 and b"beta1" in err()


def test_stacked_adam_refuses_what_the_kernel_cannot_take():
    from d2dhip.optim import StackedAdam
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    good = torch.zeros(3, 5, 4, device=dev)
    with pytest.raises(ValueError, match="contiguous fp32 CUDA"):
        StackedAdam([good.transpose(1, 2)], 3)                            # not contiguous
    with pytest.raises(ValueError, match="contiguous fp32 CUDA"):
        StackedAdam([good.double()], 3)                                   # not fp32
    with pytest.raises(ValueError, match="contiguous fp32 CUDA"):
        StackedAdam([torch.zeros(3, 5)], 3)                               # on the CPU
    with pytest.raises(ValueError, match="not a tensor"):
        StackedAdam([[1.0, 2.0]], 1)
    with pytest.raises(ValueError, match="1..16"):
        StackedAdam([], 3)
    with pytest.raises(ValueError, match="n_agents"):
        StackedAdam([good], 0)
    if dev == "cuda":
        with pytest.raises(ValueError, match="leading axis"):
            StackedAdam([good], 4)
        with pytest.raises(ValueError, match="betas"):
            StackedAdam([good], 3, betas=(0.9, 1.0))


def _torch_fp32_step(p, g, m, v, t, lr, eps):
    """One step of torch.optim.Adam in fp32 on the CPU from the given state (its state dict loaded at step t - 1)."""
    prm = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([prm], lr=lr, eps=eps)
    sd = opt.state_dict()
    sd["state"] = {0: {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}}
    opt.load_state_dict(sd)
    prm.grad = g.clone()
    opt.step()
    st = opt.state[prm]
    return dict(p=[prm.detach()], m=[st["exp_avg"]], v=[st["exp_avg_sq"]], g=[g], norm=None)


def test_the_p_bar_is_a_property_of_the_inputs_for_torch_as_well():
    """Why optim_oracle.random_state keeps |p| >= 0.05: on states where 0.9 m and 0.1 g nearly cancel, torch's own fp32
    Adam misses the bar |p' - p'64| <= 8u (|p'64| + |delta64|) once p is near zero (1e-5), with m' and v' inside their
    bars all the while, and meets it on the same moments and gradients with |p| in [0.05, 0.15].  The restriction of the
    GPU test's inputs is therefore one the bar needs of any fp32 formulation, not an allowance for the kernel."""
    gen = torch.Generator().manual_seed(5)
    n, t, lr, eps = 20000, 1000, 3e-3, 1e-8
    m = torch.randn(n, generator=gen) * 0.03
    g = -9.0 * m * (1 + 0.02 * torch.randn(n, generator=gen))          # 0.9 m + 0.1 g: a few percent of either term
    v = m * m + 0.001 * g * g                                           # |m| <= sqrt(v): a state Adam can reach
    sign = torch.randint(0, 2, (n,), generator=gen) * 2.0 - 1
    ratios = {}
    for name, p in (("near_zero", sign * 1e-5), ("away", sign * (0.05 + 0.1 * torch.rand(n, generator=gen)))):
        got = _torch_fp32_step(p, g, m, v, t, lr, eps)
        ref = O.clip_adam64([p], [g], [m], [v], 1, t, lr=lr, eps=eps)
        ratios[name] = O.one_step_ratios(got, ref, [m], [v])
    print(f"  torch fp32 on cancelling moments: {ratios}")
    assert ratios["near_zero"]["p"] > 1.0 and ratios["near_zero"]["m"] <= 1.0 and ratios["near_zero"]["v"] <= 1.0
    assert all(r <= 1.0 for r in ratios["away"].values())
