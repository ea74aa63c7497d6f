"""The hand-written central-critic dW1 kernel (d2d_central_critic_dw1, csrc/critic_kernels.hip; VERDICT r05 "missing" 3):
dW1 = sum_b dpre_b x_b^T of D2D-PPO's Value network (/root/reference/algorithms/d2d_ppo.py:440-446, value_loss.backward()
into linear1.weight) from dpre's three RNE bf16 parts [B][3H] and the bf16 state operand [B][ldx], against float64 of
the same operands (the parts summed exactly; parts and states are exact bf16, so float64 is the exact sum): within
1e-6 of max|dW1| or twice torch fp32's own distance from float64 (the rounds 4-5 hipBLASLt path's level: fp32
accumulation over up to 10^5 samples), whichever is larger.  Ragged shapes: hidden sizes whose last 16-unit
tile is partial (20, 36, 100), state widths that are not a multiple of the column block (117 with ldx 120, 3,848),
sample counts that are not a multiple of the 32-sample step, fewer samples than one step, and B = 0 (zeros).  The
forward that makes dhm (d2d_central_critic_fwd), and forward -> dW1 against float64 autograd without a learner, are
tests/test_critic_fwd_gpu.py."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _dw1(H, B, S, ldx, xb, dhm):
    from d2dhip import _lib
    lib = _lib.require_gpu()
    n = int(lib.d2d_central_critic_dw1_workspace(H, B, S, ldx))
    assert n >= 0
    ws = torch.full((max(n, 1),), float("nan"), device="cuda")
    out = torch.full((H, S), float("nan"), device="cuda")
    _lib.check(lib.d2d_central_critic_dw1(H, B, S, ldx, xb.data_ptr() if B else None, dhm.data_ptr() if B else None,
                                          ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.stream_ptr()),
               "d2d_central_critic_dw1")
    torch.cuda.synchronize()
    return out


def _operands(H, B, S, ldx, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    xb = torch.zeros((max(B, 1), ldx), dtype=torch.bfloat16, device="cuda")
    xb[:, :S] = torch.randint(-1, 12, (max(B, 1), S), device="cuda", generator=g).to(torch.bfloat16)
    dp = torch.randn((max(B, 1), H), device="cuda", generator=g) * torch.rand((max(B, 1), 1), device="cuda", generator=g)
    dp[torch.rand(dp.shape, device="cuda", generator=g) < 0.4] = 0  # relu-masked units
    h = dp.to(torch.bfloat16)
    m = (dp - h.float()).to(torch.bfloat16)
    lo = (dp - h.float() - m.float()).to(torch.bfloat16)
    dhm = torch.cat([h, m, lo], 1).contiguous()
    return xb, dhm


@pytest.mark.parametrize("H,B,S,ldx", [(64, 98_311, 3848, 3848), (64, 100_000, 248, 248), (128, 40_003, 968, 968),
                                       (32, 5_000, 128, 128), (20, 33_333, 117, 120), (36, 4_097, 248, 256),
                                       (100, 9_001, 488, 488), (64, 31, 1928, 1928), (16, 1, 24, 24)])
def test_dw1_matches_float64(H, B, S, ldx):
    xb, dhm = _operands(H, B, S, ldx, seed=H + S)
    got = _dw1(H, B, S, ldx, xb, dhm)
    parts = dhm.double().view(B, 3, H).sum(1)                                    # dpre exactly
    ref = parts.t() @ xb.double()[:, :S]                                          # [H][S]
    err = (got.double() - ref).abs().max().item()
    t32 = (dhm.float().view(B, 3, H).sum(1).t() @ xb.float()[:, :S]).double()
    err32 = (t32 - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"H {H} B {B} S {S}: max err {err:.3e} (torch fp32 {err32:.3e}) of max {scale:.3e}")
    assert torch.isfinite(got).all()
    assert err <= max(1e-6 * scale, 2 * err32) + 1e-30


def test_dw1_zero_samples_and_argument_checks():
    from d2dhip import _lib
    lib = _lib.require_gpu()
    got = _dw1(64, 0, 100, 104, None, None)
    assert torch.equal(got, torch.zeros_like(got))
    assert lib.d2d_central_critic_dw1_workspace(62, 10, 100, 104) == -1   # hidden not a multiple of 4
    assert lib.d2d_central_critic_dw1_workspace(64, 10, 100, 96) == -1    # ldx < S
    xb, dhm = _operands(64, 64, 100, 104, seed=1)
    out = torch.empty((64, 100), device="cuda")
    ws = torch.empty((8,), device="cuda")  # too small
    with pytest.raises(ValueError):
        _lib.check(lib.d2d_central_critic_dw1(64, 64, 100, 104, xb.data_ptr(), dhm.data_ptr(), ws.data_ptr(), 8,
                                              out.data_ptr(), _lib.stream_ptr()), "d2d_central_critic_dw1")
