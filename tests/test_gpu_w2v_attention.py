"""The wav2vec2 attention kernel (csrc/w2v.hip, mlvae_hip.ops.w2v_attention) against float64
softmax attention computed here.

Tolerance rule (as tests/test_gpu_w2v_kernels.py): the yardstick is the same attention in torch
on the CPU -- float32 for the fp32-MFMA parity mode, bf16 autocast for the bf16-operand mode -- and
its maximum / relative-RMS error against float64; the device is held to 4 x both.  Both modes read
the same fp32 qkv.  Figures are printed before they are asserted.
"""
import pytest
import torch

import w2v_ref as R
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu

# T: one query; a ragged 32-key tile; exactly one workgroup of 64 queries and one past it; two
# workgroups and a ragged tile; four and one query more
SHAPES = [(T, d, H) for T in (1, 37, 64, 65, 130, 257) for d in (32, 64) for H in (1, 2, 16)]


def qkv_of(B, T, H, d, seed, qscale=1.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, 3 * H * d, generator=g)
    qkv[:, :H * d] *= qscale
    return qkv


def ref_attention(qkv, B, T, H, d, dt, autocast=False):
    """softmax(Q K^T / sqrt(d)) V per (utterance, head)."""
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        q, k, v = (t.reshape(B, T, H, d).transpose(1, 2) for t in qkv.to(dt).view(B, T, 3, H * d).unbind(2))
        p = torch.softmax((q @ k.transpose(-1, -2)) * d ** -0.5, dim=-1)
        return (p.to(v.dtype) @ v).transpose(1, 2).reshape(B * T, H * d).float()


def run(qkv, B, T, H, d, prec):
    from mlvae_hip import ops
    return ops.w2v_attention(qkv.cuda(), B, T, H, d, scale=d ** -0.5, f32_math=prec == "fp32")


def held(got, r64, yard, what):
    e, y = R.errors(got.cpu(), r64), R.errors(yard, r64)
    print(f"{what}: device (max {e[0]:.3e}, rms {e[1]:.3e}), yardstick (max {y[0]:.3e}, rms {y[1]:.3e})")
    assert torch.isfinite(got).all(), what
    assert e[0] <= 4 * y[0] and e[1] <= 4 * y[1], (what, e, y)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("T,d,H", SHAPES)
def test_attention(T, d, H, prec):
    need_gpu()
    B = 2
    qkv = qkv_of(B, T, H, d, seed=T * 100 + d + H)
    r64 = ref_attention(qkv, B, T, H, d, torch.float64).double()
    yard = ref_attention(qkv, B, T, H, d, torch.float32, autocast=prec == "bf16")
    got = run(qkv, B, T, H, d, prec)
    assert got.shape == (B * T, H * d) and got.dtype == torch.float32
    held(got, r64, yard, f"attention T={T} d={d} H={H} {prec}")
    assert torch.equal(got, run(qkv, B, T, H, d, prec))  # a second launch: identical bits


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_attention_large_logits(prec):
    """Q scaled by 30: logits near 200.  exp() of an unshifted logit overflows fp32, and a lost
    running maximum shows as a wrong row, so this checks the online rescale."""
    need_gpu()
    B, T, H, d = 2, 130, 2, 64
    qkv = qkv_of(B, T, H, d, seed=5, qscale=30.0)
    assert (qkv[:, :H * d].abs().max() * qkv[:, H * d:2 * H * d].abs().max()) > 200
    r64 = ref_attention(qkv, B, T, H, d, torch.float64).double()
    yard = ref_attention(qkv, B, T, H, d, torch.float32, autocast=prec == "bf16")
    held(run(qkv, B, T, H, d, prec), r64, yard, f"attention, logits near 200, {prec}")


def test_attention_bf16_io():
    """bf16 qkv in and bf16 out (the formats an all-bf16 caller would use): the same bound as the bf16 mode."""
    need_gpu()
    from mlvae_hip import ops
    B, T, H, d = 2, 65, 2, 64
    qkv = qkv_of(B, T, H, d, seed=9).bfloat16().float()
    r64 = ref_attention(qkv, B, T, H, d, torch.float64).double()
    yard = ref_attention(qkv, B, T, H, d, torch.float32, autocast=True)
    got = ops.w2v_attention(qkv.cuda().bfloat16(), B, T, H, d, scale=d ** -0.5, out_dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16
    held(got.float(), r64, yard, "attention bf16 in / out")


def test_unsupported_head_width_raises():
    need_gpu()
    from mlvae_hip import ops
    assert not ops.w2v_attention_supported(10, 2, 48)
    with pytest.raises(ValueError, match="unsupported"):
        ops.w2v_attention(torch.zeros(10, 3 * 2 * 48, device="cuda"), 1, 10, 2, 48)
