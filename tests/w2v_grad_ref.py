"""The gradient oracle of the trainable wav2vec2 encoder: tests/w2v_ref.py is plain differentiable
torch, so its autograd in float64 is the truth; the same autograd in float32 and under bf16
autocast are the yardsticks ("The wav2vec2 encoder", "Backward").

Tolerance rule shared by the backward's tests: per tensor, the yardstick is the error against float64
of the same autograd in float32 (precision 'fp32') or under bf16 autocast ('bf16'), as maximum and
relative RMS, floored at 2^-23 relative (a yardstick that happens to be exact would otherwise ask
for more than fp32 holds); the device is held to 4 x both.
"""
import torch

import w2v_ref as R

FLOOR = 2.0 ** -23


def trainable(key):
    """What fine-tuning with a frozen feature extractor trains: everything from the projection
    upward (masked_spec_embed is unused without masking)."""
    return key.startswith(("feature_projection.", "encoder."))


def held(got, r64, yard, what):
    """Print the figures, then hold `got` to 4 x the yardstick's floored errors against float64."""
    got, r64, yard = got.detach().cpu(), r64.detach().double(), yard.detach().cpu()
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    e, y = R.errors(got, r64), R.errors(yard, r64)
    ymax, yrms = max(y[0], FLOOR * r64.abs().max().item()), max(y[1], FLOOR)
    print(f"{what}: device (max {e[0]:.3e}, rms {e[1]:.3e}), yardstick (max {y[0]:.3e}, rms {y[1]:.3e})")
    assert torch.isfinite(got).all(), what
    assert e[0] <= 4 * ymax and e[1] <= 4 * yrms, (what, e, (ymax, yrms))
    return e, y


def encoder_grads(state, cfg, wav, cot, mode, normalize_wav=True, output_norm=True):
    """loss = sum(out * cot) through w2v_ref.forward.  mode: 'fp64', 'fp32' or 'bf16' (autocast).
    Returns (out, {trainable key: gradient}, the gradient at the `proj` stage), detached."""
    dt = torch.float64 if mode == "fp64" else torch.float32
    st = {k: v.detach().to(dt).clone().requires_grad_(trainable(k)) for k, v in state.items()}
    stages = {}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=mode == "bf16"):
        out = R.forward(st, cfg, wav.to(dt), normalize_wav=normalize_wav, output_norm=output_norm, stages=stages)
    stages["proj"].retain_grad()
    (out.to(dt) * cot.to(dt)).sum().backward()
    grads = {k: v.grad.detach() for k, v in st.items() if trainable(k)}
    return out.detach(), grads, stages["proj"].grad.detach()
