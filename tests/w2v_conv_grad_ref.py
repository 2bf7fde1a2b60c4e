"""The gradient oracle of the wav2vec2 encoder trained whole (train_feature_extractor=True): the
autograd of tests/w2v_ref.py with every key but masked_spec_embed requiring grad, in float64 (the
truth), float32 and under bf16 autocast (the yardsticks), held by tests/w2v_grad_ref.held; and the
op-level oracles of the conv stack's backward ("The wav2vec2 encoder",
"Backward", "The conv stack"): F.conv1d + layer_norm + gelu autograd on the CPU.

conv_dx_by_residue restates the input gradient's residue decomposition (ops.w2v_conv_dx) in plain
torch, index for index; tests/test_w2v_conv_train_cpu.py checks it against conv1d's autograd."""
import torch
import torch.nn.functional as F

import w2v_ref as R
from w2v_grad_ref import held  # noqa: F401  (the tolerance rule, shared)


def trainable(key):
    """What train_feature_extractor=True trains: everything but masked_spec_embed (unused without masking)."""
    return key != "masked_spec_embed"


def encoder_grads(state, cfg, wav, cot, mode, normalize_wav=True, output_norm=True):
    """loss = sum(out * cot) through w2v_ref.forward.  mode: 'fp64', 'fp32' or 'bf16' (autocast).
    Returns (out, {trainable key: gradient}), detached."""
    dt = torch.float64 if mode == "fp64" else torch.float32
    st = {k: v.detach().to(dt).clone().requires_grad_(trainable(k)) for k, v in state.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=mode == "bf16"):
        out = R.forward(st, cfg, wav.to(dt), normalize_wav=normalize_wav, output_norm=output_norm)
    (out.to(dt) * cot.to(dt)).sum().backward()
    return out.detach(), {k: v.grad.detach() for k, v in st.items() if trainable(k)}


def conv_dx_by_residue(dy, w, stride, T_in):
    """dx [B, T_in, Cin] of y = conv1d(x, w [Cout, Cin, k], stride) given dy [B, Tout, Cout], channels-last:
    with n = stride u + r,  dx[n] = sum_{q < m_r} dy[u - q] . w[:, :, r + q stride],
    m_r = ceil((k - r) / stride), dy = 0 outside [0, Tout) -- one product per residue r over the
    overlapping rows [dy[u - m_r + 1] .. dy[u]] of the guarded dy against the taps in reverse order."""
    B, Tout, Cout = dy.shape
    _, Cin, k = w.shape
    m = [-((r - k) // stride) for r in range(stride)]
    pf, U = m[0] - 1, -(-T_in // stride)
    pad = dy.new_zeros(B, pf + U, Cout)  # U >= Tout: the rows past the last frame are guards too
    pad[:, pf:pf + Tout] = dy
    dx = dy.new_zeros(B, T_in, Cin)
    for r in range(stride):
        Ur = -(-(T_in - r) // stride)
        wr = w[:, :, r::stride].flip(-1).permute(1, 2, 0).reshape(Cin, m[r] * Cout)  # [Cin][q reversed][Cout]
        rows = torch.stack([pad[:, pf - (m[r] - 1) + u: pf + u + 1].reshape(B, m[r] * Cout) for u in range(Ur)], dim=1)
        dx[:, r::stride] = rows @ wr.t()
    return dx


def conv_grads(x, w, dy, stride, dtype, round_bf16=False):
    """(dx [B, T_in, Cin], dw [Cout, Cin, k]) of conv1d by autograd in `dtype`, channels-last x / dy;
    round_bf16: the three operands rounded to bf16 first (the bf16 mode's yardstick)."""
    rnd = (lambda t: t.to(torch.bfloat16)) if round_bf16 else (lambda t: t)
    x = rnd(x).to(dtype).clone().requires_grad_(True)
    w = rnd(w).to(dtype).clone().requires_grad_(True)
    y = F.conv1d(x.transpose(1, 2), w, stride=stride).transpose(1, 2)
    (y * rnd(dy).to(dtype)).sum().backward()
    return x.grad.detach(), w.grad.detach()


def conv0_grads(wav, stats, w, b, g, be, stride, dout, eps, dtype):
    """(dw [C, K], dbias, dgamma, dbeta) of GELU(LN_C(conv1d((wav - mean) rstd, w) + b)) by autograd in
    `dtype`; stats: None or the two fp32 numbers the device is given (constants: no gradient)."""
    x = wav.to(dtype)
    if stats is not None:
        x = (x - stats[0].to(dtype)) * stats[1].to(dtype)
    p = [t.to(dtype).clone().requires_grad_(True) for t in (w, b, g, be)]
    y = F.conv1d(x.unsqueeze(1), p[0].unsqueeze(1), p[1], stride=stride).transpose(1, 2)
    out = F.gelu(F.layer_norm(y, (w.shape[0],), p[2], p[3], eps))
    (out * dout.to(dtype)).sum().backward()
    return [t.grad.detach() for t in p]
