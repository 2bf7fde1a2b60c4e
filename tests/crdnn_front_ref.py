"""The CRDNN front end (modules/crdnn.py CNNFront, csrc/conv2d.hip) restated in torch on the CPU:
F.pad(mode='reflect') + F.conv2d, F.layer_norm over (F, C), F.leaky_relu(0.01), F.max_pool2d and an
injected Dropout2d keep mask, over channels-last [B, T, F, C] tensors, in fp64 by default.

bf16=True rounds every operand of an MFMA convolution to bf16 where the kernels do: its
activations and weights in the forward, and the output cotangent dy where it enters the input and
weight gradients (the bias gradient sums the unrounded dy; the Cin = 1 first layer is a direct fp32
kernel and rounds nothing).  SpeechBrain is absent here: tests/test_crdnn_front_cpu.py pins this
helper to a direct torch.nn composition."""
import torch
import torch.nn.functional as Fn


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _ste_round(t):
    """bf16-rounded values, the identity's gradient."""
    return t + (bf16_round(t) - t).detach()


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return bf16_round(g)


def conv3x3(x, w, b=None, bf16=False):
    """x [B, T, F, Cin] (or [B, T, F] for Cin = 1), w [Cout, Cin, 3, 3] -> [B, T, F, Cout]."""
    if x.dim() == 3:
        x = x.unsqueeze(-1)
    rounded = bf16 and w.shape[1] > 1
    if rounded:
        x, w = _ste_round(x), _ste_round(w)
    y = Fn.conv2d(Fn.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect"), w).permute(0, 2, 3, 1)
    if rounded:
        y = _RoundGrad.apply(y)
    return y + b if b is not None else y


def ln_act(x, gamma, beta, eps=1e-5):
    return Fn.leaky_relu(Fn.layer_norm(x, tuple(x.shape[2:]), gamma, beta, eps), 0.01)


def freq_pool(x, keep=None):
    """[B, T, F, C] -> [B, T, F // 2, C] (max over bin pairs, floor), times keep [B, F // 2]."""
    y = Fn.max_pool2d(x.permute(0, 3, 1, 2), (1, 2)).permute(0, 2, 3, 1)
    return y * keep.to(y.dtype)[:, None, :, None] if keep is not None else y


def time_pool(x):
    """[B, T, ...] -> [B, T // 2, ...] (max over frame pairs, floor)."""
    s = x.shape
    y = Fn.max_pool2d(x.reshape(s[0], 1, s[1], -1), (2, 1))
    return y.reshape(s[0], s[1] // 2, *s[2:])


def front(params, x, n_blocks, time_pooling, keep=None, bf16=False, dtype=torch.float64):
    """CNNFront.forward: params = its state dict (any dtype), x [B, T, F] -> [B, T', F_out * C]."""
    p = {k: v.to(dtype) for k, v in params.items()}
    h = x.to(dtype)
    for i in range(n_blocks):
        for j in (1, 2):
            h = conv3x3(h, p[f"block_{i}.conv_{j}.weight"], p[f"block_{i}.conv_{j}.bias"], bf16)
            h = ln_act(h, p[f"block_{i}.norm_{j}.weight"], p[f"block_{i}.norm_{j}.bias"])
        h = freq_pool(h, keep[i] if keep is not None else None)
    if time_pooling:
        h = time_pool(h)
    return h.reshape(h.shape[0], h.shape[1], -1)
