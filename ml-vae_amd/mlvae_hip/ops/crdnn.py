"""The CRDNN front end: 3x3 Conv2d, LayerNorm + LeakyReLU (+ pooling), time pooling
(csrc/conv2d.hip, csrc/norm.hip)."""
import torch

from .._lib import check, lib
from ._core import _need, _p, _prec, _stream, _workspace, _ws_bytes


def _need_bf16_products(what):
    if _prec() != 1:
        raise RuntimeError(f"{what}: the Conv2d kernels multiply bf16 operands (fp32 accumulate) and have no "
                           "fp32 form: set precision bf16")


class Conv2d3x3Fn(torch.autograd.Function):
    """y = conv2d(x) + b: 3x3, stride 1, reflect padding 1 on both axes, over channels-last
    x [B, T, F, Cin]; w [Cout, Cin, 3 (time), 3 (freq)] (torch.nn.Conv2d layout).  csrc/conv2d.hip:
    bf16 operands, fp32 accumulate; Cin, Cout multiples of 16 up to 256."""

    @staticmethod
    def forward(ctx, x, w, b):
        x, w = _need(x, "conv2d_3x3 x"), _need(w, "conv2d_3x3 weight")
        b = _need(b, "conv2d_3x3 bias") if b is not None else None
        B, T, F, Cin = x.shape
        Cout = w.shape[0]
        _need_bf16_products("conv2d_3x3")
        l = lib()
        y = torch.empty(B, T, F, Cout, device=x.device, dtype=torch.float32)
        ws = _workspace(l.mlvae_conv2d_workspace_size(0, B, T, F, Cin, Cout), "conv2d")
        check(l.mlvae_conv2d_fwd(B, T, F, Cin, Cout, _p(x), _p(w), _p(b) if b is not None else None, _p(y),
                                 _p(ws), _ws_bytes(ws), _stream()), "conv2d_fwd")
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _need(dy, "conv2d_3x3 grad")
        B, T, F, Cin = x.shape
        Cout = w.shape[0]
        _need_bf16_products("conv2d_3x3")
        l = lib()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            ws = _workspace(l.mlvae_conv2d_workspace_size(1, B, T, F, Cin, Cout), "conv2d")
            check(l.mlvae_conv2d_dgrad(B, T, F, Cin, Cout, _p(dy), _p(w), _p(dx), _p(ws), _ws_bytes(ws), _stream()),
                  "conv2d_dgrad")
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw = torch.empty_like(w)
            db = torch.empty(Cout, device=dy.device, dtype=torch.float32) if ctx.has_b else None
            ws = _workspace(l.mlvae_conv2d_workspace_size(2, B, T, F, Cin, Cout), "conv2d")
            check(l.mlvae_conv2d_wgrad(B, T, F, Cin, Cout, _p(dy), _p(x), _p(dw), _p(db) if db is not None else None,
                                       _p(ws), _ws_bytes(ws), _stream()), "conv2d_wgrad")
        return dx, dw, db


class Conv2dFirstFn(torch.autograd.Function):
    """The Cin = 1 layer: x [B, T, F] -> [B, T, F, Cout], w [Cout, 1, 3, 3]; direct fp32 kernels.  The
    features carry no gradient: an input that requires one raises."""

    @staticmethod
    def forward(ctx, x, w, b):
        x, w = _need(x, "conv2d_3x3 x"), _need(w, "conv2d_3x3 weight")
        b = _need(b, "conv2d_3x3 bias") if b is not None else None
        B, T, F = x.shape
        Cout = w.shape[0]
        y = torch.empty(B, T, F, Cout, device=x.device, dtype=torch.float32)
        check(lib().mlvae_conv2d_first_fwd(B, T, F, Cout, _p(x), _p(w), _p(b) if b is not None else None, _p(y),
                                           _stream()), "conv2d_first_fwd")
        ctx.save_for_backward(x, w)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _need(dy, "conv2d_3x3 grad")
        B, T, F = x.shape
        Cout = w.shape[0]
        l = lib()
        dw = torch.empty_like(w)
        db = torch.empty(Cout, device=dy.device, dtype=torch.float32) if ctx.has_b else None
        ws = _workspace(l.mlvae_conv2d_first_wgrad_workspace_size(B, T, F, Cout), "conv2d")
        check(l.mlvae_conv2d_first_wgrad(B, T, F, Cout, _p(dy), _p(x), _p(dw), _p(db) if db is not None else None,
                                         _p(ws), _ws_bytes(ws), _stream()), "conv2d_first_wgrad")
        return None, dw, db


def conv2d_3x3(x, w, b=None):
    """Conv2d(kernel 3x3, stride 1, padding 'same', padding_mode 'reflect') + bias over channels-last
    activations: x [B, T, F, Cin] (or the features [B, T, F] when w is [Cout, 1, 3, 3]) ->
    [B, T, F, Cout].  Unsupported sizes are a ValueError: there is no fallback."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"conv2d_3x3: weight must be [Cout, Cin, 3, 3], got {tuple(w.shape)}")
    Cout, Cin = int(w.shape[0]), int(w.shape[1])
    if b is not None and tuple(b.shape) != (Cout,):
        raise ValueError(f"conv2d_3x3: bias must be [{Cout}], got {tuple(b.shape)}")
    first = Cin == 1 and x.dim() == 3
    if not first and (x.dim() != 4 or x.shape[3] != Cin):
        raise ValueError(f"conv2d_3x3: x must be [B, T, F, {Cin}] (or [B, T, F] for Cin = 1), got {tuple(x.shape)}")
    if min(x.shape[:3]) < 1 or x.shape[1] < 2 or x.shape[2] < 2:
        raise ValueError(f"conv2d_3x3: reflect padding needs T >= 2 and F >= 2, got {tuple(x.shape)}")
    if first:
        if Cout % 16 or not 16 <= Cout <= 256:
            raise ValueError(f"conv2d_3x3: Cout = {Cout} must be a multiple of 16 up to 256")
        if x.requires_grad:
            raise ValueError("conv2d_3x3: the Cin = 1 layer has no input gradient (the features carry none)")
        return Conv2dFirstFn.apply(x, w, b)
    if not lib().mlvae_conv2d_supported(Cin, Cout):
        raise ValueError(f"conv2d_3x3: Cin = {Cin}, Cout = {Cout} must be multiples of 16 up to 256")
    return Conv2d3x3Fn.apply(x, w, b)


class LayerNormFCActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, keep, pool, eps):
        x = _need(x, "layer_norm_fc_act x")
        gamma, beta = _need(gamma, "layer_norm_fc_act weight"), _need(beta, "layer_norm_fc_act bias")
        keep = _need(keep, "layer_norm_fc_act keep") if keep is not None else None
        B, T, F, C = x.shape
        Fo = F // 2 if pool else F
        y = torch.empty(B, T, Fo, C, device=x.device, dtype=torch.float32)
        mean = torch.empty(B * T, device=x.device, dtype=torch.float32)
        rstd = torch.empty(B * T, device=x.device, dtype=torch.float32)
        check(lib().mlvae_ln_fc_act_fwd(B * T, T, F, C, _p(x), _p(gamma), _p(beta),
                                        _p(keep) if keep is not None else None, 1 if pool else 0, eps, _p(y),
                                        _p(mean), _p(rstd), _stream()), "ln_fc_act_fwd")
        ctx.save_for_backward(x, gamma, beta, mean, rstd, *([keep] if keep is not None else []))
        ctx.pool = pool
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, rstd = ctx.saved_tensors[:5]
        keep = ctx.saved_tensors[5] if len(ctx.saved_tensors) > 5 else None
        dy = _need(dy, "layer_norm_fc_act grad")
        B, T, F, C = x.shape
        l = lib()
        dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
        ws = _workspace(l.mlvae_ln_fc_act_bwd_workspace_size(B * T, F, C), "ln_fc_act")
        check(l.mlvae_ln_fc_act_bwd(B * T, T, F, C, _p(dy), _p(x), _p(gamma), _p(beta),
                                    _p(keep) if keep is not None else None, 1 if ctx.pool else 0, _p(mean), _p(rstd),
                                    _p(dx), _p(dg), _p(db), _p(ws), _ws_bytes(ws), _stream()), "ln_fc_act_bwd")
        return dx, dg, db, None, None, None


def layer_norm_fc_act(x, weight, bias, pool=False, keep=None, eps=1e-5):
    """LeakyReLU_0.01(LayerNorm over (F, C) of x [B, T, F, C]) with the affine weight / bias [F, C]
    (biased variance); pool: then the frequency max-pool 2 (floor; a tie keeps the lower bin) and the
    Dropout2d factor keep [B, F // 2] (0 or 1 / (1 - p); None = no dropout) -> [B, T, F // 2, C]."""
    if x.dim() != 4:
        raise ValueError(f"layer_norm_fc_act: x must be [B, T, F, C], got {tuple(x.shape)}")
    B, T, F, C = (int(v) for v in x.shape)
    if tuple(weight.shape) != (F, C) or tuple(bias.shape) != (F, C):
        raise ValueError(f"layer_norm_fc_act: weight / bias must be [{F}, {C}], got {tuple(weight.shape)} / "
                         f"{tuple(bias.shape)}")
    if B * T < 1 or C % 4 or (pool and F < 2):
        raise ValueError(f"layer_norm_fc_act: unsupported shape {tuple(x.shape)} (C % 4 == 0; pooling needs F >= 2)")
    if keep is not None and (not pool or tuple(keep.shape) != (B, F // 2)):
        raise ValueError(f"layer_norm_fc_act: keep must be [{B}, {F // 2}] and needs pool=True")
    return LayerNormFCActFn.apply(x, weight, bias, keep, bool(pool), float(eps))


class TimePoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _need(x, "time_pool x")
        B, T = x.shape[:2]
        D = x.numel() // (B * T)
        y = torch.empty(B, T // 2, *x.shape[2:], device=x.device, dtype=torch.float32)
        check(lib().mlvae_time_pool_fwd(B, T, D, _p(x), _p(y), _stream()), "time_pool_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        dy = _need(dy, "time_pool grad")
        B, T = x.shape[:2]
        dx = torch.empty_like(x)
        check(lib().mlvae_time_pool_bwd(B, T, x.numel() // (B * T), _p(dy), _p(x), _p(dx), _stream()),
              "time_pool_bwd")
        return dx


def time_pool(x):
    """Max over frame pairs of x [B, T, ...] -> [B, T // 2, ...] (floor: an odd last frame is dropped)."""
    if x.dim() < 3 or x.shape[0] < 1 or x.shape[1] < 2 or (x.numel() // (x.shape[0] * x.shape[1])) % 4:
        raise ValueError(f"time_pool: x must be [B, T >= 2, ...] with a multiple of 4 elements per frame, got "
                         f"{tuple(x.shape)}")
    return TimePoolFn.apply(x)
