"""Linear (+LeakyReLU) and the Conv1d encoder (csrc/gemm*.hip, csrc/conv.hip)."""
import torch

from .._lib import check, lib
from ._core import colsum, gemm, _need, _p, _prec, _rows, _stream, _workspace, _ws_bytes


# --------------------------------------------------------------------------- Linear (+LReLU)
class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b), act = LeakyReLU(0.01) or identity (ref:src/modules/fc_block.py:10-16)."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        x, w = _need(x, "linear x"), _need(w, "linear weight")
        b = _need(b, "linear bias") if b is not None else None
        M, K = _rows(x), x.shape[-1]
        N = w.shape[0]
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        gemm(0, 1, M, N, K, _p(x), K, _p(w), K, _p(y), N, bias1=_p(b) if b is not None else None,
             epi=1 if act else 0)
        ctx.save_for_backward(x, w, y)
        ctx.act, ctx.has_b = act, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = _need(dy, "linear grad")
        M, K, N = _rows(x), x.shape[-1], w.shape[0]
        if ctx.act:  # dpre = dy * lrelu'(y)
            dpre = torch.empty_like(dy)
            check(lib().mlvae_lrelu_bwd(dy.numel(), _p(dy), _p(y), _p(dpre), _stream()), "lrelu_bwd")
        else:
            dpre = dy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(0, 0, M, K, N, _p(dpre), N, _p(w), K, _p(dx), K)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w)
            gemm(1, 0, N, K, M, _p(dpre), N, _p(x), K, _p(dw), K)
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = torch.empty(N, device=dy.device, dtype=torch.float32)
            colsum(M, N, _p(dpre), N, _p(db))
        return dx, dw, db, None


def linear(x, w, b=None, act=False):
    return LinearFn.apply(x, w, b, act)


# --------------------------------------------------------------------------- Conv1d encoder
def _conv_ws(nbytes):
    return _workspace(max(int(nbytes), 16), key="conv_wgrad")


class Conv1dFn(torch.autograd.Function):
    """y = act(conv1d(x) + b) over the time axis of batch-first frames x [B, T, Cin]; w
    [Cout, Cin, K] (torch.nn.Conv1d layout, padding (K-1)/2 at each utterance's ends).
    BASELINE.json configs[3]'s Conv1d encoder (csrc/conv.hip); bf16 operands, fp32 accumulate."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        x, w = _need(x, "conv1d x"), _need(w, "conv1d weight")
        b = _need(b, "conv1d bias") if b is not None else None
        if x.dim() != 3:
            raise ValueError("conv1d: x must be [B, T, C]")
        if _prec() != 1:
            raise RuntimeError("the Conv1d encoder kernels use bf16 operands: set precision bf16")
        B, T, Cin = x.shape
        Cout, _, K = w.shape
        y = torch.empty(B, T, Cout, device=x.device, dtype=torch.float32)
        check(lib().mlvae_conv1d_fwd(B, T, Cin, Cout, K, _p(x), Cin, _p(w), _p(b) if b is not None else None,
                                     1 if act else 0, _p(y), Cout, _stream()), "conv1d_fwd")
        ctx.save_for_backward(x, w, y)
        ctx.act, ctx.has_b = act, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = _need(dy, "conv1d grad")
        B, T, Cin = x.shape
        Cout, _, K = w.shape
        if ctx.act:  # dpre = dy * lrelu'(y)
            dpre = torch.empty_like(dy)
            check(lib().mlvae_lrelu_bwd(dy.numel(), _p(dy), _p(y), _p(dpre), _stream()), "lrelu_bwd")
        else:
            dpre = dy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(lib().mlvae_conv1d_dgrad(B, T, Cin, Cout, K, _p(dpre), Cout, _p(w), None, 0, _p(dx), Cin,
                                           _stream()), "conv1d_dgrad")
        if ctx.needs_input_grad[1] or (ctx.has_b and ctx.needs_input_grad[2]):
            dw = torch.empty_like(w)
            db = torch.empty(Cout, device=dy.device, dtype=torch.float32)
            nb = lib().mlvae_conv1d_wgrad_workspace_size(B, T, Cin, Cout, K)
            ws = _conv_ws(nb)
            check(lib().mlvae_conv1d_wgrad(B, T, Cin, Cout, K, _p(dpre), Cout, _p(x), Cin, _p(dw), _p(db),
                                           _p(ws), _ws_bytes(ws), _stream()), "conv1d_wgrad")
            if not ctx.has_b:
                db = None
        return dx, dw, db, None


def conv1d(x, w, b=None, act=False):
    return Conv1dFn.apply(x, w, b, act)
