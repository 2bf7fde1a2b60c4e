"""torch.autograd.Functions over libmlvae.so: the operator layer under the drop-in
nn.Modules (modules/fc_block.py, modules/vanilla_vae.py, modules/decoder.py).

Every forward and backward below is a libmlvae.so launch on the current HIP stream; torch
only allocates the output tensors.  Inputs must be fp32 CUDA tensors (row-major [B, T, C]).
The fused training step (mlvae_hip/engine.py) uses the same kernels without autograd.
"""
import ctypes

import torch

from ._lib import SZ, check, lib

PREC = {"fp32": 0, "bf16": 1}
_state = {"prec": "fp32"}
_ws = {}


def set_precision(prec):
    """Operand precision of the matrix products: "fp32" (exact f32 MFMA) or "bf16"."""
    if prec not in PREC:
        raise ValueError(f"precision must be one of {list(PREC)}")
    _state["prec"] = prec


def get_precision():
    return _state["prec"]


class precision:
    """Context: matrix-product operand precision inside the block (the mixed-precision region of
    MDModel.fit_batch's auto_mix_prec branch; backward runs inside it too, since the HIP ops read
    the precision when they launch)."""

    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        self.prev = get_precision()
        set_precision(self.prec)
        return self

    def __exit__(self, *exc):
        set_precision(self.prev)


def _prec():
    return PREC[_state["prec"]]


class shard:
    """Context: the batch inside the block is a data-parallel shard of a global batch of
    B_global utterances, its first utterance at utt_offset.  Every drawing op (randn, the LSTM's
    inter-layer dropout, boundary_heads, pi_sample, pi_sample_k, GmmLatentFn, HvaeLatentFn) then draws, for
    each of its utterances, bit for bit what the single process draws for that utterance of the
    global batch (include/mlvae.h, "the random streams over an utterance map"): the ops take the
    seeds from torch's CPU generator as they always do, so ranks seeded alike that make the same
    calls in the same order agree.  Backward passes that recompute a draw (dropout, the boundary
    draws) use the map of their forward.  global_lens = the relative lengths [B_global] of the
    global batch: masked_mean's default global denominator inside the block.  folded(K) is the
    context of MD_VAE_sfl's K-folded batch [K * B_local, T, .] (draw k of utterance b at row
    k * B_local + b).  Without a context the ops call what they always called."""

    def __init__(self, utt_offset, B_global, global_lens=None, K=1):
        if utt_offset < 0 or B_global < 1 or K < 1:
            raise ValueError(f"shard: utt_offset {utt_offset}, B_global {B_global}, K {K}")
        self.utt_offset, self.B_global, self.K = int(utt_offset), int(B_global), int(K)
        self.global_lens = global_lens

    def folded(self, K):
        return shard(self.utt_offset, self.B_global, self.global_lens, K)

    def map(self, B):
        """The ABI's (utt_offset, seg_utts, seg_stride, total_utts) for a batch of B rows."""
        if B % self.K:
            raise ValueError(f"shard: {B} rows are not {self.K} folds of a local batch")
        Bl = max(B // self.K, 1)
        # rows past B_global are the fillers of a short slice: masked out by their zero lengths
        return (ctypes.c_longlong * 4)(self.utt_offset, Bl, self.B_global, self.K * self.B_global)

    def global_frames(self, T):
        """Valid frames of the global batch padded to T (the masked means' global count)."""
        if self.global_lens is None:
            return None
        return valid_frames(self.global_lens, T)

    def __enter__(self):
        self.prev = _state.get("shard")
        _state["shard"] = self
        return self

    def __exit__(self, *exc):
        _state["shard"] = self.prev


def current_shard():
    return _state.get("shard")


def valid_frames(lens, T):
    """Frames the masked means count for relative lengths `lens` at padded length T: frame t is
    valid iff (float)t < fp32(len * T) (csrc/common.h valid_frames), summed over the utterances."""
    lim = torch.as_tensor(lens, dtype=torch.float32).cpu() * float(T)
    c = torch.where(lim > 0, torch.ceil(lim).clamp(max=float(T)), torch.zeros_like(lim))
    return int(c.sum().item())


def _bt(shape, what):
    """(B, T, C) of a [B, T, ...] batch: what the mapped streams index."""
    if len(shape) < 2:
        raise ValueError(f"{what}: a sharded draw needs a [B, T, ...] batch, got {tuple(shape)}")
    C = 1
    for d in shape[2:]:
        C *= int(d)
    return int(shape[0]), int(shape[1]), C


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t, off=0):
    return t.data_ptr() + 4 * off


def _need(t, name):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise TypeError(f"{name}: expected a float32 HIP tensor, got {t.dtype} on {t.device} "
                        "(the HIP path has no CPU fallback)")
    return t.contiguous()


def _workspace(nbytes, key="gemm"):
    dev = torch.cuda.current_device()
    w = _ws.get((dev, key))
    if w is None or w.numel() * 4 < nbytes:
        w = torch.empty(max(nbytes // 4 + 1, 1024), device="cuda", dtype=torch.float32)
        _ws[(dev, key)] = w
    return w


def gemm(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias1=None, bias2=None, epi=0, aux=None,
         ldaux=0, beta=0.0, kshift_T=0, kshift=0):
    """C = epi(op(A) op(B) + bias1 + bias2 + beta*C) on raw device pointers (ints)."""
    l = lib()
    ws = _workspace(l.mlvae_gemm_workspace_size(M, N, K))
    check(l.mlvae_gemm(_prec(), ta, tb, M, N, K, 1.0, A, lda, B, ldb, beta, C, ldc, bias1, bias2,
                       epi, aux, ldaux, kshift_T, kshift, _p(ws), ws.numel() * 4, _stream()),
          "mlvae_gemm")


def colsum(N, Cn, src, ld, out, out2=None, beta=0.0):
    l = lib()
    ws = _workspace(l.mlvae_colsum_workspace_size(N, Cn), "colsum")
    check(l.mlvae_colsum(N, Cn, src, ld, out, out2, beta, _p(ws), ws.numel() * 4, _stream()),
          "mlvae_colsum")


def _rows(x):
    return x.numel() // x.shape[-1]


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
                                           _p(ws), ws.numel() * ws.element_size(), _stream()), "conv1d_wgrad")
            if not ctx.has_b:
                db = None
        return dx, dw, db, None


def conv1d(x, w, b=None, act=False):
    return Conv1dFn.apply(x, w, b, act)


# --------------------------------------------------------------------------- CRDNN front end
def _ws_bytes(ws):
    return ws.numel() * ws.element_size()


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


# --------------------------------------------------------------------------- ELBO part 1
class ReparamKLFn(torch.autograd.Function):
    """z = eps*exp(lv/2) + mu and per-element KL (ref:src/modules/vanilla_vae.py:37-45);
    ml = [mu | log_var] along the last dim."""

    @staticmethod
    def forward(ctx, ml, eps):
        ml, eps = _need(ml, "ml"), _need(eps, "eps")
        Z = ml.shape[-1] // 2
        N = _rows(ml)
        z = torch.empty(*ml.shape[:-1], Z, device=ml.device, dtype=torch.float32)
        kl = torch.empty_like(z)
        # rows are independent: pass them as B=N utterances of T=1 frame (mask all-valid)
        ones = _ones(N)
        check(lib().mlvae_reparam_kl_fwd(N, 1, Z, _p(ml), 2 * Z, _p(eps), _p(ones), _p(z), _p(kl),
                                         None, _stream()), "reparam_kl_fwd")
        ctx.save_for_backward(ml, eps)
        return z, kl

    @staticmethod
    def backward(ctx, dz, dkl):
        ml, eps = ctx.saved_tensors
        Z = ml.shape[-1] // 2
        N = _rows(ml)
        dz = _need(dz, "dz") if dz is not None else torch.zeros(*ml.shape[:-1], Z, device=ml.device)
        dkl = _need(dkl, "dkl") if dkl is not None else torch.zeros_like(dz)
        dml = torch.empty_like(ml)
        check(lib().mlvae_reparam_kl_bwd(N, 1, Z, _p(ml), 2 * Z, _p(eps), _p(_ones(N)), None,
                                         _p(dz), _p(dkl), 0.0, _p(dml), 2 * Z, _stream()),
              "reparam_kl_bwd")
        return dml, None


def _ones(n):
    dev = torch.cuda.current_device()
    o = _ws.get((dev, "ones"))
    if o is None or o.numel() < n:
        o = torch.ones(max(n, 1024), device="cuda", dtype=torch.float32)
        _ws[(dev, "ones")] = o
    return o


def randn(shape, generator=None):
    """N(0,1) from the library's Philox stream; the seed is drawn from torch's (CPU) RNG so
    torch.manual_seed (ref:src/config/run.yaml:2-3) makes it reproducible."""
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    out = torch.empty(*shape, device="cuda", dtype=torch.float32)
    sh = current_shard()
    if sh is not None:
        B, T, C = _bt(out.shape, "randn")
        check(lib().mlvae_randn_rows(B, T, C, seed, sh.map(B), _p(out), _stream()), "randn_rows")
        return out
    check(lib().mlvae_randn(out.numel(), seed, 0, _p(out), _stream()), "randn")
    return out


# --------------------------------------------------------------------------- ELBO part 2
LOSS = {"likelihood": 0, "mse": 1}


class ReconFn(torch.autograd.Function):
    """Per-element reconstruction loss (ref:src/modules/decoder.py:37-53)."""

    @staticmethod
    def forward(ctx, mux, lvx, x, loss_type):
        mux, x = _need(mux, "mean"), _need(x, "target")
        lt = LOSS[loss_type]
        lvx = _need(lvx, "log_var") if lt == 0 else mux
        F = mux.shape[-1]
        N = _rows(mux)
        rec = torch.empty_like(mux)
        check(lib().mlvae_recon(N, 1, F, lt, _p(mux), F, _p(lvx), F, _p(x), F, _p(_ones(N)), None,
                                _p(rec), None, None, 0.0, None, None, _stream()), "recon")
        ctx.save_for_backward(mux, lvx, x)
        ctx.lt = lt
        return rec

    @staticmethod
    def backward(ctx, drec):
        mux, lvx, x = ctx.saved_tensors
        drec = _need(drec, "recon grad")
        F, N = mux.shape[-1], _rows(mux)
        dmux = torch.empty_like(mux)
        dlvx = torch.empty_like(mux) if ctx.lt == 0 else None
        check(lib().mlvae_recon(N, 1, F, ctx.lt, _p(mux), F, _p(lvx), F, _p(x), F, _p(_ones(N)),
                                None, None, None, _p(drec), 0.0, _p(dmux),
                                _p(dlvx) if dlvx is not None else None, _stream()), "recon_bwd")
        return dmux, dlvx, None, None


def recon_loss(mean, log_var, target, loss_type):
    if loss_type not in LOSS:
        raise ValueError(f"Invalid loss type: {loss_type}")  # ref:src/modules/decoder.py:50-51
    return ReconFn.apply(mean, log_var if loss_type == "likelihood" else mean, target, loss_type)


# --------------------------------------------------------------------------- masked mean
RED = {"mean": 0, "batchmean": 1, "batch": 2}


class MaskedMeanFn(torch.autograd.Function):
    """apply_lens_to_loss (ref:src/utils/data_utils.py:67-104)."""

    @staticmethod
    def forward(ctx, loss, lens, reduction):
        loss = _need(loss, "loss")
        lens = _need(lens.to(loss.device, torch.float32), "lens")
        B, T = loss.shape[0], loss.shape[1]
        C = loss.numel() // (B * T) if B * T else 1
        out = torch.empty(2 * B if B else 2, device=loss.device, dtype=torch.float32)
        check(lib().mlvae_masked_mean(B, T, C, _p(loss), _p(lens), RED[reduction], _p(out),
                                      _stream()), "masked_mean")
        ctx.save_for_backward(lens)
        ctx.shape, ctx.red = loss.shape, RED[reduction]
        return out[:B].clone() if reduction == "batch" else out[0].clone()

    @staticmethod
    def backward(ctx, g):
        (lens,) = ctx.saved_tensors
        B, T = ctx.shape[0], ctx.shape[1]
        C = 1
        for d in ctx.shape[2:]:
            C *= d
        g = _need(g.reshape(-1), "grad")
        dloss = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        check(lib().mlvae_masked_mean_bwd(B, T, C, _p(lens), ctx.red, _p(g), _p(dloss), _stream()),
              "masked_mean_bwd")
        return dloss, None, None


def masked_mean(loss, lens, reduction="mean", global_frames=None):
    """global_frames: the valid frames of the global batch this batch is a shard of (default
    inside an ops.shard context that carries global_lens: its count).  The "mean" is then this
    shard's share of the global mean -- local masked sum / (global_frames * C), so the shares
    of all shards add up to the single-process mean -- and a shard of fillers alone gives 0."""
    if reduction not in RED:
        raise ValueError(f"unknown reduction {reduction}")
    sh = current_shard()
    if global_frames is None and sh is not None and reduction == "mean" and loss.dim() >= 2:
        global_frames = sh.global_frames(loss.shape[1])
    if global_frames is None:
        return MaskedMeanFn.apply(loss, lens, reduction)
    if reduction != "mean":
        raise ValueError("masked_mean: a global denominator belongs to reduction 'mean'")
    B, T = loss.shape[0], loss.shape[1]
    C = loss.numel() // (B * T) if B * T else 1
    if global_frames < 1:
        raise ValueError("masked_mean: the global batch has no valid frame")
    # batchmean = masked sum / B (no local count in it): rescaled to sum / (global frames * C)
    return MaskedMeanFn.apply(loss, lens, "batchmean") * (float(B) / (float(global_frames) * C))


# --------------------------------------------------------------------------- BiLSTM
def _lstm_ws(B, H):
    xb = SZ()
    check(lib().mlvae_lstm_workspace_size(B, H, _prec(), ctypes.byref(xb)), "lstm_workspace_size")
    x = _workspace(xb.value, "lstm_x")
    err = _ws.get((torch.cuda.current_device(), "lstm_err"))
    if err is None:
        err = torch.zeros(1, device="cuda", dtype=torch.int32)
        _ws[(torch.cuda.current_device(), "lstm_err")] = err
    return x, err


def _dropout(src, dst, seed, p, sh=None):
    if sh is not None:
        B, T, C = _bt(src.shape, "lstm dropout")
        check(lib().mlvae_dropout_rows(B, T, C, _p(src), _p(dst), seed, p, sh.map(B), _stream()),
              "dropout_rows")
        return
    check(lib().mlvae_dropout(src.numel(), _p(src), _p(dst), None, seed, p, _stream()), "dropout")


class LSTMFn(torch.autograd.Function):
    """nn.LSTM(batch_first=True) on libmlvae, bidirectional (ndir 2: ref:src/modules/decoder.py:14-15,22)
    or not (ndir 1: ref:src/modules/phoneme_recognizer.py:13, boundary_detector.py:19): per layer
    an input-projection GEMM per direction + the persistent recurrence; inter-layer dropout
    (Philox, recomputed in backward) in train mode.  weights = the layer-major list
    [w_ih, w_hh, b_ih, b_hh] (+ [w_ih_r, w_hh_r, b_ih_r, b_hh_r] when bidirectional) * L."""

    @staticmethod
    def forward(ctx, x, H, L, ndir, dropout, seed, *weights):
        x = _need(x, "lstm input")
        B, T, _ = x.shape
        N = B * T
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        nw = 4 * ndir
        saved, inputs, seeds = [], [], []
        h = x
        for li in range(L):
            w = [_need(t, "lstm weight") for t in weights[nw * li:nw * li + nw]]
            din = h.shape[-1]
            G = torch.empty(N, 4 * H * ndir, device=x.device, dtype=torch.float32)
            for d in range(ndir):
                wi, _, bi, bh = w[4 * d:4 * d + 4]
                gemm(0, 1, N, 4 * H, din, _p(h), din, _p(wi), din, _p(G, 4 * H * d), 4 * H * ndir,
                     bias1=_p(bi), bias2=_p(bh))
            Cs = torch.empty(N, H * ndir, device=x.device, dtype=torch.float32)
            Y = torch.empty(B, T, H * ndir, device=x.device, dtype=torch.float32)
            if ndir == 2:
                check(l.mlvae_lstm_fwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(Y),
                                       _p(xbuf), xbuf.numel() * 4, _p(err), _stream()), "lstm_fwd")
            else:
                check(l.mlvae_lstm1_fwd(_prec(), B, T, H, _p(w[1]), _p(G), _p(Cs), _p(Y), None,
                                        _p(xbuf), xbuf.numel() * 4, _p(err), _stream()), "lstm1_fwd")
            inputs.append(h)
            saved += [G, Cs, Y]
            h = Y
            if li < L - 1 and dropout > 0:
                s = (seed * 1000003 + li) & ((1 << 63) - 1)
                hd = torch.empty_like(Y)
                _dropout(Y, hd, s, dropout, current_shard())
                seeds.append(s)
                h = hd
            else:
                seeds.append(None)
        ctx.save_for_backward(*inputs, *saved, *weights)
        ctx.H, ctx.L, ctx.ndir, ctx.dropout, ctx.seeds = H, L, ndir, dropout, seeds
        ctx.shard = current_shard()  # the backward recomputes the masks under the forward's map
        # nn.LSTM's (h_n, c_n) [L*ndir, B, H]: every layer's state after its last step (t = T-1
        # forward, t = 0 reverse; no packing, as nn.LSTM on a padded batch)
        hn = torch.empty(L * ndir, B, H, device=x.device, dtype=torch.float32)
        cn = torch.empty_like(hn)
        for li in range(L):
            G_, Cs_, Y_ = saved[3 * li:3 * li + 3]
            Cv = Cs_.view(B, T, H * ndir)
            for d in range(ndir):
                t_last = 0 if d else T - 1
                hn[li * ndir + d] = Y_[:, t_last, d * H:(d + 1) * H]
                cn[li * ndir + d] = Cv[:, t_last, d * H:(d + 1) * H]
        # h_n is differentiable (its gradient joins the layer output's at the last step); c_n's
        # gradient would need an initial cell gradient the BPTT kernels do not take: refused
        # loudly in backward.  Unused outputs arrive as None (no materialised zero tensors).
        ctx.set_materialize_grads(False)
        ctx.out_shape = h.shape
        return h, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn=None, dcn=None):
        H, L, ndir = ctx.H, ctx.L, ctx.ndir
        nw, GL = 4 * ndir, 4 * H * ndir
        t = ctx.saved_tensors
        inputs, saved, weights = t[:L], t[L:4 * L], t[4 * L:]
        if dcn is not None and bool(dcn.ne(0).any()):
            raise NotImplementedError("gradient through c_n of the HIP LSTM is not supported "
                                      "(the BPTT starts from a zero cell gradient)")
        if dy is None:
            dy = torch.zeros(ctx.out_shape, device=t[0].device, dtype=torch.float32)
        dy = _need(dy, "lstm grad").clone()
        B, T = dy.shape[0], dy.shape[1]
        N = B * T
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        dW = [None] * len(weights)
        dx = None
        for li in range(L - 1, -1, -1):
            G, Cs, Y = saved[3 * li:3 * li + 3]
            w = weights[nw * li:nw * li + nw]
            xin = inputs[li]
            din = xin.shape[-1]
            if dhn is not None:  # h_n[li, d] is Y_li at t = T-1 (forward) / t = 0 (reverse)
                for d in range(ndir):
                    dy[:, 0 if d else T - 1, d * H:(d + 1) * H] += dhn[li * ndir + d]
            if ndir == 2:
                check(l.mlvae_lstm_bwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(dy),
                                       _p(xbuf), xbuf.numel() * 4, _p(err), _stream()), "lstm_bwd")
            else:
                check(l.mlvae_lstm1_bwd(_prec(), B, T, H, _p(w[1]), _p(G), _p(Cs), _p(dy), None,
                                        _p(xbuf), xbuf.numel() * 4, _p(err), _stream()), "lstm1_bwd")
            dx = torch.empty(B, T, din, device=dy.device, dtype=torch.float32)
            for d in range(ndir):
                wi = w[4 * d]
                gemm(0, 0, N, din, 4 * H, _p(G, 4 * H * d), GL, _p(wi), din, _p(dx), din,
                     beta=1.0 if d else 0.0)
                gwi = torch.empty_like(wi)
                gemm(1, 0, 4 * H, din, N, _p(G, 4 * H * d), GL, _p(xin), din, _p(gwi), din)
                gwh = torch.empty_like(w[4 * d + 1])
                # dW_hh = sum_t dG_t^T h_{t-1} (forward) / h_{t+1} (reverse): time-shifted B rows
                gemm(1, 0, 4 * H, H, N, _p(G, 4 * H * d), GL, _p(Y, H * d), H * ndir, _p(gwh), H,
                     kshift_T=T, kshift=1 if d else -1)
                gbi = torch.empty_like(w[4 * d + 2])
                gbh = torch.empty_like(w[4 * d + 3])
                colsum(N, 4 * H, _p(G, 4 * H * d), GL, _p(gbi), _p(gbh))
                base = nw * li + 4 * d
                dW[base:base + 4] = [gwi, gwh, gbi, gbh]
            if li > 0 and ctx.seeds[li - 1] is not None:
                _dropout(dx, dx, ctx.seeds[li - 1], ctx.dropout, ctx.shard)
            dy = dx
        if int(err.item()) != 0:
            raise RuntimeError("LSTM recurrence hand-off timed out")
        return (dx, None, None, None, None, None, *dW)


def lstm(x, lstm_module, train):
    """Run an nn.LSTM's parameters (batch_first, uni- or bidirectional) through the HIP
    recurrence; its own forward is not used."""
    if not lstm_module.batch_first:
        raise ValueError("the HIP LSTM path is batch_first only (as every reference LSTM)")
    H, L = lstm_module.hidden_size, lstm_module.num_layers
    ndir = 2 if lstm_module.bidirectional else 1
    weights = []
    for li in range(L):
        for sfx in ("", "_reverse")[:ndir]:
            for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                weights.append(getattr(lstm_module, f"{kind}_l{li}{sfx}"))
    p = float(lstm_module.dropout) if train else 0.0
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
    return LSTMFn.apply(x, H, L, ndir, p, seed, *weights)[0]


def lstm_full(x, lstm_module, train, seed=None):
    """nn.LSTM's whole forward on the HIP recurrence: (output, (h_n, c_n)).  seed: the
    inter-layer dropout's Philox key (drawn from torch's generator when None)."""
    if not lstm_module.batch_first:
        raise ValueError("the HIP LSTM path is batch_first only (as every reference LSTM)")
    H, L = lstm_module.hidden_size, lstm_module.num_layers
    ndir = 2 if lstm_module.bidirectional else 1
    weights = [getattr(lstm_module, f"{kind}_l{li}{sfx}") for li in range(L)
               for sfx in ("", "_reverse")[:ndir] for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    p = float(lstm_module.dropout) if train else 0.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
    out, hn, cn = LSTMFn.apply(x, H, L, ndir, p, seed, *weights)
    return out, (hn, cn)


class LSTMPairFn(torch.autograd.Function):
    """Two independent unidirectional nn.LSTM(batch_first=True) stacks of one shape over the same
    input (the joint recipes' recogniser and detector, ref:src/modules/phoneme_recognizer.py:13,
    boundary_detector.py:19): per layer two input-projection GEMMs into the column halves of one
    G [N, 8H] and ONE paired recurrence launch (mlvae_lstm_pair_fwd / _bwd), so the two stacks'
    latency-bound step chains overlap.  No dropout inside a paired stack.  weights = the
    layer-major list [w_ih, w_hh, b_ih, b_hh] of stack a + the same of stack b, * L."""

    @staticmethod
    def forward(ctx, x, H, L, *weights):
        x = _need(x, "lstm input")
        B, T, _ = x.shape
        N = B * T
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        saved, inputs = [], []
        h = x
        for li in range(L):
            w = [_need(t, "lstm weight") for t in weights[8 * li:8 * li + 8]]
            # layer 0: both stacks read x; above it stack s reads its own half of Y (lda = 2H)
            din, lda = (h.shape[-1], h.shape[-1]) if li == 0 else (H, 2 * H)
            G = torch.empty(N, 8 * H, device=x.device, dtype=torch.float32)
            for s in range(2):
                wi, _, bi, bh = w[4 * s:4 * s + 4]
                gemm(0, 1, N, 4 * H, din, _p(h, H * s if li else 0), lda, _p(wi), din,
                     _p(G, 4 * H * s), 8 * H, bias1=_p(bi), bias2=_p(bh))
            Cs = torch.empty(N, 2 * H, device=x.device, dtype=torch.float32)
            Y = torch.empty(B, T, 2 * H, device=x.device, dtype=torch.float32)
            check(l.mlvae_lstm_pair_fwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(Y), None,
                                        _p(xbuf), xbuf.numel() * 4, _p(err), _stream()), "lstm_pair_fwd")
            inputs.append(h)
            saved += [G, Cs, Y]
            h = Y
        ctx.save_for_backward(*inputs, *saved, *weights)
        ctx.H, ctx.L = H, L
        ctx.set_materialize_grads(False)  # an output outside the loss arrives as None
        return h[..., :H].contiguous(), h[..., H:].contiguous()

    @staticmethod
    def backward(ctx, dya, dyb):
        H, L = ctx.H, ctx.L
        GL = 8 * H
        t = ctx.saved_tensors
        inputs, saved, weights = t[:L], t[L:4 * L], t[4 * L:]
        B, T = inputs[0].shape[0], inputs[0].shape[1]
        N = B * T
        dev = inputs[0].device
        dy = torch.zeros(B, T, 2 * H, device=dev, dtype=torch.float32)
        for s, g in enumerate((dya, dyb)):
            if g is not None:
                dy[..., H * s:H * (s + 1)] = _need(g, "lstm grad")
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        dW = [None] * len(weights)
        dx = None
        for li in range(L - 1, -1, -1):
            G, Cs, Y = saved[3 * li:3 * li + 3]
            w = weights[8 * li:8 * li + 8]
            xin = inputs[li]
            din, ldx = (xin.shape[-1], xin.shape[-1]) if li == 0 else (H, 2 * H)
            check(l.mlvae_lstm_pair_bwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(dy), None,
                                        _p(xbuf), xbuf.numel() * 4, _p(err), _stream()), "lstm_pair_bwd")
            if li > 0:  # the dgrads fill the column halves of the layer below's dy
                dx = torch.empty(B, T, 2 * H, device=dev, dtype=torch.float32)
            elif ctx.needs_input_grad[0]:  # dx = dx_a + dx_b
                dx = torch.empty(B, T, din, device=dev, dtype=torch.float32)
            else:
                dx = None
            for s in range(2):
                wi = w[4 * s]
                if li > 0:
                    gemm(0, 0, N, H, 4 * H, _p(G, 4 * H * s), GL, _p(wi), H, _p(dx, H * s), 2 * H)
                elif dx is not None:
                    gemm(0, 0, N, din, 4 * H, _p(G, 4 * H * s), GL, _p(wi), din, _p(dx), din,
                         beta=1.0 if s else 0.0)
                gwi = torch.empty_like(wi)
                gemm(1, 0, 4 * H, din, N, _p(G, 4 * H * s), GL, _p(xin, H * s if li else 0), ldx,
                     _p(gwi), din)
                gwh = torch.empty_like(w[4 * s + 1])
                # dW_hh = sum_t dG_t^T h_{t-1}: both stacks run forward in time
                gemm(1, 0, 4 * H, H, N, _p(G, 4 * H * s), GL, _p(Y, H * s), 2 * H, _p(gwh), H,
                     kshift_T=T, kshift=-1)
                gbi = torch.empty_like(w[4 * s + 2])
                gbh = torch.empty_like(w[4 * s + 3])
                colsum(N, 4 * H, _p(G, 4 * H * s), GL, _p(gbi), _p(gbh))
                base = 8 * li + 4 * s
                dW[base:base + 4] = [gwi, gwh, gbi, gbh]
            dy = dx
        if int(err.item()) != 0:
            raise RuntimeError("LSTM recurrence hand-off timed out")
        return (dx, None, None, *dW)


def lstm_pair_ok(lstm_a, lstm_b, train):
    """True where lstm_pair can run the two modules as one paired recurrence."""
    for m in (lstm_a, lstm_b):
        if not isinstance(m, torch.nn.LSTM) or not m.batch_first or m.bidirectional or m.proj_size:
            return False
    if (lstm_a.input_size, lstm_a.hidden_size, lstm_a.num_layers) != \
            (lstm_b.input_size, lstm_b.hidden_size, lstm_b.num_layers):
        return False
    if lstm_a.hidden_size % 4:
        return False
    return not train or (float(lstm_a.dropout) == 0.0 and float(lstm_b.dropout) == 0.0)


def lstm_pair(x, lstm_a, lstm_b, train):
    """Two unidirectional nn.LSTMs of one shape over the same input x, their recurrences paired
    in one launch per layer: (out_a, out_b), each [B, T, H]."""
    if not lstm_pair_ok(lstm_a, lstm_b, train):
        raise ValueError("lstm_pair: two batch_first unidirectional nn.LSTMs of equal input_size, "
                         "hidden_size (a multiple of 4) and num_layers, without projection and "
                         "without dropout in training")
    H, L = lstm_a.hidden_size, lstm_a.num_layers
    weights = [getattr(m, f"{kind}_l{li}") for li in range(L) for m in (lstm_a, lstm_b)
               for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return LSTMPairFn.apply(x, H, L, *weights)


def bilstm(x, lstm_module, train):
    """The decoder's bidirectional nn.LSTM (ref:src/modules/decoder.py:22)."""
    return lstm(x, lstm_module, train)


# --------------------------------------------------------------------------- MD-VAE upstream losses
def _md_err():
    dev = torch.cuda.current_device()
    e = _ws.get((dev, "md_err"))
    if e is None:
        e = torch.zeros(1, device="cuda", dtype=torch.int32)
        _ws[(dev, "md_err")] = e
    return e


def _raise_md(err):
    code = int(err.item()) & 6  # bit 32 is the pi path's (raise_pi_err)
    if code:
        err.bitwise_and_(~6)
        raise AssertionError(
            "phoneme-recogniser targets: " +
            ("boundaries do not give one segment per phoneme from frame 0 " if code & 2 else "") +
            ("phoneme id outside [0, n_phonemes + 2)" if code & 4 else "") +
            " (ref:src/modules/phoneme_recognizer.py:65-67)")


class PhnBceFn(torch.autograd.Function):
    """PhonemeRecognizer.compute_losses on libmlvae (ref:src/modules/phoneme_recognizer.py:35-81):
    [B,T,C] BCE-with-logits against the boundary-expanded canonical phoneme sequence."""

    @staticmethod
    def forward(ctx, out, feat_lens, phn, phn_lens, boundary):
        out = _need(out, "recogniser output")
        B, T, C = out.shape
        fl = _need(feat_lens.to(out.device, torch.float32), "feat_lens")
        pl = _need(phn_lens.to(out.device, torch.float32), "phn_lens")
        bnd = _need(boundary.to(out.device, torch.float32), "boundary_seqs")
        ids = phn.to(out.device, torch.int64).contiguous()
        loss = torch.empty_like(out)
        err = _md_err()
        check(lib().mlvae_phn_bce(B, T, C, _p(out), C, _p(fl), ids.data_ptr(), ids.shape[1], _p(pl),
                                  _p(bnd), _p(loss), None, None, _p(err), _stream()), "phn_bce")
        _raise_md(err)  # the reference asserts on the host too (one sync per batch, not per utterance)
        ctx.save_for_backward(out, fl, ids, pl, bnd)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        out, fl, ids, pl, bnd = ctx.saved_tensors
        B, T, C = out.shape
        dloss = _need(dloss, "grad")
        dout = torch.empty_like(out)
        err = _md_err()
        check(lib().mlvae_phn_bce(B, T, C, _p(out), C, _p(fl), ids.data_ptr(), ids.shape[1], _p(pl),
                                  _p(bnd), None, _p(dloss), _p(dout), _p(err), _stream()), "phn_bce_bwd")
        return dout, None, None, None, None


def phn_bce(out, feat_lens, phn, phn_lens, boundary):
    return PhnBceFn.apply(out, feat_lens, phn, phn_lens, boundary)


class BoundaryHeadsFn(torch.autograd.Function):
    """BoundaryDetector after its FC heads (ref:src/modules/boundary_detector.py:42-97): Softplus
    + 1e-5, Beta(1, 9) KL, ten Kumaraswamy draws; returns (boundary_v, bce, kld).  u = the ten
    U(0,1) draws [10, B, T] (None: Philox keyed by seed and element index)."""

    @staticmethod
    def forward(ctx, za, zb, y, u, seed):
        za, zb = _need(za, "alpha head"), _need(zb, "beta head")
        y = _need(y.to(za.device, torch.float32), "boundary_seqs")
        u = _need(u, "uniforms") if u is not None else None
        v, bce, kld = torch.empty_like(za), torch.empty_like(za), torch.empty_like(za)
        sh = current_shard() if u is None else None  # injected draws are the shard's own
        if sh is not None:
            B, T, _ = _bt(za.shape, "boundary_heads")
            check(lib().mlvae_boundary_fwd_rows(B, T, _p(za), _p(zb), _p(y), None, seed, sh.map(B),
                                                _p(v), _p(bce), _p(kld), _stream()), "boundary_fwd_rows")
        else:
            check(lib().mlvae_boundary_fwd(za.numel(), _p(za), _p(zb), _p(y), _p(u) if u is not None else None,
                                           seed, 0, _p(v), _p(bce), _p(kld), _stream()), "boundary_fwd")
        ctx.save_for_backward(za, zb, y, *([u] if u is not None else []))
        ctx.seed, ctx.has_u, ctx.shard = seed, u is not None, sh
        return v, bce, kld

    @staticmethod
    def backward(ctx, dv, dbce, dkld):
        t = ctx.saved_tensors
        za, zb, y = t[:3]
        u = t[3] if ctx.has_u else None
        grads = [None if g is None else _need(g, "grad") for g in (dv, dbce, dkld)]
        dza, dzb = torch.empty_like(za), torch.empty_like(zb)
        gp = [(_p(g) if g is not None else None) for g in grads]
        if ctx.shard is not None:
            B, T, _ = _bt(za.shape, "boundary_heads")
            check(lib().mlvae_boundary_bwd_rows(B, T, _p(za), _p(zb), _p(y), None, ctx.seed,
                                                ctx.shard.map(B), *gp, _p(dza), _p(dzb), _stream()),
                  "boundary_bwd_rows")
            return dza, dzb, None, None, None
        check(lib().mlvae_boundary_bwd(za.numel(), _p(za), _p(zb), _p(y), _p(u) if u is not None else None,
                                       ctx.seed, 0, *gp, _p(dza), _p(dzb), _stream()), "boundary_bwd")
        return dza, dzb, None, None, None


def boundary_heads(za, zb, boundary, u=None):
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if u is None else 0
    return BoundaryHeadsFn.apply(za, zb, boundary, u, seed)


# --------------------------------------------------------------------------- MD-VAE pi path
PI_ERR_LABEL = 32  # bit of the _md_err word: a decoded frame label outside {-1, 0, 1}


def raise_pi_err():
    """Read the device error word's pi bit (one host sync): ValueError as
    Categorical.log_prob raises for a label outside its support."""
    err = _md_err()
    code = int(err.item())
    if code & PI_ERR_LABEL:
        err.bitwise_and_(~PI_ERR_LABEL)
        raise ValueError("pi_nll: frame label outside {0, 1} (-1 = past the utterance's end) "
                         "(ref:src/models/MD_VAE/model.py:149)")


class PiSampleFn(torch.autograd.Function):
    """sampled_pi of the MD-VAE forward (ref:src/models/MD_VAE/model.py:122-127): the one-hot
    [1 - label, label] of a Categorical(logits) draw (train) or the argmax (eval).  u = the
    U(0,1) draw per frame (None: Philox keyed by seed and frame index)."""

    @staticmethod
    def forward(ctx, logits, train, u, seed):
        logits = _need(logits, "pi_logits")
        if logits.shape[-1] != 2:
            raise ValueError(f"pi_sample: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        n = _rows(logits)
        if u is not None:
            u = _need(u, "uniforms")
            if u.numel() != n:
                raise ValueError(f"pi_sample: {u.numel()} uniforms for {n} frames")
        out = torch.empty_like(logits)
        sh = current_shard() if (train and u is None) else None
        if sh is not None:
            B, T, _ = _bt(logits.shape, "pi_sample")
            check(lib().mlvae_pi_sample_rows(B, T, 1, _p(logits), None, seed, sh.map(B), 1, _p(out),
                                             _stream()), "pi_sample_rows")
            ctx.mark_non_differentiable(out)
            return out
        check(lib().mlvae_pi_sample(n, _p(logits), _p(u) if u is not None else None, seed, 0,
                                    1 if train else 0, _p(out), _stream()), "pi_sample")
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        return None, None, None, None


def pi_sample(logits, train, u=None):
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (train and u is None) else 0
    return PiSampleFn.apply(logits, bool(train), u, seed)


class PiNllFn(torch.autograd.Function):
    """pi_nll_loss = -Categorical(logits).log_prob(labels) (ref:src/models/MD_VAE/model.py:145-149)
    on the decode kernel's int32 frame labels [.., T] (-1 past T_i counts as 0)."""

    @staticmethod
    def forward(ctx, logits, labels):
        logits = _need(logits, "pi_logits")
        if logits.shape[-1] != 2:
            raise ValueError(f"pi_nll: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        if not (labels.is_cuda and labels.dtype == torch.int32):
            raise TypeError(f"pi_nll labels: expected an int32 HIP tensor, got {labels.dtype} on "
                            f"{labels.device}")
        labels = labels.contiguous()
        n = _rows(logits)
        if labels.numel() != n:
            raise ValueError(f"pi_nll: {labels.numel()} labels for {n} frames")
        nll = torch.empty(logits.shape[:-1], device=logits.device, dtype=torch.float32)
        check(lib().mlvae_pi_nll_fwd(n, _p(logits), labels.data_ptr(), _p(nll), _p(_md_err()),
                                     _stream()), "pi_nll_fwd")
        ctx.save_for_backward(logits, labels)
        ctx.mark_non_differentiable(labels)
        return nll

    @staticmethod
    def backward(ctx, dnll):
        logits, labels = ctx.saved_tensors
        dnll = _need(dnll, "pi_nll grad")
        dlogits = torch.empty_like(logits)
        check(lib().mlvae_pi_nll_bwd(_rows(logits), _p(logits), labels.data_ptr(), _p(dnll),
                                     _p(dlogits), _stream()), "pi_nll_bwd")
        return dlogits, None


def pi_nll(logits, labels, sync=True):
    """sync=False leaves the error word unread (no host sync): the caller reads it with
    raise_pi_err() where it syncs anyway (the MD-VAE recipe: at the stage's end)."""
    nll = PiNllFn.apply(logits, labels)
    if sync:
        raise_pi_err()
    return nll


# --------------------------------------------------------------------------- MD_VAE_sfl
class PiSampleKFn(torch.autograd.Function):
    """K Categorical(logits) draws per frame (ref:src/models/MD_VAE_sfl/model.py:147-152) as
    one-hot rows [K, .., 2]; draw k of frame i uses uniform k n + i of u [K, ..] or of the
    Philox stream.  Eval (train false) is the argmax: K must be 1."""

    @staticmethod
    def forward(ctx, logits, K, train, u, seed):
        if K < 1 or (not train and K != 1):
            raise ValueError(f"pi_sample_k: K must be >= 1 in train and 1 in eval (the argmax), got {K}")
        if logits.shape[-1] != 2:
            raise ValueError(f"pi_sample_k: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        logits = _need(logits, "pi_logits")
        n = _rows(logits)
        if u is not None:
            u = _need(u, "uniforms")
            if u.numel() != K * n:
                raise ValueError(f"pi_sample_k: {u.numel()} uniforms for {K} draws of {n} frames")
        out = torch.empty((K,) + tuple(logits.shape), device=logits.device, dtype=torch.float32)
        sh = current_shard() if (train and u is None) else None
        if sh is not None:
            B, T, _ = _bt(logits.shape, "pi_sample_k")
            check(lib().mlvae_pi_sample_rows(B, T, K, _p(logits), None, seed, sh.map(B), 1, _p(out),
                                             _stream()), "pi_sample_rows")
            ctx.mark_non_differentiable(out)
            return out
        check(lib().mlvae_pi_sample_k(n, K, _p(logits), _p(u) if u is not None else None, seed, 0,
                                      1 if train else 0, _p(out), _stream()), "pi_sample_k")
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        return None, None, None, None, None


def pi_sample_k(logits, K, train, u=None):
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (train and u is None) else 0
    return PiSampleKFn.apply(logits, int(K), bool(train), u, seed)


class SflLossesFn(torch.autograd.Function):
    """The score-function terms of MD_VAE_sfl (ref:src/models/MD_VAE_sfl/model.py:170-186), the K
    draws summed and divided by K: rif = (reward - baseline) * nll of the draw, the negative
    entropy of Categorical(logits), and the baseline's squared error against the reward
    -(w_recon mean(recon) + w_kld mean(kld) + w_nll pi_nll).  Gradients go to logits and baseline
    only: the reference detaches the reward, and the baseline inside rif."""

    @staticmethod
    def forward(ctx, logits, sampled_pi, recon, kld, pi_nll, baseline, w_recon, w_kld, w_nll):
        if logits.shape[-1] != 2:
            raise ValueError(f"sfl_losses: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        frames = tuple(logits.shape[:-1])
        if sampled_pi.dim() != logits.dim() + 1 or tuple(sampled_pi.shape[1:]) != tuple(logits.shape):
            raise ValueError(f"sfl_losses: sampled_pi must be [K, {', '.join(map(str, logits.shape))}], "
                             f"got {tuple(sampled_pi.shape)}")
        K = sampled_pi.shape[0]
        if K < 1:
            raise ValueError("sfl_losses: no draws (K = 0)")
        for name, t in (("recon_loss", recon), ("vae_kld_loss", kld)):
            if tuple(t.shape[:-1]) != (K,) + frames or t.shape[-1] < 1:
                raise ValueError(f"sfl_losses: {name} must be [K, .., C] over {(K,) + frames}, "
                                 f"got {tuple(t.shape)}")
        for name, t in (("pi_nll_loss", pi_nll), ("baseline", baseline)):
            if tuple(t.shape) != frames:
                raise ValueError(f"sfl_losses: {name} must be {frames}, got {tuple(t.shape)}")
        logits, sampled_pi = _need(logits, "pi_logits"), _need(sampled_pi, "sampled_pi")
        recon, kld = _need(recon, "recon_loss"), _need(kld, "vae_kld_loss")
        pi_nll, baseline = _need(pi_nll, "pi_nll_loss"), _need(baseline, "baseline")
        n = _rows(logits)
        reward = torch.empty((K,) + frames, device=logits.device, dtype=torch.float32)
        rif, ent, bl = (torch.empty(frames, device=logits.device, dtype=torch.float32) for _ in range(3))
        check(lib().mlvae_sfl_fwd(n, K, recon.shape[-1], kld.shape[-1], _p(logits), _p(sampled_pi),
                                  _p(recon), _p(kld), _p(pi_nll), _p(baseline), float(w_recon),
                                  float(w_kld), float(w_nll), _p(reward), _p(rif), _p(ent), _p(bl),
                                  _stream()), "sfl_fwd")
        ctx.save_for_backward(logits, sampled_pi, reward, baseline)
        return rif, ent, bl

    @staticmethod
    def backward(ctx, d_rif, d_ent, d_bl):
        logits, sampled_pi, reward, baseline = ctx.saved_tensors
        d_rif, d_ent, d_bl = (_need(g, "sfl_losses grad") for g in (d_rif, d_ent, d_bl))
        dlogits, dbaseline = torch.empty_like(logits), torch.empty_like(baseline)
        check(lib().mlvae_sfl_bwd(_rows(logits), sampled_pi.shape[0], _p(logits), _p(sampled_pi),
                                  _p(reward), _p(baseline), _p(d_rif), _p(d_ent), _p(d_bl),
                                  _p(dlogits), _p(dbaseline), _stream()), "sfl_bwd")
        return dlogits, None, None, None, None, dbaseline, None, None, None


def sfl_losses(logits, sampled_pi, recon, kld, pi_nll, baseline, w_recon, w_kld, w_nll):
    """(rif, neg_entropy, baseline_loss), each shaped like logits[..., 0]."""
    return SflLossesFn.apply(logits, sampled_pi, recon, kld, pi_nll, baseline, w_recon, w_kld, w_nll)


# --------------------------------------------------------------------------- LSTM_FC frame-level head
FLVL_ERR_LABEL = 64  # bit of the _md_err word: a valid frame's MD label is neither 0 nor 1


def raise_flvl_err():
    """Read the device error word's frame-label bit (one host sync): ValueError as
    MDMetricStats raises for a non-binary label sequence."""
    err = _md_err()
    code = int(err.item())
    if code & FLVL_ERR_LABEL:
        err.bitwise_and_(~FLVL_ERR_LABEL)
        raise ValueError("flvl_md_head: frame-level MD label outside {0, 1} in a valid frame "
                         "(Only binary input values are supported)")


class FlvlMdHeadFn(torch.autograd.Function):
    """The LSTM_FC recipe after the FCBlock's last hidden layer (ref:src/models/LSTM_FC/
    model.py:30-61): logits = h W^T + b, the class-weighted BCE-with-logits per frame and class
    against [1 - label, label], the argmax (-1 past each length) and the per-utterance MD counts
    (both correct, both mispronounced, missed, false alarm), one kernel; the backward is one
    kernel and the fixed-order sum of its partials."""

    @staticmethod
    def forward(ctx, h, weight, bias, labels, lens, pw0, pw1):
        if h.dim() != 3:
            raise ValueError(f"flvl_md_head: h must be [B, T, E], got {tuple(h.shape)}")
        B, T, E = h.shape
        if E < 1:
            raise ValueError("flvl_md_head: h has no features (E = 0)")
        if tuple(weight.shape) != (2, E) or tuple(bias.shape) != (2,):
            raise ValueError(f"flvl_md_head: weight must be [2, {E}] and bias [2], got "
                             f"{tuple(weight.shape)} and {tuple(bias.shape)}")
        if tuple(labels.shape) != (B, T):
            raise ValueError(f"flvl_md_head: labels must be [{B}, {T}], got {tuple(labels.shape)}")
        if tuple(lens.shape) != (B,):
            raise ValueError(f"flvl_md_head: lens must be [{B}], got {tuple(lens.shape)}")
        if labels.device != h.device:
            raise TypeError(f"flvl_md_head labels: on {labels.device}, h on {h.device}")
        h, weight, bias = _need(h, "flvl_md_head h"), _need(weight, "flvl_md_head weight"), \
            _need(bias, "flvl_md_head bias")
        labels = _need(labels.to(torch.float32), "flvl_md_head labels")
        lens = _need(lens.to(h.device, torch.float32), "flvl_md_head lens")
        logits = torch.empty(B, T, 2, device=h.device, dtype=torch.float32)
        loss_e = torch.empty_like(logits)
        pred = torch.empty(B, T, device=h.device, dtype=torch.int32)
        counts = torch.empty(B, 4, device=h.device, dtype=torch.int32)
        check(lib().mlvae_flvl_head_fwd(B, T, E, _p(h), _p(weight), _p(bias), _p(labels), _p(lens),
                                        pw0, pw1, _p(logits), _p(loss_e), pred.data_ptr(),
                                        counts.data_ptr(), _p(_md_err()), _stream()), "flvl_head_fwd")
        ctx.save_for_backward(h, weight, logits, labels)
        ctx.pw = (pw0, pw1)
        ctx.mark_non_differentiable(logits, pred, counts)
        return logits, loss_e, pred, counts

    @staticmethod
    def backward(ctx, dlogits, dloss_e, dpred, dcounts):
        h, weight, logits, labels = ctx.saved_tensors
        B, T, E = h.shape
        dloss_e = _need(dloss_e, "flvl_md_head grad")
        dh, dw = torch.empty_like(h), torch.empty_like(weight)
        db = torch.empty(2, device=h.device, dtype=torch.float32)
        if B * T == 0:
            return dh, dw.zero_(), db.zero_(), None, None, None, None
        l = lib()
        ws = _workspace(l.mlvae_flvl_head_workspace_size(B, T, E), "flvl")
        check(l.mlvae_flvl_head_bwd(B, T, E, _p(h), _p(weight), _p(logits), _p(labels), _p(dloss_e),
                                    ctx.pw[0], ctx.pw[1], _p(dh), _p(dw), _p(db), _p(ws),
                                    ws.numel() * 4, _stream()), "flvl_head_bwd")
        return dh, dw, db, None, None, None, None


def flvl_md_head(h, weight, bias, labels, lens, pos_weight):
    """(logits [B,T,2], loss_e [B,T,2], pred int32 [B,T], counts int32 [B,4]) from h [B,T,E], the
    final Linear's weight [2,E] and bias [2], the frame labels [B,T] (0 / 1) and the relative
    lengths [B]; pos_weight = (class 0, class 1).  Gradients reach h, weight and bias through
    loss_e only.  A label outside {0, 1} in a valid frame sets a bit of the device error word:
    raise_flvl_err() reads it (where the counts are read, not per batch)."""
    pw0, pw1 = (float(v) for v in pos_weight)
    return FlvlMdHeadFn.apply(h, weight, bias, labels, lens, pw0, pw1)


# --------------------------------------------------------------------------- upstream-module scoring
SCORE_ERR_SEGMENTS = 128  # bit of the _md_err word: the flags do not give L_i segments from frame 0
SCORE_ERR_K = 256         # bit of the _md_err word: more boundaries asked for than frames (k > T_i)


def raise_score_err():
    """Read the device error word's scoring bits (one host sync) and clear them alone:
    AssertionError as plvl_phn_acc_scoring's asserts, RuntimeError as torch.topk's."""
    err = _md_err()
    code = int(err.item()) & (SCORE_ERR_SEGMENTS | SCORE_ERR_K)
    if code:
        err.bitwise_and_(~(SCORE_ERR_SEGMENTS | SCORE_ERR_K))
        if code & SCORE_ERR_SEGMENTS:
            raise AssertionError(
                "phn_acc_counts: boundary_seqs do not give one segment per phoneme from frame 0 "
                "(ref:src/utils/metric_stats/phn_acc_metric_stats.py:69-73)")
        raise RuntimeError("boundary_topk: k out of range: fa_boundary_seqs has more boundaries than "
                           "the utterance has frames (ref:src/models/test_b_ind_classifier/model.py:61)")


def _score_lens(lens, B, dev, what):
    if tuple(lens.shape) != (B,):
        raise ValueError(f"{what}: lengths must be [{B}], got {tuple(lens.shape)}")
    return _need(lens.to(dev, torch.float32), f"{what} lengths")


def _score_seq(x, shape, dev, dtype, what):
    if tuple(x.shape) != shape:
        raise ValueError(f"{what} must be {list(shape)}, got {tuple(x.shape)}")
    if x.device != dev:
        raise TypeError(f"{what}: on {x.device}, the scored output on {dev}")
    return x.to(dtype).contiguous()


def phn_acc_counts(out, feat_lens, flvl_targets, plvl_targets=None, phn_lens=None, boundary_seqs=None):
    """int32 [B, 4] = (flvl_correct, T_i, plvl_correct, L_i) per utterance of the recogniser
    output out [B, T, C]: what PhnAccMetricStats.append_counts takes.  flvl_targets [B, T] and
    plvl_targets [B, L] are phoneme ids, boundary_seqs [B, T] the 0/1 flags that open the phoneme
    segments; plvl_targets None gives (.., .., 0, 0).  Stays on the device; a bad flag count sets
    a bit of the device error word (raise_score_err)."""
    if out.dim() != 3 or out.shape[2] < 1:
        raise ValueError(f"phn_acc_counts: out must be [B, T, C] with C >= 1, got {tuple(out.shape)}")
    out = _need(out.detach(), "phn_acc_counts out")
    B, T, C = out.shape
    dev = out.device
    fl = _score_lens(feat_lens, B, dev, "phn_acc_counts feat")
    ft = _score_seq(flvl_targets, (B, T), dev, torch.int64, "phn_acc_counts flvl_targets")
    pt = pl = bnd = None
    L = 0
    if plvl_targets is not None:
        if boundary_seqs is None or phn_lens is None:
            raise ValueError("boundary_seqs must be provided when plvl_targets is not None")
        if plvl_targets.dim() != 2:
            raise ValueError(f"phn_acc_counts plvl_targets must be [B, L], got {tuple(plvl_targets.shape)}")
        L = plvl_targets.shape[1]
        pt = _score_seq(plvl_targets, (B, L), dev, torch.int64, "phn_acc_counts plvl_targets")
        pl = _score_lens(phn_lens, B, dev, "phn_acc_counts phoneme")
        bnd = _score_seq(boundary_seqs, (B, T), dev, torch.float32, "phn_acc_counts boundary_seqs")
    counts = torch.zeros(B, 4, device=dev, dtype=torch.int32)
    check(lib().mlvae_phn_acc(B, T, C, L, _p(out), C, _p(fl), ft.data_ptr(),
                              pt.data_ptr() if pt is not None else None,
                              _p(pl) if pl is not None else None,
                              _p(bnd) if bnd is not None else None, counts.data_ptr(),
                              _p(_md_err()), _stream()), "phn_acc")
    return counts


def boundary_topk(boundary_v, feat_lens, fa_boundary_seqs):
    """pred int32 [B, T]: 1 at the k_i largest of boundary_v[i, :T_i] (0 elsewhere, -1 past T_i),
    k_i = the ones of fa_boundary_seqs[i] -- the reference's per-utterance torch.topk, for the
    whole batch on the device.  k_i > T_i sets a bit of the device error word (raise_score_err)."""
    if boundary_v.dim() != 2:
        raise ValueError(f"boundary_topk: boundary_v must be [B, T], got {tuple(boundary_v.shape)}")
    v = _need(boundary_v.detach(), "boundary_topk boundary_v")
    B, T = v.shape
    limit = lib().mlvae_boundary_topk_max_frames()
    if T > limit:
        raise ValueError(f"boundary_topk: {T} frames, the kernel ranks a row of at most {limit}")
    fl = _score_lens(feat_lens, B, v.device, "boundary_topk feat")
    fa = _score_seq(fa_boundary_seqs, (B, T), v.device, torch.float32, "boundary_topk fa_boundary_seqs")
    pred = torch.empty(B, T, device=v.device, dtype=torch.int32)
    k = torch.empty(B, device=v.device, dtype=torch.int32)
    check(lib().mlvae_boundary_topk(B, T, _p(v), _p(fl), _p(fa), pred.data_ptr(), k.data_ptr(),
                                    _p(_md_err()), _stream()), "boundary_topk")
    return pred


def boundary_counts(pred, targets, feat_lens):
    """int32 [B, 3] = (correct, n_pred, n_target) per utterance: boundary_scoring's two-pointer
    walk of the frames with pred == 1 (int32 [B, T]) over the segments of the 0/1 targets [B, T].
    What BoundaryMetricStats.append_counts takes; stays on the device."""
    if pred.dim() != 2 or pred.dtype != torch.int32 or not pred.is_cuda:
        raise TypeError(f"boundary_counts: pred must be an int32 [B, T] HIP tensor, got {pred.dtype} "
                        f"{tuple(pred.shape)} on {pred.device}")
    pred = pred.contiguous()
    B, T = pred.shape
    fl = _score_lens(feat_lens, B, pred.device, "boundary_counts feat")
    tgt = _score_seq(targets, (B, T), pred.device, torch.float32, "boundary_counts targets")
    counts = torch.zeros(B, 3, device=pred.device, dtype=torch.int32)
    check(lib().mlvae_boundary_score(B, T, pred.data_ptr(), _p(tgt), _p(fl), counts.data_ptr(),
                                     _stream()), "boundary_score")
    return counts


# --------------------------------------------------------------------------- GMM-VAE / H-VAE
class GmmLatentFn(torch.autograd.Function):
    """GMM-VAE latent block on the stacked head output P = [pm | plv | m | lv | logits]
    (ref:src/modules/gmm_vae.py:24-67): returns z, per-element KL and the straight-through
    hard Gumbel-softmax weights.  expo = the Exp(1) draws [.., N] (None: library Philox)."""

    @staticmethod
    def forward(ctx, P, eps, expo, N, Z, tau, seed):
        P, eps = _need(P, "gmm heads"), _need(eps, "eps")
        expo = _need(expo, "expo") if expo is not None else None
        rows = _rows(P)
        z = torch.empty(*P.shape[:-1], N * Z, device=P.device, dtype=torch.float32)
        kl = torch.empty_like(z)
        w = torch.empty(*P.shape[:-1], N, device=P.device, dtype=torch.float32)
        ysoft = torch.empty_like(w)
        sh = current_shard() if expo is None else None
        if sh is not None:
            B, T, _ = _bt(P.shape, "gmm_latent")
            check(lib().mlvae_gmm_latent_fwd_rows(B, T, N, Z, _p(P), P.shape[-1], _p(eps), None, seed,
                                                  sh.map(B), tau, _p(z), _p(kl), _p(w), _p(ysoft),
                                                  _stream()), "gmm_latent_fwd_rows")
            ctx.save_for_backward(P, eps, ysoft)
            ctx.shape = (N, Z, tau)
            return z, kl, w
        check(lib().mlvae_gmm_latent_fwd(rows, N, Z, _p(P), P.shape[-1], _p(eps),
                                         _p(expo) if expo is not None else None, seed, 0, tau,
                                         _p(z), _p(kl), _p(w), _p(ysoft), _stream()),
              "gmm_latent_fwd")
        ctx.save_for_backward(P, eps, ysoft)
        ctx.shape = (N, Z, tau)
        return z, kl, w

    @staticmethod
    def backward(ctx, dz, dkl, dw):
        P, eps, ysoft = ctx.saved_tensors
        N, Z, tau = ctx.shape
        opt = lambda t, n: _need(t, n) if t is not None else None
        dz, dkl, dw = opt(dz, "dz"), opt(dkl, "dkl"), opt(dw, "dw")
        dP = torch.empty_like(P)
        nz = lambda t: _p(t) if t is not None else None
        check(lib().mlvae_gmm_latent_bwd(_rows(P), N, Z, _p(P), P.shape[-1], _p(eps), _p(ysoft),
                                         tau, nz(dz), nz(dkl), nz(dw), _p(dP), P.shape[-1],
                                         _stream()), "gmm_latent_bwd")
        return dP, None, None, None, None, None, None


class ApplyWeightFn(torch.autograd.Function):
    """y[.., c] = sum_n w[.., n] x[.., n*C + c] (ref:src/utils/data_utils.py:32-64)."""

    @staticmethod
    def forward(ctx, x, w):
        x, w = _need(x, "apply_weight x"), _need(w, "apply_weight weight")
        N = w.shape[-1]
        C = x.shape[-1] // N
        rows = _rows(w)
        if x.numel() != rows * N * C:
            raise ValueError(f"apply_weight: x {tuple(x.shape)} does not match weight {tuple(w.shape)}")
        y = torch.empty(*w.shape[:-1], C, device=x.device, dtype=torch.float32)
        check(lib().mlvae_apply_weight_fwd(rows, N, C, _p(x), N * C, _p(w), _p(y), C, _stream()),
              "apply_weight_fwd")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _need(dy, "apply_weight grad")
        N = w.shape[-1]
        C = x.shape[-1] // N
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        check(lib().mlvae_apply_weight_bwd(_rows(w), N, C, _p(x), N * C, _p(w), _p(dy), C,
                                           _p(dx) if dx is not None else None, N * C,
                                           _p(dw) if dw is not None else None, _stream()),
              "apply_weight_bwd")
        return dx, dw


def apply_weight(x, weight):
    """(B,T,N*C) or (B,T,N,C) weighted by (B,T,N) -> (B,T,C)."""
    B, T, N = weight.shape
    return ApplyWeightFn.apply(x.reshape(B, T, -1), weight)


class HvaeLatentFn(torch.autograd.Function):
    """The H-VAE's latent stretch in one launch (csrc/hvae.hip; ref:src/modules/h_vae.py:21-72):
    ml = [mean_v | log_var_v], P = the GMM's stacked heads, pi [.., 2] -> the mixed (mean, log_var,
    sampled_h, kl) [.., Z] and the hard Gumbel-softmax weights [.., N].  ml = pi = None is the
    GMM-only mode: (None, None, collapsed h, collapsed kl, weights).  expo = the Exp(1) draws
    [.., N] (None: library Philox under `seed`, mapped inside an ops.shard context)."""

    @staticmethod
    def forward(ctx, ml, P, pi, eps_v, eps_g, expo, N, Z, tau, seed):
        hier = ml is not None
        ctx.set_materialize_grads(False)  # an unused output's cotangent reaches the kernel as NULL
        P, eps_g = _need(P, "gmm heads"), _need(eps_g, "eps_g")
        expo = _need(expo, "expo") if expo is not None else None
        if hier:
            ml, pi, eps_v = _need(ml, "ml"), _need(pi, "pi"), _need(eps_v, "eps_v")
        rows = _rows(P)
        lead = P.shape[:-1]
        new = lambda n: torch.empty(*lead, n, device=P.device, dtype=torch.float32)
        h, kl, w, ysoft = new(Z), new(Z), new(N), new(N)
        mean, log_var = (new(Z), new(Z)) if hier else (None, None)
        nz = lambda t: _p(t) if t is not None else None
        ldml = ml.shape[-1] if hier else 0
        sh = current_shard() if expo is None else None
        if sh is not None:
            B, T, _ = _bt(P.shape, "hvae_latent")
            check(lib().mlvae_hvae_latent_fwd_rows(
                B, T, N, Z, nz(ml), ldml, _p(P), P.shape[-1], nz(pi), nz(eps_v), _p(eps_g), None, seed,
                sh.map(B), tau, nz(mean), nz(log_var), _p(h), _p(kl), _p(w), _p(ysoft), _stream()),
                "hvae_latent_fwd_rows")
        else:
            check(lib().mlvae_hvae_latent_fwd(
                rows, N, Z, nz(ml), ldml, _p(P), P.shape[-1], nz(pi), nz(eps_v), _p(eps_g), nz(expo),
                seed, 0, tau, nz(mean), nz(log_var), _p(h), _p(kl), _p(w), _p(ysoft), _stream()),
                "hvae_latent_fwd")
        ctx.hier = hier
        ctx.save_for_backward(*((ml, pi, eps_v) if hier else ()), P, eps_g, w, ysoft)
        ctx.shape = (N, Z, tau)
        return mean, log_var, h, kl, w

    @staticmethod
    def backward(ctx, d_mean, d_log_var, d_h, d_kl, d_w):
        if ctx.hier:
            ml, pi, eps_v, P, eps_g, w, ysoft = ctx.saved_tensors
        else:
            (P, eps_g, w, ysoft), ml, pi, eps_v = ctx.saved_tensors, None, None, None
        N, Z, tau = ctx.shape
        nz = lambda t: _p(t) if t is not None else None
        keep =[None if t is None else _need(t, "grad") for t in (d_mean, d_log_var, d_h, d_kl, d_w)]
        dP = torch.empty_like(P)
        if P.shape[-1] > 4 * N * Z + N:
            dP[..., 4 * N * Z + N:] = 0  # columns past the heads: never written by the kernel
        dml = torch.empty(*P.shape[:-1], 2 * Z, device=P.device, dtype=torch.float32) if ctx.hier else None
        dpi = torch.empty_like(pi) if ctx.hier and ctx.needs_input_grad[2] else None
        check(lib().mlvae_hvae_latent_bwd(
            _rows(P), N, Z, nz(ml), ml.shape[-1] if ctx.hier else 0, _p(P), P.shape[-1], nz(pi),
            nz(eps_v), _p(eps_g), _p(w), _p(ysoft), tau, *[nz(t) for t in keep], nz(dml), _p(dP),
            P.shape[-1], nz(dpi), _stream()), "hvae_latent_bwd")
        if ctx.hier and ml.shape[-1] != 2 * Z:
            wide = torch.zeros_like(ml)
            wide[..., :2 * Z] = dml
            dml = wide
        return dml, dP, dpi, None, None, None, None, None, None, None


def _latent_shapes(what, P, eps_g, expo, N, Z):
    if not (1 <= N <= 64) or Z < 1:
        raise ValueError(f"{what}: N must be in [1, 64] and Z >= 1, got N={N} Z={Z}")
    if P.shape[-1] < 4 * N * Z + N:
        raise ValueError(f"{what}: the stacked heads need {4 * N * Z + N} columns, got {tuple(P.shape)}")
    lead = tuple(P.shape[:-1])
    if tuple(eps_g.shape) != lead + (N * Z,):
        raise ValueError(f"{what}: eps_g {tuple(eps_g.shape)} is not {lead + (N * Z,)}")
    if expo is not None and tuple(expo.shape) != lead + (N,):
        raise ValueError(f"{what}: expo {tuple(expo.shape)} is not {lead + (N,)}")
    return lead


def hvae_latent(ml, P, pi, eps_v, eps_g, expo, N, Z, tau, seed):
    """(mean, log_var, sampled_h, kl) [.., Z] and gmm_weight [.., N] of the Hierarchical VAE from
    its two encoders' head outputs, one launch each way (HvaeLatentFn)."""
    lead = _latent_shapes("hvae_latent", P, eps_g, expo, N, Z)
    if ml is None or pi is None or eps_v is None:
        raise ValueError("hvae_latent: ml, pi and eps_v are required (gmm_collapsed is the GMM-only form)")
    if tuple(ml.shape[:-1]) != lead or ml.shape[-1] < 2 * Z:
        raise ValueError(f"hvae_latent: ml {tuple(ml.shape)} is not {lead} + (>= {2 * Z},)")
    if tuple(pi.shape) != lead + (2,):
        raise ValueError(f"hvae_latent: pi {tuple(pi.shape)} is not {lead + (2,)}")
    if tuple(eps_v.shape) != lead + (Z,):
        raise ValueError(f"hvae_latent: eps_v {tuple(eps_v.shape)} is not {lead + (Z,)}")
    return HvaeLatentFn.apply(ml, P, pi, eps_v, eps_g, expo, N, Z, tau, seed)


def gmm_collapsed(P, eps, expo, N, Z, tau, seed):
    """(weighted_h, weighted_loss) [.., Z] and gmm_weight [.., N] of the GMM-VAE: apply_weight of
    GmmLatentFn's sampled_h and loss with its own weights, in one launch each way."""
    _latent_shapes("gmm_collapsed", P, eps, expo, N, Z)
    return HvaeLatentFn.apply(None, P, None, None, eps, expo, N, Z, tau, seed)[2:]


# --------------------------------------------------------------------------- HMM / CTC sequence lattice
ALIGN_ERR_SHORT = 512    # bit of the _md_err word: HMM chain infeasible (T_i < U_i, U_i = 0 or T_i = 0)
ALIGN_ERR_CLASS = 1024   # bit of the _md_err word: a phoneme id whose state class is outside [0, C)
ALIGN_ERR_BLANK = 2048   # bit of the _md_err word: CTC, a target class equal to blank
TOPO_HMM, TOPO_CTC = 0, 1


def raise_align_err():
    """Read the device error word's lattice bits (one host sync) and clear them alone:
    AssertionError naming the condition (what the aligner's own asserts would have said per batch)."""
    err = _md_err()
    mask = ALIGN_ERR_SHORT | ALIGN_ERR_CLASS | ALIGN_ERR_BLANK
    code = int(err.item()) & mask
    if code:
        err.bitwise_and_(~mask)
        what = []
        if code & ALIGN_ERR_SHORT:
            what.append("an utterance has fewer frames than HMM states (or no states, or no frames)")
        if code & ALIGN_ERR_CLASS:
            what.append("a phoneme id expands to a state class outside [0, C)")
        if code & ALIGN_ERR_BLANK:
            what.append("a CTC target class equals the blank index")
        raise AssertionError("sequence lattice: " + "; ".join(what))


class CenterLogSoftmaxFn(torch.autograd.Function):
    """y = log_softmax(x - mean_t(x), dim=-1) over [B, T, C], the mean over all T rows of the
    padded batch (ref:src/models/HMM_DNN_ALI/model.py:43-44)."""

    @staticmethod
    def forward(ctx, x):
        x = _need(x, "center_log_softmax x")
        B, T, C = x.shape
        y = torch.empty_like(x)
        ws = _workspace(lib().mlvae_center_lsm_workspace_size(B, C), "center_lsm")
        check(lib().mlvae_center_lsm_fwd(B, T, C, _p(x), _p(y), _p(ws), ws.numel() * 4, _stream()),
              "center_lsm_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        B, T, C = y.shape
        dy = _need(dy, "center_log_softmax grad")
        dx = torch.empty_like(y)
        ws = _workspace(lib().mlvae_center_lsm_workspace_size(B, C), "center_lsm")
        check(lib().mlvae_center_lsm_bwd(B, T, C, _p(dy), _p(y), _p(dx), _p(ws), ws.numel() * 4,
                                         _stream()), "center_lsm_bwd")
        return dx


def center_log_softmax(x):
    if x.dim() != 3 or x.shape[2] < 1:
        raise ValueError(f"center_log_softmax: x must be [B, T, C] with C >= 1, got {tuple(x.shape)}")
    return CenterLogSoftmaxFn.apply(x)


def _lattice_args(what, pout, lens, phns, phn_lens, spp):
    if pout.dim() != 3 or pout.shape[2] < 1:
        raise ValueError(f"{what}: pout must be [B, T, C] with C >= 1, got {tuple(pout.shape)}")
    if phns.dim() != 2 or phns.shape[0] != pout.shape[0]:
        raise ValueError(f"{what}: phns must be [{pout.shape[0]}, L], got {tuple(phns.shape)}")
    spp = int(spp)
    if spp < 1:
        raise ValueError(f"{what}: states per phoneme must be >= 1, got {spp}")
    B, L = phns.shape
    fl = _score_lens(lens, B, pout.device, f"{what} frame")
    pl = _score_lens(phn_lens, B, pout.device, f"{what} phoneme")
    ids = phns.to(pout.device, torch.int64).contiguous()
    return fl, pl, ids, L, spp


class LatticeFn(torch.autograd.Function):
    """score [B] = log of the summed path likelihoods of the HMM or CTC chain (csrc/align.hip).
    The forward runs the alpha chain (and, when a gradient is wanted, the beta chain beside it);
    the backward is the occupancy pass with g = the incoming gradient."""

    @staticmethod
    def forward(ctx, pout, fl, ids, pl, spp, topo, blank):
        pout = _need(pout, "lattice pout")
        B, T, C = pout.shape
        L = ids.shape[1]
        limit = lib().mlvae_lattice_max_nodes()
        nodes = L * spp * (2 if topo == TOPO_CTC else 1) + (1 if topo == TOPO_CTC else 0)
        if nodes > limit:
            raise ValueError(f"lattice: {L} phonemes of {spp} states give a chain of {nodes} nodes, "
                             f"the kernel holds at most {limit}")
        need_beta = bool(ctx.needs_input_grad[0])
        nbytes = lib().mlvae_lattice_workspace_size(B, T, L, spp, topo)
        ws = torch.empty(max(nbytes // 4, 1), device=pout.device, dtype=torch.float32)
        score = torch.empty(B, device=pout.device, dtype=torch.float32)
        check(lib().mlvae_lattice_fb(B, T, C, L, _p(pout), C, _p(fl), ids.data_ptr(), _p(pl), spp, topo,
                                     blank, int(need_beta), _p(score), _p(ws), ws.numel() * 4,
                                     _p(_md_err()), _stream()), "lattice_fb")
        if need_beta:
            ctx.save_for_backward(pout, fl, ids, pl, ws)
        ctx.cfg = (spp, topo, blank)
        return score

    @staticmethod
    def backward(ctx, g):
        pout, fl, ids, pl, ws = ctx.saved_tensors
        spp, topo, blank = ctx.cfg
        B, T, C = pout.shape
        g = _need(g, "lattice grad")
        dpout = torch.empty_like(pout)
        check(lib().mlvae_lattice_grad(B, T, C, ids.shape[1], _p(pout), C, _p(fl), ids.data_ptr(), _p(pl),
                                       spp, topo, blank, _p(g), _p(ws), ws.numel() * 4, _p(dpout), C,
                                       _stream()), "lattice_grad")
        return dpout, None, None, None, None, None, None


def hmm_forward(pout, lens, phns, phn_lens, spp):
    """score [B]: log sum over the left-to-right HMM paths of exp(sum_t pout[b, t, state_t]) --
    the forward score SpeechBrain's HMMAligner trains on.  pout [B, T, C] log-probabilities, phns
    [B, L] phoneme ids (each expands into spp states of classes id * spp + j), lens / phn_lens the
    relative lengths.  Autograd: d score_b / d pout = the state occupancies.  An infeasible
    utterance or a bad id scores 0 and sets a bit of the device error word (raise_align_err)."""
    fl, pl, ids, _, spp = _lattice_args("hmm_forward", pout, lens, phns, phn_lens, spp)
    return LatticeFn.apply(pout, fl, ids, pl, spp, TOPO_HMM, 0)


def ctc_nll(pout, lens, phns, phn_lens, spp, blank):
    """nll [B] = -log p(targets | pout) of the CTC chain over the spp-expanded phonemes:
    F.ctc_loss(reduction='none', zero_infinity=True) per utterance, on log-probabilities pout.
    The gradient is the true partial derivative with respect to pout (minus the occupancies), not
    torch's, which folds the log-softmax backward in: chained through a log-softmax both agree."""
    fl, pl, ids, _, spp = _lattice_args("ctc_nll", pout, lens, phns, phn_lens, spp)
    blank = int(blank)
    if not 0 <= blank < pout.shape[2]:
        raise ValueError(f"ctc_nll: blank {blank} outside [0, {pout.shape[2]})")
    return -LatticeFn.apply(pout, fl, ids, pl, spp, TOPO_CTC, blank)


def hmm_viterbi(pout, lens, phns, phn_lens, spp):
    """(vscore [B] fp32, align [B, T] int32): the best HMM path's score (float64 sums, rounded
    once) and its state position per frame in [0, U_i), -1 past T_i; a tie keeps "stay".  No
    gradient; errors as hmm_forward's."""
    fl, pl, ids, L, spp = _lattice_args("hmm_viterbi", pout, lens, phns, phn_lens, spp)
    pout = _need(pout.detach(), "hmm_viterbi pout")
    B, T, C = pout.shape
    limit = lib().mlvae_lattice_max_nodes()
    if L * spp > limit:
        raise ValueError(f"hmm_viterbi: {L} phonemes of {spp} states, the kernel holds at most {limit} states")
    ws = _workspace(lib().mlvae_hmm_viterbi_workspace_size(B, T), "hmm_viterbi")
    vscore = torch.empty(B, device=pout.device, dtype=torch.float32)
    align = torch.empty(B, T, device=pout.device, dtype=torch.int32)
    check(lib().mlvae_hmm_viterbi(B, T, C, L, _p(pout), C, _p(fl), ids.data_ptr(), _p(pl), spp,
                                  _p(vscore), align.data_ptr(), _p(ws), ws.numel() * 4, _p(_md_err()),
                                  _stream()), "hmm_viterbi")
    return vscore, align


def align_counts(align, lens, phns, phn_lens, spp, phn_ends, samples_per_frame):
    """int32 [B, 2] = (frames correct, T_i) per utterance of a Viterbi alignment (int32 [B, T] state
    positions): frame t is correct iff the phoneme of its state, phns[i, align[i, t] // spp], is
    the phoneme of the ground-truth segment that holds it -- the first k with t * samples_per_frame
    < phn_ends[i, k] (exclusive ends in samples), the last phoneme if none.  What
    AlignAccMetricStats.append_counts takes; stays on the device."""
    if align.dim() != 2 or align.dtype != torch.int32 or not align.is_cuda:
        raise TypeError(f"align_counts: align must be an int32 [B, T] HIP tensor, got {align.dtype} "
                        f"{tuple(align.shape)} on {align.device}")
    align = align.contiguous()
    B, T = align.shape
    if phns.dim() != 2 or phns.shape[0] != B or tuple(phn_ends.shape) != tuple(phns.shape):
        raise ValueError(f"align_counts: phns and phn_ends must be [{B}, L], got {tuple(phns.shape)} "
                         f"and {tuple(phn_ends.shape)}")
    spp, spf = int(spp), int(samples_per_frame)
    if spp < 1 or spf < 1:
        raise ValueError(f"align_counts: spp {spp} and samples_per_frame {spf} must be >= 1")
    L = phns.shape[1]
    fl = _score_lens(lens, B, align.device, "align_counts frame")
    pl = _score_lens(phn_lens, B, align.device, "align_counts phoneme")
    ids = phns.to(align.device, torch.int64).contiguous()
    ends = phn_ends.to(align.device, torch.int64).contiguous()
    counts = torch.zeros(B, 2, device=align.device, dtype=torch.int32)
    check(lib().mlvae_align_counts(B, T, L, align.data_ptr(), _p(fl), ids.data_ptr(), _p(pl), spp,
                                   ends.data_ptr(), spf, counts.data_ptr(), _stream()), "align_counts")
    return counts


# --------------------------------------------------------------------------- CTC evaluation (csrc/ctc_eval.hip)
CTC_ERR_PAIR = 4096  # bit of the _md_err word: pronounced and canonical sequences differ in length


def raise_ctc_eval_err():
    """Read the device error word's CTC-evaluation bits (one host sync) and clear them alone."""
    err = _md_err()
    mask = ALIGN_ERR_CLASS | ALIGN_ERR_BLANK | CTC_ERR_PAIR
    code = int(err.item()) & mask
    if code:
        err.bitwise_and_(~mask)
        what = []
        if code & ALIGN_ERR_CLASS:
            what.append("a phoneme id is outside [0, C)")
        if code & ALIGN_ERR_BLANK:
            what.append("a target phoneme equals the blank index")
        if code & CTC_ERR_PAIR:
            what.append("gt_phn_seq and gt_cnncl_seq of an utterance differ in length")
        raise AssertionError("CTC evaluation: " + "; ".join(what))


class LogSoftmaxFn(torch.autograd.Function):
    """y = log_softmax(x, dim=-1) over [.., C]."""

    @staticmethod
    def forward(ctx, x):
        x = _need(x, "log_softmax x")
        C = x.shape[-1]
        y = torch.empty_like(x)
        check(lib().mlvae_log_softmax_fwd(x.numel() // C, C, _p(x), _p(y), _stream()), "log_softmax_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        C = y.shape[-1]
        dy = _need(dy, "log_softmax grad")
        dx = torch.empty_like(y)
        check(lib().mlvae_log_softmax_bwd(y.numel() // C, C, _p(dy), _p(y), _p(dx), _stream()),
              "log_softmax_bwd")
        return dx


def log_softmax(x):
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"log_softmax: x must be [.., C] with C >= 1, got {tuple(x.shape)}")
    return LogSoftmaxFn.apply(x)


def _rows_ld(pout, what):
    """(tensor, ld) of a float32 HIP [B, T, C] whose rows lie ld >= C floats apart (a column slice
    of a wider contiguous tensor is taken as it is); anything else is made contiguous."""
    if pout.dim() != 3 or pout.shape[2] < 1:
        raise ValueError(f"{what}: pout must be [B, T, C] with C >= 1, got {tuple(pout.shape)}")
    if not (pout.is_cuda and pout.dtype == torch.float32):
        raise TypeError(f"{what} pout: expected a float32 HIP tensor, got {pout.dtype} on {pout.device} "
                        "(the HIP path has no CPU fallback)")
    B, T, C = pout.shape
    s0, s1, s2 = pout.stride()
    if B and T and s2 == 1 and s1 >= C and (s0 == T * s1 or B == 1):
        return pout, s1
    return pout.contiguous(), C


def _blank_arg(what, blank, C):
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f"{what}: blank {blank} outside [0, {C})")
    return blank


def ctc_greedy_decode(pout, lens, blank):
    """(pred [B, T] int32 padded with -1, pred_len [B] int32): SpeechBrain's ctc_greedy_decode for
    the whole batch on the device -- per frame t < T_i the argmax over the classes (a tie keeps the
    lowest), consecutive repeats merged, blanks dropped.  No gradient."""
    pout, ld = _rows_ld(pout.detach(), "ctc_greedy_decode")
    B, T, C = pout.shape
    blank = _blank_arg("ctc_greedy_decode", blank, C)
    fl = _score_lens(lens, B, pout.device, "ctc_greedy_decode frame")
    pred = torch.empty(B, T, device=pout.device, dtype=torch.int32)
    pred_len = torch.empty(B, device=pout.device, dtype=torch.int32)
    check(lib().mlvae_ctc_greedy_decode(B, T, C, _p(pout), ld, _p(fl), blank, pred.data_ptr(),
                                        pred_len.data_ptr(), _stream()), "ctc_greedy_decode")
    return pred, pred_len


def _ref_pair(what, phns, phn_lens, cnncls, cnncl_lens, dev):
    """refs int64 [B, 2, L] and ref_lens fp32 [B, 2] of the pronounced and the canonical sequences."""
    if phns.dim() != 2 or tuple(cnncls.shape) != tuple(phns.shape):
        raise ValueError(f"{what}: phns and cnncls must both be [B, L], got {tuple(phns.shape)} and "
                         f"{tuple(cnncls.shape)}")
    B = phns.shape[0]
    refs = torch.stack([phns.to(dev, torch.int64), cnncls.to(dev, torch.int64)], dim=1).contiguous()
    ref_lens = torch.stack([_score_lens(phn_lens, B, dev, f"{what} phoneme"),
                            _score_lens(cnncl_lens, B, dev, f"{what} canonical")], dim=1).contiguous()
    return refs, ref_lens


def edit_align(pred, pred_len, phns, phn_lens, cnncls, cnncl_lens):
    """(ali [B, 2, L] int32, ops [B, 2, 4] int32): the decoded sequences pred[i, :pred_len[i]]
    aligned by edit distance to the pronounced (index 0) and the canonical (index 1) phonemes.
    ali = the hypothesis token at every reference position, -1 for a deletion and past L_i
    (insertions dropped, align_sequences(ignore_insertion=True)); ops = (insertions, deletions,
    substitutions, L_i).  Tie rule: include/mlvae.h; the definition is tests/ctc_np.py."""
    if pred.dim() != 2 or pred.dtype != torch.int32 or not pred.is_cuda:
        raise TypeError(f"edit_align: pred must be an int32 [B, T] HIP tensor, got {pred.dtype} "
                        f"{tuple(pred.shape)} on {pred.device}")
    B, Tp = pred.shape
    if tuple(pred_len.shape) != (B,) or pred_len.dtype != torch.int32 or pred_len.device != pred.device:
        raise TypeError(f"edit_align: pred_len must be an int32 [{B}] tensor on {pred.device}")
    if phns.shape[0] != B:
        raise ValueError(f"edit_align: phns must be [{B}, L], got {tuple(phns.shape)}")
    pred, pred_len = pred.contiguous(), pred_len.contiguous()
    refs, ref_lens = _ref_pair("edit_align", phns, phn_lens, cnncls, cnncl_lens, pred.device)
    L = refs.shape[2]
    limit = lib().mlvae_edit_align_max_ref()
    if L > limit:
        raise ValueError(f"edit_align: a reference of {L} tokens, the kernel holds at most {limit}")
    ws = _workspace(lib().mlvae_edit_align_workspace_size(B, L, Tp), "edit_align")
    ali = torch.empty(B, 2, L, device=pred.device, dtype=torch.int32)
    ops_ = torch.empty(B, 2, 4, device=pred.device, dtype=torch.int32)
    check(lib().mlvae_edit_align(B, L, Tp, refs.data_ptr(), _p(ref_lens), pred.data_ptr(),
                                 pred_len.data_ptr(), ali.data_ptr(), ops_.data_ptr(), _p(ws),
                                 ws.numel() * 4, _stream()), "edit_align")
    return ali, ops_


def ctc_md_counts(ali, phns, phn_lens, cnncls, cnncl_lens):
    """int32 [B, 8] per utterance from edit_align's ali [B, 2, L], over the alignment to the
    pronounced sequence, with pred_md = (ali != cnncl) (a deletion counts as a predicted
    mispronunciation) and gt_md = (phn != cnncl): (both correct, both mispronounced, missed, false
    alarm) as MDMetricStats counts them, then (canonical positions, of them recognised wrongly,
    mispronounced positions, of them recognised wrongly): per_scoring's correct_per / misp_per.
    Stays on the device; sequences of unequal length set a bit of the error word."""
    if ali.dim() != 3 or ali.shape[1] != 2 or ali.dtype != torch.int32 or not ali.is_cuda:
        raise TypeError(f"ctc_md_counts: ali must be an int32 [B, 2, L] HIP tensor, got {ali.dtype} "
                        f"{tuple(ali.shape)} on {ali.device}")
    B, _, L = ali.shape
    if tuple(phns.shape) != (B, L):
        raise ValueError(f"ctc_md_counts: phns must be [{B}, {L}], got {tuple(phns.shape)}")
    refs, ref_lens = _ref_pair("ctc_md_counts", phns, phn_lens, cnncls, cnncl_lens, ali.device)
    ali = ali.contiguous()
    counts = torch.zeros(B, 8, device=ali.device, dtype=torch.int32)
    check(lib().mlvae_ctc_md_counts(B, L, refs.data_ptr(), _p(ref_lens), ali.data_ptr(), counts.data_ptr(),
                                    _p(_md_err()), _stream()), "ctc_md_counts")
    return counts


def ctc_viterbi(pout, lens, phns, phn_lens, blank):
    """(vscore [B] fp32, boundary [B, T] int32, infeasible [B] int32): the best path of the CTC
    chain over phns (one state per phoneme) -- what the reference asks the ctc_segmentation package
    for.  boundary is 1 at frame 0 and at the first frame of every later phoneme (exactly L_i
    ones), 0 elsewhere, -1 past T_i; a chain without a path scores 0, sets infeasible and marks
    frames 0 .. min(L_i, T_i) - 1.  Tie order: stay, next, skip; the final blank over the last
    phoneme.  No gradient; a bad id sets a bit of the error word (raise_ctc_eval_err)."""
    pout, ld = _rows_ld(pout.detach(), "ctc_viterbi")
    B, T, C = pout.shape
    blank = _blank_arg("ctc_viterbi", blank, C)
    if phns.dim() != 2 or phns.shape[0] != B:
        raise ValueError(f"ctc_viterbi: phns must be [{B}, L], got {tuple(phns.shape)}")
    L = phns.shape[1]
    limit = lib().mlvae_lattice_max_nodes()
    if 2 * L + 1 > limit:
        raise ValueError(f"ctc_viterbi: {L} phonemes give a chain of {2 * L + 1} nodes, the kernel holds "
                         f"at most {limit}")
    fl = _score_lens(lens, B, pout.device, "ctc_viterbi frame")
    pl = _score_lens(phn_lens, B, pout.device, "ctc_viterbi phoneme")
    ids = phns.to(pout.device, torch.int64).contiguous()
    ws = _workspace(lib().mlvae_ctc_viterbi_workspace_size(B, T), "ctc_viterbi")
    vscore = torch.empty(B, device=pout.device, dtype=torch.float32)
    boundary = torch.empty(B, T, device=pout.device, dtype=torch.int32)
    infeasible = torch.empty(B, device=pout.device, dtype=torch.int32)
    check(lib().mlvae_ctc_viterbi(B, T, C, L, _p(pout), ld, _p(fl), ids.data_ptr(), _p(pl), blank,
                                  _p(vscore), boundary.data_ptr(), infeasible.data_ptr(), _p(ws),
                                  ws.numel() * 4, _p(_md_err()), _stream()), "ctc_viterbi")
    return vscore, boundary, infeasible


# ---- the feature front end (csrc/fbank.hip)
_fbank_tables = {}


def _fbank_table(dev, sample_rate, win, n_fft, n_mels, f_min, f_max):
    """The windowed twiddles and mel filters of one geometry on one device: filled once on the host
    (mlvae_fbank_table, float64 rounded to fp32) and kept."""
    key = (dev, sample_rate, win, n_fft, n_mels, float(f_min), float(f_max))
    t = _fbank_tables.get(key)
    if t is None:
        nbytes = lib().mlvae_fbank_table_size(win, n_fft, n_mels)
        if nbytes == 0:
            check(1, "fbank")
        host = torch.empty(nbytes // 4, dtype=torch.float32)
        check(lib().mlvae_fbank_table(sample_rate, win, n_fft, n_mels, float(f_min), float(f_max),
                                      host.data_ptr(), nbytes), "fbank_table")
        t = _fbank_tables[key] = host.to(dev)
    return t


def fbank(wav, wav_lens=None, *, sample_rate=16000, hop_length=10, win_length=25, n_fft=400, n_mels=40,
          f_min=0.0, f_max=None):
    """(feats [B, Tmax, 3 n_mels] fp32, frames [B] int32) of the padded waveforms wav [B, N]:
    log-mel filterbank, deltas and delta-deltas as SpeechBrain's Fbank(deltas=True) computes them
    per utterance (include/mlvae.h, mlvae_fbank), Tmax = 1 + N // hop, rows past an utterance's
    frames[b] = 1 + N_b // hop exact zeros.  wav_lens: None (every row N samples), an integer
    tensor of sample counts N_b, or a floating tensor of relative lengths (N_b = round(N len_b));
    samples at or past N_b are never read.  hop_length / win_length in milliseconds.  No autograd:
    the front end has no parameters; an input that requires grad raises."""
    if wav.dim() != 2:
        raise ValueError(f"fbank: wav must be [B, N], got {tuple(wav.shape)}")
    if wav.requires_grad:
        raise RuntimeError("fbank: the front end has no backward; detach the waveform")
    wav = _need(wav, "fbank wav")
    B, N = wav.shape
    dev = wav.device
    sample_rate, n_fft, n_mels = int(sample_rate), int(n_fft), int(n_mels)
    # samples from SpeechBrain's milliseconds
    hop, win = (int(round(sample_rate / 1000.0 * ms)) for ms in (hop_length, win_length))
    f_max = sample_rate / 2 if f_max is None else f_max
    if wav_lens is None:
        ns = torch.full((B,), N, device=dev, dtype=torch.int32)
    else:
        wav_lens = torch.as_tensor(wav_lens)
        if tuple(wav_lens.shape) != (B,):
            raise ValueError(f"fbank: wav_lens must be [{B}], got {tuple(wav_lens.shape)}")
        if wav_lens.is_floating_point():
            ns = torch.round(wav_lens.to(dev, torch.float64) * N).to(torch.int32)
        else:
            ns = wav_lens.to(dev, torch.int32)
        ns = ns.contiguous()
    # geometry errors come from the library (status 1 with its message)
    table = _fbank_table(dev, sample_rate, win, n_fft, n_mels, f_min, f_max)
    Tmax = 1 + N // max(hop, 1)
    feats = torch.empty(B, Tmax, 3 * n_mels, device=dev, dtype=torch.float32)
    frames = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        ws = _workspace(lib().mlvae_fbank_workspace_size(B, N, hop, n_mels), "fbank")
        check(lib().mlvae_fbank(B, N, _p(wav) if N else None, N, ns.data_ptr(), hop, win, n_fft, n_mels,
                                _p(table), _p(feats), 3 * n_mels, frames.data_ptr(), _p(ws),
                                ws.numel() * 4, _stream()), "fbank")
    return feats, frames


# ---- the Kaldi-compatible front end and per-speaker CMVN (csrc/kaldi_fbank.hip)
_kaldi_tables = {}


def _kaldi_table(dev, sample_rate, L, P, n_mels):
    """The Hamming-windowed twiddles and mel filters of one geometry on one device: filled once on
    the host (mlvae_kaldi_fbank_table, float64 rounded to fp32) and kept."""
    key = (dev, sample_rate, L, P, n_mels)
    t = _kaldi_tables.get(key)
    if t is None:
        nbytes = lib().mlvae_kaldi_fbank_table_size(L, P, n_mels)
        if nbytes == 0:
            check(1, "kaldi_fbank")
        host = torch.empty(nbytes // 4, dtype=torch.float32)
        check(lib().mlvae_kaldi_fbank_table(sample_rate, L, P, n_mels, host.data_ptr(), nbytes),
              "kaldi_fbank_table")
        t = _kaldi_tables[key] = host.to(dev)
    return t


def kaldi_fbank(wav, wav_lens=None, *, sample_rate=16000, hop_length=20, win_length=25, n_mels=40,
                deltas=True):
    """(feats [B, Tmax, 3 n_mels] fp32, frames [B] int32) of the padded waveforms wav [B, N]: Kaldi's
    compute-fbank-feats (Hamming, snip-edges=false, no dither) + add-deltas as restated in
    include/mlvae.h (mlvae_kaldi_fbank), before CMVN.  Tmax = (N + hop/2) // hop, rows past an
    utterance's frames[b] = (N_b + hop/2) // hop exact zeros; deltas=False gives the n_mels statics.
    wav_lens as ops.fbank: None (every row N samples), an integer tensor of sample counts N_b, or a
    floating tensor of relative lengths (N_b = round(N len_b)); samples at or past N_b are never
    read.  hop_length / win_length in milliseconds.  No autograd: an input that requires grad
    raises."""
    if wav.dim() != 2:
        raise ValueError(f"kaldi_fbank: wav must be [B, N], got {tuple(wav.shape)}")
    if wav.requires_grad:
        raise RuntimeError("kaldi_fbank: the front end has no backward; detach the waveform")
    wav = _need(wav, "kaldi_fbank wav")
    B, N = wav.shape
    dev = wav.device
    sample_rate, n_mels = int(sample_rate), int(n_mels)
    hop, L = (int(round(sample_rate / 1000.0 * ms)) for ms in (hop_length, win_length))
    P = 1 << max(L - 1, 0).bit_length()  # the power of two at or above L
    if wav_lens is None:
        ns = torch.full((B,), N, device=dev, dtype=torch.int32)
    else:
        wav_lens = torch.as_tensor(wav_lens)
        if tuple(wav_lens.shape) != (B,):
            raise ValueError(f"kaldi_fbank: wav_lens must be [{B}], got {tuple(wav_lens.shape)}")
        if wav_lens.is_floating_point():
            ns = torch.round(wav_lens.to(dev, torch.float64) * N).to(torch.int32)
        else:
            ns = wav_lens.to(dev, torch.int32)
        ns = ns.contiguous()
    # geometry errors come from the library (status 1 with its message)
    table = _kaldi_table(dev, sample_rate, L, P, n_mels)
    Tmax = (N + hop // 2) // max(hop, 1)
    D = (3 if deltas else 1) * n_mels
    feats = torch.empty(B, Tmax, D, device=dev, dtype=torch.float32)
    frames = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        ws = _workspace(lib().mlvae_kaldi_fbank_workspace_size(B, N, hop, n_mels), "kaldi_fbank")
        check(lib().mlvae_kaldi_fbank(B, N, _p(wav) if N else None, N, ns.data_ptr(), hop, L, P, n_mels,
                                      int(bool(deltas)), _p(table), _p(feats) if Tmax else None, D,
                                      frames.data_ptr(), _p(ws), ws.numel() * 4, _stream()), "kaldi_fbank")
    return feats, frames


def _cmvn_args(feats, frames, spk, stats, who):
    if feats.dim() != 3:
        raise ValueError(f"{who}: feats must be [B, T, D], got {tuple(feats.shape)}")
    if not (feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous()):
        raise TypeError(f"{who}: feats must be a contiguous float32 HIP tensor "
                        "(the HIP path has no CPU fallback)")
    B, T, D = feats.shape
    if not (stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous() and
            stats.dim() == 2 and stats.shape[1] == 2 * D + 1):
        raise TypeError(f"{who}: stats must be a contiguous float64 HIP tensor [S, {2 * D + 1}]")
    dev = feats.device
    frames = torch.as_tensor(frames).to(dev, torch.int32).contiguous()
    spk = torch.as_tensor(spk).to(dev, torch.int32).contiguous()
    if tuple(frames.shape) != (B,) or tuple(spk.shape) != (B,):
        raise ValueError(f"{who}: frames and spk must be [{B}]")
    return B, T, D, stats.shape[0], frames, spk


def _raise_cmvn(err, who):
    code = int(err.item())  # one host sync: corpus preparation, not the training step
    if code & 1:
        raise ValueError(f"{who}: speaker id outside [0, S)")
    if code & 2:
        raise ValueError(f"{who}: a speaker of the batch has no accumulated statistics")


def cmvn_accumulate(stats, feats, frames, spk):
    """Adds the batch's per-speaker (sum x | sum x^2 | n) over the rows t < frames[b] of feats
    [B, T, D] into stats [S, 2 D + 1] float64, in place (include/mlvae.h, mlvae_cmvn_accumulate):
    a fixed accumulation order, so a rerun is bit-identical.  A speaker id outside [0, S) raises
    ValueError (that utterance is not accumulated)."""
    B, T, D, S, frames, spk = _cmvn_args(feats, frames, spk, stats, "cmvn_accumulate")
    err = torch.zeros(1, device=feats.device, dtype=torch.int32)
    with torch.cuda.device(feats.device):
        check(lib().mlvae_cmvn_accumulate(B, T, D, S, _p(feats) if feats.numel() else None, D,
                                          frames.data_ptr(), spk.data_ptr(), stats.data_ptr(),
                                          err.data_ptr(), _stream()), "cmvn_accumulate")
    if B:
        _raise_cmvn(err, "cmvn_accumulate")
    return stats


def cmvn_apply(feats, frames, spk, stats):
    """y = (x - mean) / sqrt(var) of the speaker's statistics on the rows t < frames[b] of feats
    [B, T, D], in place (mean = sum x / n, var = max(sum x^2 / n - mean^2, 1e-20)); rows past
    frames[b] are not touched.  Returns feats."""
    B, T, D, S, frames, spk = _cmvn_args(feats, frames, spk, stats, "cmvn_apply")
    err = torch.zeros(1, device=feats.device, dtype=torch.int32)
    with torch.cuda.device(feats.device):
        check(lib().mlvae_cmvn_apply(B, T, D, S, _p(feats) if feats.numel() else None, D,
                                     frames.data_ptr(), spk.data_ptr(), stats.data_ptr(),
                                     err.data_ptr(), _stream()), "cmvn_apply")
    if B and T:
        _raise_cmvn(err, "cmvn_apply")
    return feats


# ---- the frozen wav2vec2 encoder (csrc/w2v.hip); forward only, no autograd
def _w2v_dev(t, what, dtypes=(torch.float32,)):
    if not (t.is_cuda and t.dtype in dtypes and t.is_contiguous()):
        raise TypeError(f"{what}: expected a contiguous HIP tensor of {dtypes}, got {t.dtype} on {t.device} "
                        "(the HIP path has no CPU fallback)")
    return t


def w2v_tensor_stats(x, eps=1e-5):
    """[mean, 1 / sqrt(biased var + eps)] over every element of the fp32 tensor x, as a device
    tensor of two floats (F.layer_norm(x, x.shape)'s statistics; fixed-order sums)."""
    x = _w2v_dev(x, "w2v_tensor_stats")
    if x.numel() == 0:
        raise ValueError("w2v_tensor_stats: empty tensor")
    stats = torch.empty(2, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        ws = _workspace(lib().mlvae_w2v_stats_workspace_size(x.numel()), "w2v_stats")
        check(lib().mlvae_w2v_tensor_stats(x.numel(), _p(x), float(eps), _p(stats), _p(ws), ws.numel() * 4,
                                           _stream()), "w2v_tensor_stats")
    return stats


def w2v_scale_shift(x, stats):
    """(x - stats[0]) * stats[1], fp32, same shape."""
    x = _w2v_dev(x, "w2v_scale_shift")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(lib().mlvae_w2v_scale_shift(x.numel(), _p(x), _p(stats), _p(out), _stream()), "w2v_scale_shift")
    return out


def w2v_conv0(wav, stats, w, bias, gamma, beta, stride, eps=1e-5, out_dtype=torch.float32):
    """[B, T0, C] = GELU(LN_C(conv1d((wav - mean) rstd, w [C, K], stride) + bias)), channels-last;
    stats None: the waveform as it is."""
    wav = _w2v_dev(wav, "w2v_conv0 wav")
    B, N = wav.shape
    C, K = w.shape
    if not lib().mlvae_w2v_conv0_supported(C, K):
        raise ValueError(f"w2v_conv0: C = {C}, K = {K} unsupported (C <= 512, K <= 10)")
    if N < K:
        raise ValueError(f"w2v_conv0: {N} samples are shorter than the kernel ({K})")
    T0 = (N - K) // stride + 1
    out = torch.empty(B, T0, C, device=wav.device, dtype=out_dtype)
    with torch.cuda.device(wav.device):
        check(lib().mlvae_w2v_conv0(B, N, T0, C, K, stride, _p(wav), None if stats is None else _p(stats),
                                    _p(w), _p(bias), _p(gamma), _p(beta), float(eps), out.data_ptr(),
                                    int(out_dtype == torch.bfloat16), _stream()), "w2v_conv0")
    return out


def w2v_rows(x, *, bias=None, gamma=None, beta=None, eps=1e-5, gelu=False, res=None, out_f32=False,
             out_bf16=False):
    """Per row of the fp32 x [..., C]: y = x + bias; LN_C (gamma given); GELU; + res.  out_f32: False,
    True (a new tensor) or a tensor to write (res itself: in place); out_bf16: False / True.
    Returns (fp32 result or None, bf16 result or None)."""
    x = _w2v_dev(x, "w2v_rows x")
    C = x.shape[-1]
    N = x.numel() // C
    if C % 4 or (gamma is not None and C > 2048):
        raise ValueError(f"w2v_rows: C = {C} is unsupported (a multiple of 4; LayerNorm over at most 2048)")
    f32 = torch.empty_like(x) if out_f32 is True else (None if out_f32 is False else out_f32)
    b16 = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16) if out_bf16 else None
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(x.device):
        check(lib().mlvae_w2v_rows(N, C, _p(x), C, ptr(bias), ptr(gamma), ptr(beta), float(eps), int(gelu),
                                   ptr(res), C, ptr(f32), ptr(b16), C, _stream()), "w2v_rows")
    return f32, b16


def w2v_regroup(h, G, K, out_dtype=torch.float32):
    """h [B, T, C] fp32 -> the zero-padded group-major copy [B, G, T + K, C / G] (frames at rows
    K/2 .. K/2 + T - 1): a positional-conv window is contiguous in it."""
    h = _w2v_dev(h, "w2v_regroup h")
    B, T, C = h.shape
    out = torch.empty(B, G, T + K, C // G, device=h.device, dtype=out_dtype)
    with torch.cuda.device(h.device):
        check(lib().mlvae_w2v_regroup(B, T, C, G, K, _p(h), out.data_ptr(), int(out_dtype == torch.bfloat16),
                                      _stream()), "w2v_regroup")
    return out


def w2v_attention_supported(T, H, d):
    return bool(lib().mlvae_w2v_attention_supported(T, H, d))


def w2v_attention(qkv, B, T, H, d, *, scale=1.0, f32_math=False, out_dtype=torch.float32):
    """[B T, H d] = softmax(scale Q K^T) V per (utterance, head) from the fused qkv [B T, 3 H d]
    (fp32 or bf16), no mask.  An unsupported shape raises: there is no fallback."""
    qkv = _w2v_dev(qkv, "w2v_attention qkv", (torch.float32, torch.bfloat16))
    if tuple(qkv.shape) != (B * T, 3 * H * d):
        raise ValueError(f"w2v_attention: qkv is {tuple(qkv.shape)}, expected {(B * T, 3 * H * d)}")
    if not w2v_attention_supported(T, H, d) or B > 65535:
        raise ValueError(f"w2v_attention: B = {B}, T = {T}, H = {H}, d = {d} is unsupported "
                         "(d in {32, 64}, B and H <= 65535)")
    out = torch.empty(B * T, H * d, device=qkv.device, dtype=out_dtype)
    with torch.cuda.device(qkv.device):
        check(lib().mlvae_w2v_attention(B, T, H, d, qkv.data_ptr(), int(qkv.dtype == torch.bfloat16),
                                        int(f32_math), float(scale), out.data_ptr(),
                                        int(out_dtype == torch.bfloat16), _stream()), "w2v_attention")
    return out


def w2v_gemm(A, W, C, M, N, K, lda, ldc, *, bias=None, beta=0.0, batch=1, a_bs=0, b_bs=0, c_bs=0, ta=0, tb=1,
             ldb=None):
    """C_z [M, N] (fp32, leading dimension ldc) = A_z W_z^T + bias + beta C_z for z < batch, A_z rows
    of K elements every lda (lda < K: overlapping rows, the conv windows of a channels-last
    sequence), W_z [N, K]; strides in elements.  bf16 operands: mlvae_gemm_bf16 (one batched launch;
    a bf16 C is written by its EPI_OUT_BF16 epilogue, beta 0); fp32 operands: mlvae_gemm's exact-fp32
    path, one launch per z (the parity mode).  The backward's forms: ta = 1: A stored [K][M] (rows
    every lda); tb = 0: W stored [K][N] (rows every ldb; ldb < N: overlapping rows on the B side)."""
    if ldb is None:
        ldb = K
    l = lib()
    c_bf16 = C.dtype == torch.bfloat16
    if A.dtype != W.dtype or A.dtype not in (torch.float32, torch.bfloat16) or not (
            C.dtype == torch.float32 or (c_bf16 and A.dtype == torch.bfloat16 and beta == 0.0)):
        raise TypeError(f"w2v_gemm: operands {A.dtype} / {W.dtype}, C {C.dtype}, beta {beta}")
    bp = None if bias is None else bias.data_ptr()
    with torch.cuda.device(A.device):
        if A.dtype == torch.bfloat16:
            ws = _workspace(l.mlvae_gemm_bf16_workspace_size(M, N, K, batch))
            check(l.mlvae_gemm_bf16(ta, tb, M, N, K, batch, A.data_ptr(), lda, a_bs, W.data_ptr(), ldb, b_bs,
                                    C.data_ptr(), ldc, c_bs, float(beta), bp, None, 32 if c_bf16 else 0, None, 0,
                                    0, 0, 0, 0, 0, 0.0, _p(ws), ws.numel() * 4, _stream()), "mlvae_gemm_bf16")
        else:
            ws = _workspace(l.mlvae_gemm_workspace_size(M, N, K))
            for z in range(batch):
                check(l.mlvae_gemm(0, ta, tb, M, N, K, 1.0, A.data_ptr() + 4 * z * a_bs, lda,
                                   W.data_ptr() + 4 * z * b_bs, ldb, float(beta), C.data_ptr() + 4 * z * c_bs, ldc,
                                   bp, None, 0, None, 0, 0, 0, _p(ws), ws.numel() * 4, _stream()), "mlvae_gemm")
    return C


def w2v_linear(x, W, bias=None, out=None, beta=0.0, out_dtype=torch.float32):
    """out [M, N] = x [M, K] W [N, K]^T + bias + beta out; fp32, or bf16 (bf16 operands, no out)."""
    M, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=out_dtype)
    return w2v_gemm(x, W, out, M, N, K, K, N, bias=bias, beta=beta)


def w2v_conv_gemm(x, W, bias, k, stride):
    """Strided conv1d of the channels-last x [B, T, Cin] as a GEMM over overlapping rows: frame t's
    window is the k Cin contiguous elements at t stride Cin.  W [Cout, k Cin] (the conv weight
    permuted to [Cout][k][Cin]).  Returns fp32 [B, Tout, Cout]."""
    B, T, Cin = x.shape
    Cout = W.shape[0]
    if T < k:
        raise ValueError(f"w2v_conv_gemm: {T} frames are shorter than the kernel ({k})")
    Tout = (T - k) // stride + 1
    out = torch.empty(B, Tout, Cout, device=x.device, dtype=torch.float32)
    return w2v_gemm(x, W, out, Tout, Cout, k * Cin, stride * Cin, Cout, bias=bias, batch=B,
                    a_bs=T * Cin, c_bs=Tout * Cout)


def w2v_pos_conv(hp, W, T, C):
    """The grouped positional conv on the regrouped hp [B, G, T + K, C / G] (w2v_regroup): per
    (utterance, group) a GEMM over overlapping rows, M = T (the conv's last frame is dropped),
    against W [G, C / G, K C / G] (the folded weight regrouped to [G][out][K][in]).  Returns the
    fp32 conv output [B, T, C] without the bias."""
    B, G, TP, Cg = hp.shape
    K = TP - T
    out = torch.empty(B, T, C, device=hp.device, dtype=torch.float32)
    for b in range(B):  # the weight's stride follows the group, not the utterance
        w2v_gemm(hp[b], W, out[b], T, Cg, K * Cg, Cg, C, batch=G, a_bs=TP * Cg, b_bs=Cg * K * Cg, c_bs=Cg)
    return out


# ---- the wav2vec2 encoder's backward (csrc/w2v.hip) and the autograd pieces of the trainable module
def w2v_attention_train(qkv, B, T, H, d, *, scale=1.0, f32_math=False, out_dtype=torch.float32):
    """w2v_attention (the same kernel and output bits) that also returns the per-query log-sum-exp
    of the scaled logits, [B, H, T] fp32: (out, lse)."""
    qkv = _w2v_dev(qkv, "w2v_attention_train qkv", (torch.float32, torch.bfloat16))
    if tuple(qkv.shape) != (B * T, 3 * H * d):
        raise ValueError(f"w2v_attention_train: qkv is {tuple(qkv.shape)}, expected {(B * T, 3 * H * d)}")
    if not w2v_attention_supported(T, H, d) or B > 65535:
        raise ValueError(f"w2v_attention_train: B = {B}, T = {T}, H = {H}, d = {d} is unsupported "
                         "(d in {32, 64}, B and H <= 65535)")
    out = torch.empty(B * T, H * d, device=qkv.device, dtype=out_dtype)
    lse = torch.empty(B, H, T, device=qkv.device, dtype=torch.float32)
    with torch.cuda.device(qkv.device):
        check(lib().mlvae_w2v_attention_train(B, T, H, d, qkv.data_ptr(), int(qkv.dtype == torch.bfloat16),
                                              int(f32_math), float(scale), out.data_ptr(),
                                              int(out_dtype == torch.bfloat16), _p(lse), _stream()),
              "w2v_attention_train")
    return out, lse


def w2v_attention_bwd(qkv, dout, lse, B, T, H, d, *, scale=1.0, f32_math=False):
    """dqkv [B T, 3 H d] of w2v_attention_train from qkv, the output's gradient (both fp32 or both
    bf16; dqkv in the same type) and lse."""
    dt = qkv.dtype
    for t, n in ((qkv, "qkv"), (dout, "dout")):
        _w2v_dev(t, "w2v_attention_bwd " + n, (dt,))
    _w2v_dev(lse, "w2v_attention_bwd lse")
    if dt not in (torch.float32, torch.bfloat16):
        raise TypeError(f"w2v_attention_bwd: {dt} operands")
    if tuple(qkv.shape) != (B * T, 3 * H * d) or tuple(dout.shape) != (B * T, H * d) or tuple(lse.shape) != (B, H, T):
        raise ValueError(f"w2v_attention_bwd: shapes {tuple(qkv.shape)}, {tuple(dout.shape)}, {tuple(lse.shape)} "
                         f"do not fit B = {B}, T = {T}, H = {H}, d = {d}")
    if not w2v_attention_supported(T, H, d) or B > 65535:
        raise ValueError(f"w2v_attention_bwd: B = {B}, T = {T}, H = {H}, d = {d} is unsupported "
                         "(d in {32, 64}, B and H <= 65535)")
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    with torch.cuda.device(qkv.device):
        check(lib().mlvae_w2v_attention_bwd(B, T, H, d, qkv.data_ptr(), dout.data_ptr(),
                                            int(dt == torch.bfloat16), int(f32_math), float(scale), _p(lse),
                                            _p(delta), dqkv.data_ptr(), _stream()), "w2v_attention_bwd")
    return dqkv


def w2v_rows_bwd(dy, x=None, *, bias=None, gamma=None, beta=None, eps=1e-5, gelu=False, acc=None, out_f32=False,
                 out_bf16=False):
    """The backward of w2v_rows through y = [GELU] [LN] (x [+ bias]): out = [acc +] dx.  out_f32: False,
    True (a new tensor) or a tensor to write (acc itself: in place); out_bf16: False / True.
    Returns (fp32 or None, bf16 or None, dgamma or None, dbeta or None)."""
    dy = _w2v_dev(dy, "w2v_rows_bwd dy")
    C = dy.shape[-1]
    N = dy.numel() // C
    if C % 4 or (gamma is not None and C > 2048):
        raise ValueError(f"w2v_rows_bwd: C = {C} is unsupported (a multiple of 4; LayerNorm over at most 2048)")
    for t in (x, acc):
        if t is not None and _w2v_dev(t, "w2v_rows_bwd x / acc").shape != dy.shape:
            raise ValueError(f"w2v_rows_bwd: {tuple(t.shape)} against dy {tuple(dy.shape)}")
    f32 = torch.empty_like(dy) if out_f32 is True else (None if out_f32 is False else out_f32)
    b16 = torch.empty(dy.shape, device=dy.device, dtype=torch.bfloat16) if out_bf16 else None
    dg = db = ws = None
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dy.device):
        nbytes = 0
        if gamma is not None:
            dg, db = torch.empty_like(gamma), torch.empty_like(gamma)
            nbytes = lib().mlvae_w2v_rows_bwd_workspace_size(N, C)
            ws = _workspace(nbytes, "w2v_rows_bwd")
        check(lib().mlvae_w2v_rows_bwd(N, C, _p(dy), ptr(x), ptr(bias), ptr(gamma), ptr(beta), float(eps),
                                       int(gelu), ptr(acc), ptr(f32), ptr(b16), ptr(dg), ptr(db), ptr(ws),
                                       nbytes, _stream()), "w2v_rows_bwd")
    return f32, b16, dg, db


def w2v_norm_bwd(dy, xhat, stats):
    """dx of the whole-tensor norm xhat = (x - mean) rstd (w2v_tensor_stats + w2v_scale_shift) given
    its output and stats: stats[1] (dy - mean(dy) - xhat mean(dy xhat)), fp64 fixed-order sums."""
    dy, xhat = _w2v_dev(dy, "w2v_norm_bwd dy"), _w2v_dev(xhat, "w2v_norm_bwd xhat")
    if dy.shape != xhat.shape or dy.numel() == 0:
        raise ValueError(f"w2v_norm_bwd: dy {tuple(dy.shape)} against xhat {tuple(xhat.shape)}")
    dx = torch.empty_like(dy)
    with torch.cuda.device(dy.device):
        nbytes = lib().mlvae_w2v_norm_bwd_workspace_size(dy.numel())
        ws = _workspace(nbytes, "w2v_stats")
        check(lib().mlvae_w2v_norm_bwd(dy.numel(), _p(dy), _p(xhat), _p(stats), _p(dx), _p(ws), ws.numel() * 4,
                                       _stream()), "w2v_norm_bwd")
    return dx


def w2v_colsum(t):
    """The column sums of t [N, C] (fp32 or bf16) as fp32 [C]: a bias gradient (mlvae_colsum_ex)."""
    t = _w2v_dev(t, "w2v_colsum", (torch.float32, torch.bfloat16))
    N, C = t.shape
    out = torch.empty(C, device=t.device, dtype=torch.float32)
    with torch.cuda.device(t.device):
        ws = _workspace(lib().mlvae_colsum_workspace_size(N, C), "colsum")
        check(lib().mlvae_colsum_ex(N, C, t.data_ptr(), int(t.dtype == torch.bfloat16), C, _p(out), None, 0.0,
                                    _p(ws), ws.numel() * 4, _stream()), "mlvae_colsum_ex")
    return out


def w2v_cast(t, dtype):
    """t itself (fp32 wanted) or its bf16 copy (mlvae_cast_bf16): a GEMM operand."""
    if dtype == torch.float32:
        return t
    out = torch.empty(t.shape, device=t.device, dtype=torch.bfloat16)
    with torch.cuda.device(t.device):
        check(lib().mlvae_cast_bf16(t.numel(), _p(t), out.data_ptr(), _stream()), "mlvae_cast_bf16")
    return out


def w2v_linear_dx(dy, W, out_dtype=torch.float32):
    """dx [M, K] = dy [M, N] W [N, K]: the weight as it is stored, read n-major (trans_b = 0)."""
    M, N = dy.shape
    K = W.shape[1]
    out = torch.empty(M, K, device=dy.device, dtype=out_dtype)
    return w2v_gemm(dy, W, out, M, K, N, N, K, tb=0, ldb=K)


def w2v_linear_dw(dy, x):
    """dW [N, K] fp32 = dy [M, N]^T x [M, K]: both operands as the forward wrote them (frames along
    the product's K dimension, which need not be a multiple of 8: those forms mask whole k-rows)."""
    M, N = dy.shape
    K = x.shape[1]
    out = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    return w2v_gemm(dy, x, out, N, K, M, N, K, ta=1, tb=0, ldb=K)


def w2v_pos_conv_dx(dpr, Wrev, T, C, out):
    """out [B, T, C] += the positional conv's input gradient: the same overlapping-row GEMM as the
    forward on the regrouped gradient dpr [B, G, T + K, C / G], one row further down, against the
    tap-reversed, in / out-swapped weight Wrev [G, in, K out]."""
    B, G, TP, Cg = dpr.shape
    K = TP - T
    flat = dpr.view(B, -1)
    for b in range(B):
        w2v_gemm(flat[b, Cg:], Wrev, out[b], T, Cg, K * Cg, Cg, C, beta=1.0, batch=G, a_bs=TP * Cg,
                 b_bs=Cg * K * Cg, c_bs=Cg)
    return out


def w2v_pos_conv_dw(dpc, hp, T, C):
    """The regrouped positional weight's gradient [G, out, K in] fp32: per group dpc_g^T (frames x out,
    a column slice of dpc [B, T, C]) times the overlapping-row windows of hp [B, G, T + K, C / G] on
    the B side, summed over the utterances in order (beta = 1 from the second on)."""
    B, G, TP, Cg = hp.shape
    K = TP - T
    out = torch.empty(G, Cg, K * Cg, device=hp.device, dtype=torch.float32)
    dpc = dpc.view(B, T * C)
    for b in range(B):
        w2v_gemm(dpc[b], hp[b], out, Cg, K * Cg, T, C, K * Cg, beta=0.0 if b == 0 else 1.0, batch=G, a_bs=Cg,
                 b_bs=TP * Cg, c_bs=Cg * K * Cg, ta=1, tb=0, ldb=Cg)
    return out


class W2VHeadFn(torch.autograd.Function):
    """The projection's LayerNorm and Linear and h += GELU(pos_conv(h) + bias) on the frozen conv
    stack's fp32 output xf [B, T, Cc].  P: the kernel-side weights (modules/wav2vec2.py).  The
    trailing tensors are the fp32 masters the gradients go to: LN weight / bias, projection weight /
    bias, the positional conv's bias, g, v.  Saved: xf, the LN output and the regrouped projection
    (the weight gradients' operands, bf16 in bf16 mode) and the fp32 conv output before its GELU."""

    @staticmethod
    def forward(ctx, xf, P, geo, ln_w, ln_b, pw, pb, cb, cg, cv):
        B, T, H, G, K, eps, bf = geo
        ad = torch.bfloat16 if bf else torch.float32
        act = lambda pair: pair[1] if bf else pair[0]
        x0 = act(w2v_rows(xf.view(B * T, -1), gamma=P["proj_ln"][0], beta=P["proj_ln"][1], eps=eps,
                          out_f32=not bf, out_bf16=bf))
        h = w2v_linear(x0, *P["proj"])
        hp = w2v_regroup(h.view(B, T, H), G, K, out_dtype=ad)
        pc = w2v_pos_conv(hp, P["pos"][0], T, H)
        w2v_rows(pc.view(B * T, H), bias=P["pos"][1], gelu=True, res=h, out_f32=h)
        ctx.save_for_backward(xf, x0, hp, pc, cg, cv)
        ctx.P, ctx.geo = P, geo
        return h

    @staticmethod
    def backward(ctx, dh):
        xf, x0, hp, pc, cg, cv = ctx.saved_tensors
        P, (B, T, H, G, K, eps, bf) = ctx.P, ctx.geo
        ad = torch.bfloat16 if bf else torch.float32
        dh = dh.contiguous()
        Cg = H // G
        # through h += GELU(pc + bias): the residual branch carries dh on
        dpc, dpcb, _, _ = w2v_rows_bwd(dh, pc.view(B * T, H), bias=P["pos"][1], gelu=True, out_f32=True,
                                       out_bf16=bf)
        d_cb = w2v_colsum(dpc)
        dpr = w2v_regroup(dpc.view(B, T, H), G, K, out_dtype=ad)
        dhp = w2v_pos_conv_dx(dpr, P["pos_rev"], T, H, dh.clone().view(B, T, H)).view(B * T, H)
        dwg = w2v_pos_conv_dw(dpcb if bf else dpc, hp, T, H)  # [G, out, K in]
        dwf = dwg.view(G, Cg, K, Cg).permute(0, 1, 3, 2).reshape(H, Cg, K)  # the folded weight's layout
        # weight norm (dim 2): w = v g / n, n = ||v[:, :, k]||: elementwise on a small parameter
        n = cv.detach().norm(dim=(0, 1), keepdim=True)
        dot = (dwf * cv.detach()).sum(dim=(0, 1), keepdim=True)
        d_cg = dot / n
        d_cv = dwf * (cg.detach() / n) - cv.detach() * (cg.detach() * dot / n.pow(3))
        # the projection
        d_pb = w2v_colsum(dhp)
        dhpb = w2v_cast(dhp, ad)
        d_pw = w2v_linear_dw(dhpb, x0)
        dx0 = w2v_linear_dx(dhpb, P["proj"][0])
        _, _, d_lw, d_lb = w2v_rows_bwd(dx0, xf.view(B * T, -1), gamma=P["proj_ln"][0], beta=P["proj_ln"][1],
                                        eps=eps, out_f32=True)  # the conv stack is frozen: dx is not used
        return None, None, None, d_lw, d_lb, d_pw, d_pb, d_cb, d_cg, d_cv


class W2VLayerFn(torch.autograd.Function):
    """One pre-LN transformer layer on the fp32 residual stream h [B T, H]:
    h += out_proj(attn(LN(h))); h += W2 GELU(W1 LN(h)).  L: the layer's kernel-side weights.  The
    trailing tensors are the fp32 masters, in this order: layer_norm w / b, q / k / v / out_proj w / b
    each, final_layer_norm w / b, intermediate_dense w / b, output_dense w / b.  Saved: the two LN
    inputs (the residual stream, fp32), the three GEMM-operand activations and the attention output
    (bf16 in bf16 mode), qkv, the log-sum-exp and the fp32 FFN activation before its GELU."""

    @staticmethod
    def forward(ctx, h0, L, geo, *masters):
        B, T, H, heads, eps, bf = geo
        d = H // heads
        ad = torch.bfloat16 if bf else torch.float32
        act = lambda pair: pair[1] if bf else pair[0]
        x1 = act(w2v_rows(h0, gamma=L["ln1"][0], beta=L["ln1"][1], eps=eps, out_f32=not bf, out_bf16=bf))
        qkv = w2v_linear(x1, *L["qkv"], out_dtype=ad)
        a, lse = w2v_attention_train(qkv, B, T, heads, d, f32_math=not bf, out_dtype=ad)
        h1 = h0.clone()
        w2v_linear(a, *L["out"], out=h1, beta=1.0)
        x2 = act(w2v_rows(h1, gamma=L["ln2"][0], beta=L["ln2"][1], eps=eps, out_f32=not bf, out_bf16=bf))
        f1 = w2v_linear(x2, *L["w1"])
        x3 = act(w2v_rows(f1, gelu=True, out_f32=not bf, out_bf16=bf))
        h2 = h1.clone()
        w2v_linear(x3, *L["w2"], out=h2, beta=1.0)
        ctx.save_for_backward(h0, x1, qkv, a, lse, h1, x2, f1, x3)
        ctx.L, ctx.geo = L, geo
        return h2

    @staticmethod
    def backward(ctx, dh):
        h0, x1, qkv, a, lse, h1, x2, f1, x3 = ctx.saved_tensors
        L, (B, T, H, heads, eps, bf) = ctx.L, ctx.geo
        d = H // heads
        ad = torch.bfloat16 if bf else torch.float32
        act = lambda t: t[1] if bf else t[0]
        dh = dh.contiguous()
        # the FFN branch
        dhb = w2v_cast(dh, ad)
        d_b2 = w2v_colsum(dh)
        d_w2 = w2v_linear_dw(dhb, x3)
        dx3 = w2v_linear_dx(dhb, L["w2"][0])
        df1 = act(w2v_rows_bwd(dx3, f1, gelu=True, out_f32=not bf, out_bf16=bf))
        d_b1 = w2v_colsum(df1)
        d_w1 = w2v_linear_dw(df1, x2)
        dx2 = w2v_linear_dx(df1, L["w1"][0])
        dh1, dh1b, d_g2, d_be2 = w2v_rows_bwd(dx2, h1, gamma=L["ln2"][0], beta=L["ln2"][1], eps=eps, acc=dh,
                                              out_f32=True, out_bf16=bf)
        if not bf:
            dh1b = dh1
        # the attention branch
        d_bo = w2v_colsum(dh1)
        d_wo = w2v_linear_dw(dh1b, a)
        da = w2v_linear_dx(dh1b, L["out"][0], out_dtype=ad)
        dqkv = w2v_attention_bwd(qkv, da, lse, B, T, heads, d, f32_math=not bf)
        d_bqkv = w2v_colsum(dqkv)
        d_wqkv = w2v_linear_dw(dqkv, x1)
        dx1 = w2v_linear_dx(dqkv, L["qkv"][0])
        dh0, _, d_g1, d_be1 = w2v_rows_bwd(dx1, h0, gamma=L["ln1"][0], beta=L["ln1"][1], eps=eps, acc=dh1,
                                           out_f32=dh1)
        # 1 / sqrt(d) is folded into the fused weight's Q rows: q_proj's gradients carry it
        scale = d ** -0.5
        return (dh0, None, None, d_g1, d_be1, d_wqkv[:H] * scale, d_bqkv[:H] * scale, d_wqkv[H:2 * H],
                d_bqkv[H:2 * H], d_wqkv[2 * H:], d_bqkv[2 * H:], d_wo, d_bo, d_g2, d_be2, d_w1, d_b1, d_w2, d_b2)


class W2VTailFn(torch.autograd.Function):
    """The final LayerNorm and, with output_norm, the whole-tensor norm.  Masters: encoder.layer_norm
    w / b.  Saved: the residual stream and the returned output (the whole-tensor norm's x hat)."""

    @staticmethod
    def forward(ctx, h, P, eps, output_norm, ln_w, ln_b):
        out = w2v_rows(h, gamma=P["final_ln"][0], beta=P["final_ln"][1], eps=eps, out_f32=True)[0]
        stats = None
        if output_norm:
            stats = w2v_tensor_stats(out)
            out = w2v_scale_shift(out, stats)
        ctx.save_for_backward(h, out, stats)
        ctx.P, ctx.eps = P, eps
        return out

    @staticmethod
    def backward(ctx, dout):
        h, out, stats = ctx.saved_tensors
        dout = dout.contiguous()
        if stats is not None:
            dout = w2v_norm_bwd(dout, out, stats)
        dh, _, d_w, d_b = w2v_rows_bwd(dout.view(h.shape), h, gamma=ctx.P["final_ln"][0], beta=ctx.P["final_ln"][1],
                                       eps=ctx.eps, out_f32=True)
        return dh, None, None, None, d_w, d_b
