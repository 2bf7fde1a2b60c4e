"""The wav2vec2 encoder: forward, backward and the autograd pieces of the trainable module
(csrc/w2v.hip)."""
import torch

from .._lib import check, lib
from ._core import _p, _stream, _workspace, _ws_bytes


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
        check(lib().mlvae_w2v_tensor_stats(x.numel(), _p(x), float(eps), _p(stats), _p(ws), _ws_bytes(ws),
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
                                    0, 0, 0, 0, 0, 0.0, _p(ws), _ws_bytes(ws), _stream()), "mlvae_gemm_bf16")
        else:
            ws = _workspace(l.mlvae_gemm_workspace_size(M, N, K))
            for z in range(batch):
                check(l.mlvae_gemm(0, ta, tb, M, N, K, 1.0, A.data_ptr() + 4 * z * a_bs, lda,
                                   W.data_ptr() + 4 * z * b_bs, ldb, float(beta), C.data_ptr() + 4 * z * c_bs, ldc,
                                   bp, None, 0, None, 0, 0, 0, _p(ws), _ws_bytes(ws), _stream()), "mlvae_gemm")
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
        check(lib().mlvae_w2v_norm_bwd(dy.numel(), _p(dy), _p(xhat), _p(stats), _p(dx), _p(ws), _ws_bytes(ws),
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
                                    _p(ws), _ws_bytes(ws), _stream()), "mlvae_colsum_ex")
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


# ---- the conv stack's backward ("The wav2vec2 encoder", "Backward", "The conv stack")
def w2v_conv0_bwd(wav, stats, w, bias, gamma, beta, stride, dout, eps=1e-5):
    """The backward of w2v_conv0 given dout [B, T0, C] fp32, the gradient at its output: (dw [C, K],
    dbias, dgamma, dbeta).  The pre-LN activation is recomputed from the waveform, never stored;
    fixed-order sums, no input gradient (the waveform carries none, and neither do stats)."""
    wav, dout = _w2v_dev(wav, "w2v_conv0_bwd wav"), _w2v_dev(dout, "w2v_conv0_bwd dout")
    B, N = wav.shape
    C, K = w.shape
    if not lib().mlvae_w2v_conv0_supported(C, K):
        raise ValueError(f"w2v_conv0_bwd: C = {C}, K = {K} unsupported (C <= 512, K <= 10)")
    if N < K:
        raise ValueError(f"w2v_conv0_bwd: {N} samples are shorter than the kernel ({K})")
    T0 = (N - K) // stride + 1
    if tuple(dout.shape) != (B, T0, C):
        raise ValueError(f"w2v_conv0_bwd: dout is {tuple(dout.shape)}, expected {(B, T0, C)}")
    for t, n in ((w, "w"), (bias, "bias"), (gamma, "gamma"), (beta, "beta")):
        _w2v_dev(t, "w2v_conv0_bwd " + n)
    dw = torch.empty(C, K, device=wav.device, dtype=torch.float32)
    db, dg, dbe = (torch.empty(C, device=wav.device, dtype=torch.float32) for _ in range(3))
    with torch.cuda.device(wav.device):
        nbytes = lib().mlvae_w2v_conv0_bwd_workspace_size(B, T0, C, K)
        ws = _workspace(nbytes, "w2v_conv0_bwd")
        check(lib().mlvae_w2v_conv0_bwd(B, N, T0, C, K, stride, _p(wav), None if stats is None else _p(stats),
                                        _p(w), _p(bias), _p(gamma), _p(beta), float(eps), _p(dout), _p(dw), _p(db),
                                        _p(dg), _p(dbe), _p(ws), _ws_bytes(ws), _stream()), "w2v_conv0_bwd")
    return dw, db, dg, dbe


def _conv_geometry(k, stride, T_in):
    """(Tout, taps per residue m_r, guard rows before, guard rows after) of a strided conv's input
    gradient.  Input frame n = stride u + r takes dx[n] = sum_{q < m_r} dy[u - q] W[:, :, r + q stride],
    m_r = ceil((k - r) / stride), dy = 0 outside [0, Tout): u - q reaches m_0 - 1 rows before the first
    frame and u reaches ceil(T_in / stride) - 1, at or past the last."""
    if not 1 <= stride <= k:
        raise ValueError(f"w2v_conv_dx: stride {stride} against kernel {k} is unsupported (1 <= stride <= k)")
    if T_in < k:
        raise ValueError(f"w2v_conv_dx: {T_in} frames are shorter than the kernel ({k})")
    Tout = (T_in - k) // stride + 1
    m = [-((r - k) // stride) for r in range(stride)]
    return Tout, m, m[0] - 1, -(-T_in // stride) - Tout


def w2v_conv_dx_weights(w, stride, dtype):
    """The conv weight [Cout, Cin, k] regrouped for w2v_conv_dx: per residue r the taps r, r + stride,
    ... in reverse order with in / out swapped, [Cin, m_r Cout] in `dtype`."""
    Cout, Cin, k = w.shape
    _, m, _, _ = _conv_geometry(k, stride, k)
    return [w[:, :, r::stride].flip(-1).permute(1, 2, 0).reshape(Cin, m[r] * Cout).to(dtype).contiguous()
            for r in range(stride)]


def w2v_conv_pad(dy, k, stride, T_in, dtype):
    """dy [B, Tout, Cout] fp32 with the zero guard rows of w2v_conv_dx before and after every
    utterance, in `dtype` (fp32 or bf16): ([B, pf + Tout + pa, Cout], pf).  One kernel: the copy is the
    bf16 mode's operand cast as well, and w2v_conv_dw reads the same copy."""
    dy = _w2v_dev(dy, "w2v_conv_pad dy")
    B, Tout, Cout = dy.shape
    T, _, pf, pa = _conv_geometry(k, stride, T_in)
    if T != Tout:
        raise ValueError(f"w2v_conv_pad: dy has {Tout} frames, a conv of {T_in} frames gives {T}")
    if pf == 0 and pa == 0 and dtype == torch.float32:
        return dy, 0
    out = torch.empty(B, pf + Tout + pa, Cout, device=dy.device, dtype=dtype)
    with torch.cuda.device(dy.device):
        check(lib().mlvae_w2v_pad_rows(B, Tout, Cout, pf, pa, _p(dy), out.data_ptr(),
                                       int(dtype == torch.bfloat16), _stream()), "w2v_pad_rows")
    return out, pf


def w2v_conv_dx(dy, W, k, stride, T_in, padded=None):
    """The strided conv's input gradient dx [B, T_in, Cin] fp32 from dy [B, Tout, Cout] fp32: one GEMM
    per residue r over overlapping rows of the guarded dy (lda = Cout, m_r Cout wide), written at
    ldc = stride Cin with column offset r Cin -- the exact dgrad's FLOPs, no zero blocks and no
    column tensor.  W: w2v_conv_dx_weights (their dtype is the operand dtype); padded: w2v_conv_pad's
    result when the caller already has it.  Frames at or past (Tout - 1) stride + k get exactly 0."""
    Tout, m, pf, pa = _conv_geometry(k, stride, T_in)
    if len(W) != stride:
        raise ValueError(f"w2v_conv_dx: {len(W)} residue weights for stride {stride}")
    dyp, pf_ = padded if padded is not None else w2v_conv_pad(dy, k, stride, T_in, W[0].dtype)
    B, TP, Cout = dyp.shape
    Cin = W[0].shape[0]
    if TP != pf + Tout + pa or pf_ != pf or dyp.dtype != W[0].dtype or any(
            tuple(W[r].shape) != (Cin, m[r] * Cout) for r in range(stride)):
        raise ValueError(f"w2v_conv_dx: dy {tuple(dyp.shape)} / weights {[tuple(t.shape) for t in W]} do not fit "
                         f"k = {k}, stride = {stride}, T_in = {T_in}")
    dx = torch.empty(B, T_in, Cin, device=dyp.device, dtype=torch.float32)
    flat, out = dyp.view(-1), dx.view(-1)
    for r in range(stride):
        U = -(-(T_in - r) // stride)  # the frames of this residue
        w2v_gemm(flat[(pf - (m[r] - 1)) * Cout:], W[r], out[r * Cin:], U, Cin, m[r] * Cout, Cout, stride * Cin,
                 batch=B, a_bs=TP * Cout, c_bs=T_in * Cin)
    return dx


def w2v_conv_dw(dy, x, k, stride):
    """The conv weight's gradient [Cout, k Cin] fp32 (the kernel-side [Cout][k][Cin] order): per
    utterance dy_b^T [Cout, Tout] times the overlapping-row windows of x_b [B, T_in, Cin] on the B
    side (ldb = stride Cin), the utterances summed in order (beta = 1 from the second on).  dy
    [B, Tout, Cout] in x's dtype; its utterances may lie apart (a slice of the guarded copy)."""
    B, Tout, Cout = dy.shape
    _, T_in, Cin = x.shape
    if Tout != (T_in - k) // stride + 1 or dy.dtype != x.dtype or dy.stride()[1:] != (Cout, 1):
        raise ValueError(f"w2v_conv_dw: dy {tuple(dy.shape)} ({dy.dtype}) against x {tuple(x.shape)} ({x.dtype}), "
                         f"k = {k}, stride = {stride}")
    out = torch.empty(Cout, k * Cin, device=x.device, dtype=torch.float32)
    for b in range(B):
        w2v_gemm(dy[b], x[b], out, Cout, k * Cin, Tout, Cout, k * Cin, beta=0.0 if b == 0 else 1.0, ta=1, tb=0,
                 ldb=stride * Cin)
    return out


class W2VConvFn(torch.autograd.Function):
    """normalize_wav and the conv layers on wav [B, N]: the last layer's fp32 output [B, T, conv_dim]
    (Wav2Vec2._conv_stack's kernel sequence unchanged: the same bits).  P: the kernel-side weights; geo:
    (kernels, strides, eps, bf, normalize_wav, stages).  The trailing tensors are the fp32 masters the
    gradients go to, four per layer: conv weight / bias, LN weight / bias.  Saved: the waveform and its
    statistics (layer 0 is recomputed in its backward), and per layer i >= 1 its input in the GEMM
    operand dtype (what the forward produces anyway) and its fp32 pre-LN output."""

    @staticmethod
    def forward(ctx, wav, P, geo, *masters):
        ks, ss, eps, bf, normalize_wav, stages = geo
        ad = torch.bfloat16 if bf else torch.float32
        keep = (lambda n, t: stages.__setitem__(n, t.float().clone())) if stages is not None else (lambda n, t: None)
        wav = wav.detach().float().contiguous()
        stats = w2v_tensor_stats(wav) if normalize_wav else None
        W, b, g, be = P["conv"][0][:4]
        x = w2v_conv0(wav, stats, W, b, g, be, ss[0], eps, out_dtype=ad)
        keep("conv0", x)
        n_conv = len(ks)
        xf = x if not bf else None
        saved = [wav, stats]
        for i in range(1, n_conv):
            W, b, g, be = P["conv"][i][:4]
            y = w2v_conv_gemm(x, W, b, ks[i], ss[i])
            last = i == n_conv - 1
            saved += [x, y]
            xf, xb = w2v_rows(y, gamma=g, beta=be, eps=eps, gelu=True, out_f32=last or not bf,
                              out_bf16=bf and not last)
            x = xb if xb is not None else xf
            keep(f"conv{i}", x)
        if xf is None:  # a one-layer conv stack in bf16: conv0 wrote bf16
            xf = x.float()
        ctx.save_for_backward(*saved)
        ctx.P, ctx.geo = P, geo
        return xf

    @staticmethod
    def backward(ctx, d):
        wav, stats, *acts = ctx.saved_tensors
        P, (ks, ss, eps, bf, _, _) = ctx.P, ctx.geo
        ad = torch.bfloat16 if bf else torch.float32
        d = d.contiguous()
        grads = []
        for i in range(len(ks) - 1, 0, -1):
            x, y = acts[2 * (i - 1)], acts[2 * (i - 1) + 1]
            W, _, g, be, Wdx = P["conv"][i]
            B, T_in, Cin = x.shape
            Cout = y.shape[2]
            dy, _, d_g, d_be = w2v_rows_bwd(d, y, gamma=g, beta=be, eps=eps, gelu=True, out_f32=True)
            d_b = w2v_colsum(dy.view(-1, Cout))
            dyp, pf = w2v_conv_pad(dy, ks[i], ss[i], T_in, ad)
            d_w = w2v_conv_dw(dyp[:, pf:pf + dy.shape[1]], x, ks[i], ss[i])
            d = w2v_conv_dx(None, Wdx, ks[i], ss[i], T_in, padded=(dyp, pf))
            grads = [d_w.view(Cout, ks[i], Cin).permute(0, 2, 1).contiguous(), d_b, d_g, d_be] + grads
        W, b, g, be = P["conv"][0][:4]
        d_w, d_b, d_g, d_be = w2v_conv0_bwd(wav, stats, W, b, g, be, ss[0], d, eps)
        return (None, None, None, d_w.view(W.shape[0], 1, W.shape[1]), d_b, d_g, d_be, *grads)


class W2VHeadFn(torch.autograd.Function):
    """The projection's LayerNorm and Linear and h += GELU(pos_conv(h) + bias) on the conv stack's
    fp32 output xf [B, T, Cc] (frozen, or W2VConvFn's: then its gradient is returned too).  P: the
    kernel-side weights (modules/wav2vec2.py).  The
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
        dxf, _, d_lw, d_lb = w2v_rows_bwd(dx0, xf.view(B * T, -1), gamma=P["proj_ln"][0], beta=P["proj_ln"][1],
                                          eps=eps, out_f32=True)
        # the conv stack's gradient, when it trains (W2VConvFn); frozen: dx is not used
        dxf = dxf.view(xf.shape) if ctx.needs_input_grad[0] else None
        return dxf, None, None, d_lw, d_lb, d_pw, d_pb, d_cb, d_cg, d_cv


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
