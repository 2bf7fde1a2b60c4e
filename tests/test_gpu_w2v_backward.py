"""The wav2vec2 encoder's backward kernels (csrc/w2v.hip) one by one against float64 autograd of
the same operation in torch: attention (with the training forward's log-sum-exp), the row kernel's
backward in every form the forward uses, the whole-tensor norm's backward and the positional conv's
input and weight gradients (the existing GEMMs over the regrouped layout).

Tolerance rule: tests/w2v_grad_ref.py -- the yardstick is the same autograd on the CPU in float32
(fp32 mode) or under bf16 autocast (bf16 mode), its error against float64 floored at 2^-23
relative; the device is held to 4 x, maximum and relative RMS.  Figures are printed before they are
asserted.  Measured (largest maximum error over a group's cases: device, yardstick; the worst single
device / yardstick ratio of the maximum error, bound 4):

    quantity                         fp32 device  yardstick  ratio    bf16 device  yardstick  ratio
    attention log-sum-exp (84 cases)   8.8e-07     7.9e-07    3.45      6.6e-03     1.5e-02    1.31
    attention dqkv (84 cases)          1.4e-06     1.2e-06    2.29      1.6e-02     2.7e-02    1.05
    attention dqkv, Q x 30             6.5e-04     5.8e-04    1.11      5.1e+00     6.4e+00    0.80
    attention dqkv, bf16 in / out                                       7.3e-03     8.7e-03    0.84
    rows dx (LN, GELU + bias, GELU)    6.0e-07     9.0e-07    1.87      7.8e-03     7.8e-03    1.00  (bf16 out)
    rows dgamma                        4.0e-06     8.6e-06    2.11
    rows dbeta                         1.9e-06     1.0e-05    0.39
    rows bias sums                     5.1e-06     7.0e-06    0.94
    whole-tensor norm dx               3.5e-07     4.0e-07    1.38
    positional conv dh                 3.1e-06     2.1e-06    2.15      1.1e-02     1.2e-02    0.87
    positional conv dw                 1.4e-05     1.3e-05    1.07      1.5e-01     2.3e-01    0.84
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_utils import need_gpu
from w2v_grad_ref import held

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "bf16"]


# ------------------------------------------------------------------ attention
def att_inputs(B, T, H, d, seed, qscale=1.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, 3 * H * d, generator=g)
    qkv[:, :H * d] *= qscale
    return qkv, torch.randn(B * T, H * d, generator=g)


def ref_attention_grads(qkv, dout, B, T, H, d, dt, autocast=False):
    """(out, lse, dqkv) of softmax(Q K^T / sqrt(d)) V per (utterance, head) by autograd."""
    x = qkv.to(dt).clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        q, k, v = (t.reshape(B, T, H, d).transpose(1, 2) for t in x.view(B, T, 3, H * d).unbind(2))
        s = (q @ k.transpose(-1, -2)) * d ** -0.5
        p = torch.softmax(s, dim=-1)
        out = (p.to(v.dtype) @ v).transpose(1, 2).reshape(B * T, H * d)
        lse = torch.logsumexp(s.float() if autocast else s, dim=-1)
    (out.to(dt) * dout.to(dt)).sum().backward()
    return out.detach().float() if dt != torch.float64 else out.detach(), lse.detach(), x.grad.detach()


def run_attention(qkv, dout, B, T, H, d, prec):
    from mlvae_hip import ops
    f32 = prec == "fp32"
    q = qkv.cuda()
    out, lse = ops.w2v_attention_train(q, B, T, H, d, scale=d ** -0.5, f32_math=f32)
    dqkv = ops.w2v_attention_bwd(q, dout.cuda(), lse, B, T, H, d, scale=d ** -0.5, f32_math=f32)
    return out, lse, dqkv


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 31, 33, 257])  # the 16-query and 32-key tile edges, five workgroups
def test_attention_backward(T, d, prec):
    need_gpu()
    from mlvae_hip import ops
    for H in (1, 2, 16):
        for B in (1, 3):
            qkv, dout = att_inputs(B, T, H, d, seed=1000 * T + 10 * d + H + B)
            o64, l64, g64 = ref_attention_grads(qkv, dout, B, T, H, d, torch.float64)
            oy, ly, gy = ref_attention_grads(qkv, dout, B, T, H, d, torch.float32, autocast=prec == "bf16")
            out, lse, dqkv = run_attention(qkv, dout, B, T, H, d, prec)
            what = f"T={T} d={d} H={H} B={B} {prec}"
            assert dqkv.shape == (B * T, 3 * H * d) and dqkv.dtype == torch.float32 and lse.shape == (B, H, T)
            held(lse, l64, ly, "attention lse " + what)
            # per tensor: dqkv as a whole.  Its maximum bounds every section's; a section alone is not a
            # tensor of the rule (at T = 1 dQ and dK are identically zero and so is torch's softmax
            # backward, in every precision, which leaves no yardstick to scale)
            held(dqkv, g64, gy, "attention dqkv " + what)
            # the training forward is the frozen kernel: the same output bits; a rerun: the same bits
            assert torch.equal(out, ops.w2v_attention(qkv.cuda(), B, T, H, d, scale=d ** -0.5, f32_math=prec == "fp32"))
            out2, lse2, dqkv2 = run_attention(qkv, dout, B, T, H, d, prec)
            assert torch.equal(dqkv, dqkv2) and torch.equal(lse, lse2) and torch.equal(out, out2)


@pytest.mark.parametrize("prec", PRECS)
def test_attention_backward_saturated_rows(prec):
    """Q scaled by 30 (logits near 200, rows close to one-hot): P is recomputed from the log-sum-exp
    without overflow and every gradient is finite."""
    need_gpu()
    B, T, H, d = 3, 33, 2, 64
    qkv, dout = att_inputs(B, T, H, d, seed=5, qscale=30.0)
    o64, l64, g64 = ref_attention_grads(qkv, dout, B, T, H, d, torch.float64)
    oy, ly, gy = ref_attention_grads(qkv, dout, B, T, H, d, torch.float32, autocast=prec == "bf16")
    out, lse, dqkv = run_attention(qkv, dout, B, T, H, d, prec)
    assert l64.abs().max() > 100
    held(lse, l64, ly, f"saturated lse {prec}")
    held(dqkv, g64, gy, f"saturated dqkv {prec}")


def test_attention_backward_bf16_io():
    """bf16 qkv and dout in and bf16 dqkv out: what the bf16 encoder passes."""
    need_gpu()
    from mlvae_hip import ops
    B, T, H, d = 3, 33, 2, 64
    qkv, dout = att_inputs(B, T, H, d, seed=9)
    qkv, dout = qkv.bfloat16().float(), dout.bfloat16().float()
    o64, l64, g64 = ref_attention_grads(qkv, dout, B, T, H, d, torch.float64)
    oy, ly, gy = ref_attention_grads(qkv, dout, B, T, H, d, torch.float32, autocast=True)
    q = qkv.cuda().bfloat16()
    out, lse = ops.w2v_attention_train(q, B, T, H, d, scale=d ** -0.5, out_dtype=torch.bfloat16)
    dqkv = ops.w2v_attention_bwd(q, dout.cuda().bfloat16(), lse, B, T, H, d, scale=d ** -0.5)
    assert dqkv.dtype == torch.bfloat16
    held(dqkv.float(), g64, gy.bfloat16().float(), "attention backward bf16 in / out")


# ------------------------------------------------------------------ the row kernel's backward
ROW_FORMS = ["ln", "bias_gelu_res", "gelu", "ln_bf16"]


def row_ref(form, x, dy, bias, gamma, beta, acc, dt):
    """(dx [+ acc], dgamma, dbeta, dbias) by autograd in dt."""
    xx = x.to(dt).clone().requires_grad_(True)
    ps = [None if t is None else t.to(dt).clone().requires_grad_(True) for t in (bias, gamma, beta)]
    b, g, be = ps
    y = xx if b is None else xx + b
    if g is not None:
        y = F.layer_norm(y, (x.shape[-1],), g, be, 1e-5)
    if "gelu" in form:
        y = F.gelu(y)
    (y * dy.to(dt)).sum().backward()
    dx = xx.grad if acc is None else xx.grad + acc.to(dt)
    return dx, *(None if p is None else p.grad for p in (g, be, b))


@pytest.mark.parametrize("form", ROW_FORMS)
@pytest.mark.parametrize("C", [32, 128, 1024, 2048])
@pytest.mark.parametrize("N", [1, 36, 257])
def test_rows_backward(N, C, form):
    """Every form the forward uses: LN (fp32 out; accumulating into the residual gradient in place),
    h += GELU(x + bias) (the positional step: dx = dy gelu'(x + bias)), GELU alone, LN with a bf16 out."""
    need_gpu()
    from mlvae_hip import ops
    g_ = torch.Generator().manual_seed(N * 7 + C)
    x, dy = torch.randn(N, C, generator=g_) * 1.5, torch.randn(N, C, generator=g_)
    ln = form.startswith("ln")
    gamma = 1 + 0.1 * torch.randn(C, generator=g_) if ln else None
    beta = 0.1 * torch.randn(C, generator=g_) if ln else None
    bias = 0.1 * torch.randn(C, generator=g_) if form == "bias_gelu_res" else None
    acc = torch.randn(N, C, generator=g_) if form == "ln" else None
    r64 = row_ref(form, x, dy, bias, gamma, beta, acc, torch.float64)
    r32 = row_ref(form, x, dy, bias, gamma, beta, acc, torch.float32)
    cu = lambda t: None if t is None else t.cuda()

    def run():
        a = cu(acc)
        return ops.w2v_rows_bwd(dy.cuda(), x.cuda(), bias=cu(bias), gamma=cu(gamma), beta=cu(beta),
                                gelu="gelu" in form, acc=a, out_f32=a if a is not None else form != "ln_bf16",
                                out_bf16=form == "ln_bf16")
    f32, b16, dg, db = run()
    what = f"rows_bwd {form} N={N} C={C}"
    if form == "ln_bf16":
        assert f32 is None and b16.dtype == torch.bfloat16
        held(b16.float(), r64[0], r32[0].bfloat16().float(), what + " dx (bf16)")
    else:
        held(f32, r64[0], r32[0], what + " dx")
    if ln:
        held(dg, r64[1], r32[1], what + " dgamma")
        held(db, r64[2], r32[2], what + " dbeta")
    if bias is not None:  # the bias gradient is the existing column sum of the row kernel's output
        held(ops.w2v_colsum(f32), r64[3], r32[3], what + " dbias")
    again = run()
    for a, b in zip((f32, b16, dg, db), again):
        assert (a is None and b is None) or torch.equal(a, b)


# ------------------------------------------------------------------ whole-tensor norm backward
@pytest.mark.parametrize("shape", [(1, 1, 4), (36, 128), (4097, 1), (3, 50, 1024)])  # 4097: one past a workgroup's 4096
def test_norm_backward(shape):
    need_gpu()
    from mlvae_hip import ops
    g = torch.Generator().manual_seed(sum(shape))
    x, dy = torch.randn(shape, generator=g) * 2 + 0.5, torch.randn(shape, generator=g)

    def ref(dt):
        xx = x.to(dt).clone().requires_grad_(True)
        (F.layer_norm(xx, xx.shape) * dy.to(dt)).sum().backward()
        return xx.grad
    xc = x.cuda()
    stats = ops.w2v_tensor_stats(xc)
    xhat = ops.w2v_scale_shift(xc, stats)
    dx = ops.w2v_norm_bwd(dy.cuda(), xhat, stats)
    held(dx, ref(torch.float64), ref(torch.float32), f"norm_bwd {shape}")
    assert torch.equal(dx, ops.w2v_norm_bwd(dy.cuda(), xhat, stats))


# ------------------------------------------------------------------ positional conv gradients
@functools.lru_cache(maxsize=None)
def pos_case(B, T, C, G, K, seed):
    g = torch.Generator().manual_seed(seed)
    Cg = C // G
    h, dpc = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    w = torch.randn(C, Cg, K, generator=g) / (Cg * K) ** 0.5

    def ref(dt, autocast=False):
        hh, ww = h.to(dt).clone().requires_grad_(True), w.to(dt).clone().requires_grad_(True)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            y = F.conv1d(hh.transpose(1, 2), ww, None, padding=K // 2, groups=G)[:, :, :-1].transpose(1, 2)
        (y.to(dt) * dpc.to(dt)).sum().backward()
        return hh.grad, ww.grad
    return h, dpc, w, ref(torch.float64), ref(torch.float32), ref(torch.float32, True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("T,C,G,K", [(1, 128, 4, 16), (12, 128, 4, 16), (40, 128, 4, 16), (50, 1024, 16, 128)])
def test_pos_conv_gradients(T, C, G, K, prec):
    """The input gradient (the overlapping-row GEMM on the regrouped gradient against the tap-reversed,
    in / out-swapped weight) and the weight gradient (overlapping rows on the B side, frames along the
    product's K dimension: B T is not a multiple of 8), elementwise on the first and last K/2 frames."""
    need_gpu()
    from mlvae_hip import ops
    B, Cg = 3, C // G
    h, dpc, w, r64, r32, r16 = pos_case(B, T, C, G, K, 11 + T)
    yard = r32 if prec == "fp32" else r16
    ad = torch.float32 if prec == "fp32" else torch.bfloat16
    wc = w.cuda()
    wrev = wc.view(G, Cg, Cg, K).flip(-1).permute(0, 2, 3, 1).reshape(G, Cg, K * Cg).to(ad).contiguous()
    dpcc = dpc.cuda()
    dpr = ops.w2v_regroup(dpcc, G, K, out_dtype=ad)
    dh = ops.w2v_pos_conv_dx(dpr, wrev, T, C, torch.zeros(B, T, C, device="cuda"))
    hp = ops.w2v_regroup(h.cuda(), G, K, out_dtype=ad)
    dwg = ops.w2v_pos_conv_dw(ops.w2v_cast(dpcc, ad), hp, T, C)
    dw = dwg.view(G, Cg, K, Cg).permute(0, 1, 3, 2).reshape(C, Cg, K)
    what = f"pos conv T={T} C={C} G={G} K={K} {prec}"
    held(dh, r64[0], yard[0], what + " dh")
    held(dw, r64[1], yard[1], what + " dw")
    edge = sorted(set(range(min(K // 2, T))) | set(range(max(T - K // 2, 0), T)))
    held(dh[:, edge], r64[0][:, edge], yard[0][:, edge], what + " dh, the frames at the zero padding")
    assert torch.equal(dwg, ops.w2v_pos_conv_dw(ops.w2v_cast(dpcc, ad), hp, T, C))
