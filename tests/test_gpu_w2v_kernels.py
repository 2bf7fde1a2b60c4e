"""The wav2vec2 encoder's kernels (csrc/w2v.hip through mlvae_hip.ops.w2v_*) one by one against
float64 torch on the CPU.

Tolerance rule ("The wav2vec2 encoder"): the yardstick is the same torch
operation on the same input in float32 (for fp32 operands / outputs) or under bf16 autocast (for
bf16 operands); its maximum and relative-RMS error against float64 are computed here, and the
device's must be at most 4 x those (4: a different summation order and the MFMA's accumulation).
A bf16 OUTPUT of an fp32 computation is held to 4 x the error of rounding the float32 result to
bf16 (the format's precision).  Every figure is printed before it is asserted.
"""
import pytest
import torch
import torch.nn.functional as F

import w2v_ref as R
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu
EPS = 1e-5


def held(got, ref64, yard, what):
    """Device error <= 4 x the yardstick's, maximum and relative RMS."""
    e, y = R.errors(got.detach().cpu(), ref64), R.errors(yard, ref64)
    print(f"{what}: device (max {e[0]:.3e}, rms {e[1]:.3e}), yardstick (max {y[0]:.3e}, rms {y[1]:.3e})")
    assert torch.isfinite(got).all(), what
    assert e[0] <= 4 * y[0] and e[1] <= 4 * y[1], (what, e, y)


def bf16_exact(t):
    return t.bfloat16().float()


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ tensor statistics
@pytest.mark.parametrize("n", [1, 1000, 70001])  # one element; no multiple of the block's 256; 18 workgroups
def test_tensor_stats(n):
    need_gpu()
    from mlvae_hip import ops
    x = torch.randn(n, generator=gen(n)) * 0.7 + 0.5
    x64 = x.double()
    mean, var = x64.mean(), x64.var(unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    stats = ops.w2v_tensor_stats(x.cuda())
    again = ops.w2v_tensor_stats(x.cuda())
    assert torch.equal(stats, again)  # fixed-order sums
    got = stats.cpu().double()
    print(f"n={n}: mean {got[0].item():.9e} (ref {mean.item():.9e}), rstd {got[1].item():.9e} (ref {rstd.item():.9e})")
    # fp64 sums rounded once to fp32: half an ulp of the value (2^-24), held to 2^-23
    assert abs(got[0] - mean) <= 2.0 ** -23 * abs(mean) + 1e-12
    assert abs(got[1] - rstd) <= 2.0 ** -23 * rstd
    out = ops.w2v_scale_shift(x.cuda(), stats)
    held(out, F.layer_norm(x64, x64.shape), F.layer_norm(x, x.shape), f"layer_norm over all {n}")


# ------------------------------------------------------------------ conv layer 0
@pytest.mark.parametrize("C", [32, 512])
@pytest.mark.parametrize("N", [10, 400, 4000])  # T0 = 1, 79, 799
def test_conv0(N, C):
    need_gpu()
    from mlvae_hip import ops
    g = gen(N + C)
    B, K, S = 2, 10, 5
    wav = torch.randn(B, N, generator=g) * 0.2
    w = torch.randn(C, 1, K, generator=g) / K ** 0.5
    b, ga, be = torch.randn(C, generator=g) * 0.1, 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)

    def ref(dt, autocast=False):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            x = F.layer_norm(wav.to(dt), wav.shape)
            y = F.conv1d(x.unsqueeze(1), w.to(dt), b.to(dt), stride=S).transpose(1, 2)
            return F.gelu(F.layer_norm(y, (C,), ga.to(dt), be.to(dt), EPS))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert r64.shape[1] == (N - K) // S + 1
    dev = lambda t: t.cuda()
    stats = ops.w2v_tensor_stats(dev(wav))
    for dt in (torch.float32, torch.bfloat16):
        got = ops.w2v_conv0(dev(wav), stats, dev(w[:, 0].contiguous()), dev(b), dev(ga), dev(be), S, EPS, out_dtype=dt)
        assert got.dtype == dt and got.shape == r64.shape
        yard = r32 if dt == torch.float32 else bf16_exact(r32)
        held(got.float(), r64, yard, f"conv0 N={N} C={C} {dt}")


# ------------------------------------------------------------------ the row kernel
MODES = ["ln", "ln_gelu", "ln_both", "gelu_bias", "pos_form"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [32, 512, 1024])
def test_rows(C, mode):
    need_gpu()
    from mlvae_hip import ops
    g = gen(C)
    N = 37  # four rows per workgroup: a ragged last one
    x = torch.randn(N, C, generator=g) * 1.5 + 0.3
    bias, ga, be = 0.1 * torch.randn(C, generator=g), 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    res = torch.randn(N, C, generator=g)

    def ref(dt):
        X, Bi, G, Be, Rs = (t.to(dt) for t in (x, bias, ga, be, res))
        if mode == "ln":
            return F.layer_norm(X, (C,), G, Be, EPS)
        if mode in ("ln_gelu", "ln_both"):
            return F.gelu(F.layer_norm(X, (C,), G, Be, EPS))
        if mode == "gelu_bias":
            return F.gelu(X + Bi)
        return Rs + F.gelu(X + Bi)

    r64, r32 = ref(torch.float64), ref(torch.float32)
    d = lambda t: t.cuda()
    if mode == "ln":
        f32, b16 = ops.w2v_rows(d(x), gamma=d(ga), beta=d(be), eps=EPS, out_f32=True)
    elif mode == "ln_gelu":
        f32, b16 = ops.w2v_rows(d(x), gamma=d(ga), beta=d(be), eps=EPS, gelu=True, out_bf16=True)
    elif mode == "ln_both":
        f32, b16 = ops.w2v_rows(d(x), gamma=d(ga), beta=d(be), eps=EPS, gelu=True, out_f32=True, out_bf16=True)
    elif mode == "gelu_bias":
        f32, b16 = ops.w2v_rows(d(x), bias=d(bias), gelu=True, out_bf16=True)
    else:
        h = d(res)
        f32, b16 = ops.w2v_rows(d(x), bias=d(bias), gelu=True, res=h, out_f32=h)  # in place on the residual
        assert f32 is h
    assert (f32 is None) == (mode in ("ln_gelu", "gelu_bias")) and (b16 is None) == (mode in ("ln", "pos_form"))
    if f32 is not None:
        held(f32, r64, r32, f"rows {mode} C={C} fp32")
    if b16 is not None:
        assert b16.dtype == torch.bfloat16
        held(b16.float(), r64, bf16_exact(r32), f"rows {mode} C={C} bf16")


# ------------------------------------------------------------------ conv layers as GEMMs over overlapping rows
# (K, Tin): the last output frame's window ends exactly at the input's last element (the A
# operand's rows end past M lda: the descriptor-range case), and one frame shorter
@pytest.mark.parametrize("K,Tin,C", [(3, 41, 32), (3, 40, 32), (2, 40, 32), (2, 39, 32), (3, 41, 512), (2, 40, 512)])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_conv_gemm(K, Tin, C, prec):
    need_gpu()
    from mlvae_hip import ops
    g = gen(K * 100 + Tin)
    B, S = 2, 2
    x = bf16_exact(torch.randn(B, Tin, C, generator=g))           # bf16-representable: both paths read
    w = bf16_exact(torch.randn(C, C, K, generator=g) / (C * K) ** 0.5)  # the same values
    b = 0.1 * torch.randn(C, generator=g)
    Tout = (Tin - K) // S + 1
    assert ((Tout - 1) * S + K == Tin) == ((K, Tin) in ((3, 41), (2, 40)))

    def ref(dt, autocast=False):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            return F.conv1d(x.to(dt).transpose(1, 2), w.to(dt), b.to(dt), stride=S).transpose(1, 2).float()

    r64 = ref(torch.float64).double()
    yard = ref(torch.float32) if prec == "fp32" else ref(torch.float32, autocast=True)
    dt = torch.float32 if prec == "fp32" else torch.bfloat16
    W = w.permute(0, 2, 1).reshape(C, K * C).contiguous()  # [Cout][K][Cin]
    got = ops.w2v_conv_gemm(x.cuda().to(dt), W.cuda().to(dt), b.cuda(), K, S)
    assert got.shape == (B, Tout, C)
    held(got, r64, yard, f"conv-gemm K={K} Tin={Tin} C={C} {prec}")
    held(got[:, -2:], r64[:, -2:], yard[:, -2:], f"conv-gemm K={K} Tin={Tin} C={C} {prec}, the last two frames")
    # elementwise on the last two frames: a zeroed window tail would be off by a whole term
    tol = 4 * (yard[:, -2:].double() - r64[:, -2:]).abs().max().item()
    assert (got[:, -2:].cpu().double() - r64[:, -2:]).abs().max().item() <= tol


# ------------------------------------------------------------------ the positional conv
@pytest.mark.parametrize("T,K,G,C", [(1, 16, 4, 128), (15, 16, 4, 128), (16, 16, 4, 128), (37, 16, 4, 128),
                                     (130, 128, 16, 1024)])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_pos_conv(T, K, G, C, prec):
    need_gpu()
    from mlvae_hip import ops
    g = gen(T + K)
    B = 2 if C == 128 else 1
    h = torch.randn(B, T, C, generator=g)
    v = torch.randn(C, C // G, K, generator=g) / (K * C // G) ** 0.5
    gn = v.norm(dim=(0, 1), keepdim=True) * (1 + 0.1 * torch.rand(1, 1, K, generator=g))
    bias = 0.1 * torch.randn(C, generator=g)

    def ref(dt, autocast=False):
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            w = R.fold_pos_conv(gn.to(dt), v.to(dt))
            pos = F.conv1d(h.to(dt).transpose(1, 2), w, bias.to(dt), padding=K // 2, groups=G)[:, :, :-1]
            return (h.to(dt) + F.gelu(pos).transpose(1, 2)).float()

    r64 = ref(torch.float64).double()
    yard = ref(torch.float32) if prec == "fp32" else ref(torch.float32, autocast=True)
    dt = torch.float32 if prec == "fp32" else torch.bfloat16
    Cg = C // G
    W = R.fold_pos_conv(gn, v).view(G, Cg, Cg, K).permute(0, 1, 3, 2).reshape(G, Cg, K * Cg).contiguous()
    hd = h.cuda()
    hp = ops.w2v_regroup(hd, G, K, out_dtype=dt)
    assert hp.shape == (B, G, T + K, Cg)
    exp = torch.zeros(B, G, T + K, Cg)
    exp[:, :, K // 2:K // 2 + T] = h.view(B, T, G, Cg).permute(0, 2, 1, 3)
    assert torch.equal(hp.float().cpu(), exp if prec == "fp32" else bf16_exact(exp))
    pc = ops.w2v_pos_conv(hp, W.cuda().to(dt), T, C)
    ops.w2v_rows(pc.view(B * T, C), bias=bias.cuda(), gelu=True, res=hd.view(B * T, C), out_f32=hd.view(B * T, C))
    held(hd, r64, yard, f"pos-conv T={T} K={K} G={G} C={C} {prec}")
