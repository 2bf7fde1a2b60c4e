"""The wav2vec2 conv stack's backward on the device (csrc/w2v.hip, ops.W2VConvFn;
modules.wav2vec2.Wav2Vec2(freeze=False, train_feature_extractor=True)): layer 0's fused backward, the
strided conv's input and weight gradients, every parameter's gradient of the whole encoder, one layer
at the real conv widths and one Adam step.

Tolerance rule (tests/w2v_grad_ref.held): per tensor, 4 x the error against float64 of the same
autograd in float32 (precision 'fp32') or in bf16 (autocast for the encoder, operands rounded to
bf16 first for the ops), maximum and relative RMS, floored at 2^-23 relative.  The float64 truth of
the op tests is F.conv1d + layer_norm + gelu autograd on the CPU (tests/w2v_conv_grad_ref.py).
Measured on an MI355X (largest maximum error over the tensors and cases of a group: device, yardstick;
the worst single device / yardstick ratio of the relative RMS, bound 4):

                                      fp32 device  yardstick  ratio    bf16 device  yardstick  ratio
    conv0_bwd dw                        7.7e-06     6.7e-05    0.77
    conv0_bwd dbias                     7.7e-05     3.1e-04    1.21
    conv0_bwd dgamma / dbeta            1.4e-05     2.0e-05    1.05
    conv_dx, 32 <-> 64                  2.9e-06     1.6e-06    1.94      1.3e-02     1.3e-02    1.00
    conv_dx, 512 -> 512                 2.6e-06     3.6e-06    1.00      8.4e-03     8.4e-03    1.00
    conv_dw, 32 <-> 64                  8.3e-06     1.2e-05    0.79      1.1e-01     1.1e-01    1.00
    conv_dw, 512 -> 512                 1.2e-05     2.2e-05    0.74      1.3e-01     1.3e-01    1.00
    w2v_tiny  feature_extractor.0.*     3.6e-04     4.0e-04    2.65      4.9e+00     3.9e+00    1.10
    w2v_tiny  feature_extractor.1-6.*   2.9e-04     1.8e-04    2.99      3.7e+00     5.0e+00    1.41
    w2v_tiny  projection and upward     5.2e-05     3.6e-05    2.53      5.6e-01     7.8e-01    1.36
    w2v_tiny_d32  feature_extractor.*   2.5e-04     2.8e-04    1.79      2.9e+00     8.8e+00    0.79
    w2v_tiny_d32  projection and upward 3.8e-05     2.8e-05    2.32      4.1e-01     9.6e-01    0.92
    real widths, layer 0                2.2e-05     2.3e-05    1.10      1.8e-01     3.5e-01    0.71
    real widths, layers 1-6             2.7e-05     2.2e-05    1.25      1.8e-01     3.9e-01    0.62
(bf16 ops: device and yardstick round the same operands to bf16 and accumulate in fp32, so they agree to
fp32 rounding against a bf16-sized error.)
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import w2v_conv_grad_ref as CR
import w2v_ref as R
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECS = ["fp32", "bf16"]
EPS = 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------- layer 0
def _conv0_case(C, K, stride, N, B, use_stats, seed):
    g = _gen(seed)
    lens = [N, max(K, (3 * N) // 4), max(K, N // 2)][:B]
    wav = R.ragged_wav(seed, B=B, N=N, lens=tuple(lens))
    w = torch.randn(C, K, generator=g) / K ** 0.5
    b = 0.1 * torch.randn(C, generator=g)
    ga = 1.0 + 0.1 * (2 * torch.rand(C, generator=g) - 1)
    be = 0.1 * torch.randn(C, generator=g)
    T0 = (N - K) // stride + 1
    dout = torch.randn(B, T0, C, generator=g)
    stats = None
    if use_stats:
        w64 = wav.double()
        stats = torch.tensor([w64.mean().item(), (w64.var(unbiased=False) + 1e-5).rsqrt().item()])
    return wav, stats, w, b, ga, be, dout


def _conv0_check(C, K, stride, N, B, use_stats, what):
    from mlvae_hip import ops
    wav, stats, w, b, ga, be, dout = _conv0_case(C, K, stride, N, B, use_stats, 7 * C + K + stride)
    r64 = CR.conv0_grads(wav, stats, w, b, ga, be, stride, dout, EPS, torch.float64)
    yard = CR.conv0_grads(wav, stats, w, b, ga, be, stride, dout, EPS, torch.float32)
    dev = lambda t: None if t is None else t.cuda()
    run = lambda: ops.w2v_conv0_bwd(dev(wav), dev(stats), dev(w), dev(b), dev(ga), dev(be), stride, dev(dout), EPS)
    got, again = run(), run()
    for n, a, a2, r, y in zip(("dw", "dbias", "dgamma", "dbeta"), got, again, r64, yard):
        assert torch.equal(a, a2), (what, n)  # fixed-order sums: a rerun gives the same bits
        CR.held(a, r, y, f"conv0_bwd {what} {n}")
    return got


@pytest.mark.parametrize("use_stats", [True, False])
@pytest.mark.parametrize("K,stride", [(10, 5), (10, 2), (4, 5), (4, 2)])
@pytest.mark.parametrize("C", [32, 48, 512])
def test_conv0_bwd(C, K, stride, use_stats):
    """B = 3 ragged; N: the first from 401 on at which B T0 is no multiple of the frames a wave walks
    and no utterance ends where a wave's span does (several workgroups, 15 or 16 frames a wave)."""
    need_gpu()

    def spans(N):
        T0 = (N - K) // stride + 1
        frames = 3 * T0
        waves = 4 * min(256, -(-(-(-frames // 16)) // 4))
        per = -(-frames // waves)
        return frames % per and all((b * T0) % per for b in (1, 2))
    N = next(n for n in range(401, 500) if spans(n))
    _conv0_check(C, K, stride, N, 3, use_stats, f"C={C} K={K} s={stride} stats={use_stats}")


@pytest.mark.parametrize("C", [48, 512])
def test_conv0_bwd_fewer_frames_than_waves(C):
    """3 frames, 4 waves: the idle wave's partial row must be zeros (it is summed like the others)."""
    need_gpu()
    from mlvae_hip import _lib
    K, stride, N = 10, 5, 10
    # a workspace that starts out dirty: what an idle wave would leave if it wrote nothing
    from mlvae_hip.ops import _core
    ws = _core._workspace(_lib.lib().mlvae_w2v_conv0_bwd_workspace_size(3, 1, C, K), "w2v_conv0_bwd")
    ws.fill_(1e30)
    _conv0_check(C, K, stride, N, 3, True, f"C={C} 3 frames")


def test_conv0_bwd_refusals():
    need_gpu()
    from mlvae_hip import ops
    wav = torch.zeros(2, 100).cuda()
    p = lambda *s: torch.zeros(*s).cuda()
    with pytest.raises(ValueError, match="unsupported"):
        ops.w2v_conv0_bwd(wav, None, p(513, 10), p(513), p(513), p(513), 5, p(2, 19, 513))
    with pytest.raises(ValueError, match="dout is"):
        ops.w2v_conv0_bwd(wav, None, p(32, 10), p(32), p(32), p(32), 5, p(2, 18, 32))


# --------------------------------------------------------------------------- layers >= 1: dx and dw
def _conv_case(k, stride, Cin, Cout, B, T_in, seed):
    g = _gen(seed)
    x = torch.randn(B, T_in, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5
    dy = torch.randn(B, (T_in - k) // stride + 1, Cout, generator=g)
    return x, w, dy


def _conv_check(k, stride, Cin, Cout, B, T_in, prec, what, leak=True):
    from mlvae_hip import ops
    bf = prec == "bf16"
    ad = torch.bfloat16 if bf else torch.float32
    x, w, dy = _conv_case(k, stride, Cin, Cout, B, T_in, 13 * k + stride + Cin)
    Tout = dy.shape[1]
    dx64, dw64 = CR.conv_grads(x, w, dy, stride, torch.float64)
    dxy, dwy = CR.conv_grads(x, w, dy, stride, torch.float32, round_bf16=bf)
    W = ops.w2v_conv_dx_weights(w.cuda(), stride, ad)
    dx = ops.w2v_conv_dx(dy.cuda(), W, k, stride, T_in)
    assert dx.shape == (B, T_in, Cin) and dx.dtype == torch.float32
    assert torch.equal(dx, ops.w2v_conv_dx(dy.cuda(), W, k, stride, T_in))  # a rerun: the same bits
    used = (Tout - 1) * stride + k
    assert torch.equal(dx[:, used:], torch.zeros_like(dx[:, used:]))  # the unused trailing frames: exactly 0
    CR.held(dx, dx64, dxy, f"conv_dx {what} {prec}")
    xo, dyo = x.cuda().to(ad), dy.cuda().to(ad)
    dw = ops.w2v_conv_dw(dyo, xo, k, stride)
    assert dw.shape == (Cout, k * Cin) and torch.equal(dw, ops.w2v_conv_dw(dyo, xo, k, stride))
    CR.held(dw.view(Cout, k, Cin).permute(0, 2, 1), dw64, dwy, f"conv_dw {what} {prec}")
    # dy read from the guarded copy, as W2VConvFn reads it: the same bits
    dyp, pf = ops.w2v_conv_pad(dy.cuda(), k, stride, T_in, ad)
    assert torch.equal(dw, ops.w2v_conv_dw(dyp[:, pf:pf + Tout], xo, k, stride))
    if leak and B > 1:  # nothing crosses an utterance boundary: another utterance's dy does not reach this dx
        dy2 = dy.clone()
        dy2[1] = torch.randn(dy2[1].shape, generator=_gen(5)) * 3
        dx2 = ops.w2v_conv_dx(dy2.cuda(), W, k, stride, T_in)
        assert torch.equal(dx2[0], dx[0]) and torch.equal(dx2[2:], dx[2:]) and not torch.equal(dx2[1], dx[1])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cin,Cout", [(32, 64), (64, 32)])
@pytest.mark.parametrize("k,stride", [(3, 2), (2, 2), (3, 1), (4, 3), (3, 3)])
def test_conv_dx_dw(k, stride, Cin, Cout, prec):
    """B = 3, T_in = 41 + (a remainder that leaves (T_in - k) % stride != 0 where stride > 1)."""
    need_gpu()
    T_in = 41
    while stride > 1 and (T_in - k) % stride == 0:
        T_in += 1
    _conv_check(k, stride, Cin, Cout, 3, T_in, prec, f"k={k} s={stride} {Cin}->{Cout} T_in={T_in}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k,stride", [(3, 2), (2, 2), (3, 1), (4, 3), (3, 3)])
def test_conv_dx_dw_one_output_frame(k, stride, prec):
    need_gpu()
    _conv_check(k, stride, 32, 64, 3, k + stride - 1, prec, f"k={k} s={stride} Tout=1")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k,T_in", [(3, 101), (2, 51)])
def test_conv_dx_dw_real_width(k, T_in, prec):
    need_gpu()
    _conv_check(k, 2, 512, 512, 2, T_in, prec, f"512->512 k={k} s=2 T_in={T_in}", leak=False)


def test_conv_dx_refuses_a_stride_longer_than_the_kernel():
    need_gpu()
    from mlvae_hip import ops
    with pytest.raises(ValueError, match="1 <= stride <= k"):
        ops.w2v_conv_dx_weights(torch.zeros(32, 32, 2).cuda(), 3, torch.float32)
    W = ops.w2v_conv_dx_weights(torch.zeros(32, 32, 2).cuda(), 2, torch.float32)
    with pytest.raises(ValueError, match="1 <= stride <= k"):
        ops.w2v_conv_dx(torch.zeros(1, 5, 32).cuda(), W + W[:1], 2, 3, 16)


# --------------------------------------------------------------------------- the whole encoder
@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["config"]))
    return torch.from_numpy(z["wav"]), cfg, R.fill_state(cfg, int(z["seed"]))


def cotangent(shape, seed=3):
    return torch.randn(shape, generator=_gen(seed))


@functools.lru_cache(maxsize=None)
def oracle(name, output_norm, normalize_wav):
    """{mode: (out, grads)} of the fixture's batch: computed once, shared, read only."""
    wav, cfg, state = fixture(name)
    cot = cotangent((wav.shape[0], R.n_frames(cfg, wav.shape[1]), cfg["hidden_size"]))
    return cot, {m: CR.encoder_grads(state, cfg, wav, cot, m, normalize_wav=normalize_wav, output_norm=output_norm)
                 for m in ("fp64", "fp32", "bf16")}


def encoder(cfg, state, prec, kind="whole", **kw):
    from modules.wav2vec2 import Wav2Vec2
    extra = {"whole": dict(freeze=False, train_feature_extractor=True),
             "head": dict(freeze=False, freeze_feature_extractor=True), "frozen": {}}[kind]
    m = Wav2Vec2(config=cfg, precision=prec, **extra, **kw)
    m.load_state_dict(state)
    return m.cuda()


def grads_of(m, wav, cot):
    for p in m.parameters():
        p.grad = None
    out = m(wav)
    (out * cot).sum().backward()
    return out.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}


CASES = [("w2v_tiny", True, True), ("w2v_tiny", False, True), ("w2v_tiny_d32", True, True),
         ("w2v_tiny_d32", False, True), ("w2v_tiny", True, False)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,output_norm,normalize_wav", CASES)
def test_encoder_gradients(name, output_norm, normalize_wav, prec):
    need_gpu()
    wav, cfg, state = fixture(name)
    cot, ref = oracle(name, output_norm, normalize_wav)
    (_, g64), (_, gy) = ref["fp64"], ref[prec]
    kw = dict(output_norm=output_norm, normalize_wav=normalize_wav)
    m = encoder(cfg, state, prec, **kw)
    m.train()
    out, got = grads_of(m, wav.cuda(), cot.cuda())
    assert list(got) == [k for k in state if CR.trainable(k)] and set(got) == set(g64)
    what = f"{name} {prec} output_norm={output_norm} normalize_wav={normalize_wav}"
    for k in g64:
        CR.held(got[k], g64[k], gy[k], f"{what} d {k}")
    # the forward's bits are the frozen module's
    assert torch.equal(out, encoder(cfg, state, prec, "frozen", **kw)(wav.cuda()))
    # above the conv stack: the same kernels in the same order as with a frozen extractor
    out_h, got_h = grads_of(encoder(cfg, state, prec, "head", **kw), wav.cuda(), cot.cuda())
    assert torch.equal(out, out_h)
    for k in got_h:
        assert torch.equal(got[k], got_h[k]), k
    assert set(got) - set(got_h) == {k for k in state if k.startswith("feature_extractor.")}
    # train() / eval() and a rerun: the same bits
    m.eval()
    out2, got2 = grads_of(m, wav.cuda(), cot.cuda())
    assert torch.equal(out, out2)
    for k in got:
        assert torch.equal(got[k], got2[k]), k


@pytest.mark.parametrize("prec", PRECS)
def test_conv_stack_at_the_real_widths(prec):
    """conv_dim = [512] * 7 under a one-layer hidden-64 encoder, B = 1, N = 400 + 320 * 9 (10 frames)."""
    need_gpu()
    cfg = dict(R.TINY_D32, conv_dim=[512] * 7, num_hidden_layers=1)
    state = R.fill_state(cfg, 41)
    N = 400 + 320 * 9
    wav = R.ragged_wav(41, B=1, N=N, lens=(N - 700,))
    cot = cotangent((1, 10, 64))
    _, g64 = CR.encoder_grads(state, cfg, wav, cot, "fp64")
    _, gy = CR.encoder_grads(state, cfg, wav, cot, prec)
    _, got = grads_of(encoder(cfg, state, prec), wav.cuda(), cot.cuda())
    for k in g64:
        if k.startswith("feature_extractor."):
            CR.held(got[k], g64[k], gy[k], f"real-width {prec} d {k}")


def test_adam_step_moves_the_conv_masters():
    """One Adam step of the wav2vec2 group: every conv master moves, the next forward uses the moved
    weights (the kernel-side copies, the regrouped dgrad weights included, follow the version counters)
    and equals a fresh module's loaded from the new state_dict; so does the next backward."""
    need_gpu()
    from mlvae_hip import optim as hip_optim
    wav, cfg, state = fixture("w2v_tiny")
    cot = cotangent((wav.shape[0], R.n_frames(cfg, wav.shape[1]), cfg["hidden_size"])).cuda()
    m = encoder(cfg, state, "bf16")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = hip_optim.Adam(torch.nn.ModuleDict({"wav2vec2": m}).parameters(), lr=1e-4)
    out0 = m(wav.cuda())
    (out0 * cot).sum().backward()
    opt.step()
    torch.cuda.synchronize()
    after = {k: v.clone() for k, v in m.state_dict().items()}
    for k in after:
        assert torch.equal(after[k], before[k]) == (k == "masked_spec_embed"), k
    out1, g1 = grads_of(m, wav.cuda(), cot)
    assert not torch.equal(out1, out0)
    fresh = encoder(cfg, {k: v.cpu() for k, v in after.items()}, "bf16")
    out_f, g_f = grads_of(fresh, wav.cuda(), cot)
    assert torch.equal(out1, out_f)
    assert torch.equal(out1, encoder(cfg, {k: v.cpu() for k, v in after.items()}, "bf16", "frozen")(wav.cuda()))
    for k in g1:
        assert torch.equal(g1[k], g_f[k]), k
