"""The CRDNN front end's kernels (csrc/conv2d.hip) through mlvae_hip.ops, against the fp64 CPU
restatement tests/crdnn_front_ref.py on the SAME bf16-rounded operands.

* Conv2d 3x3 (reflect "same"): forward, input gradient and weight gradient at 2e-5 max-relative
  (the bound tests/test_gpu_conv.py holds Conv1d to), bias gradient 1e-5; a second launch of the
  weight gradient gives equal bits.  Shapes: the direct Cin = 1 layer; T = F = 2 (both reflected
  borders fold inward); tiles crossing time rows and utterances; odd F; the recipe's K = 1152 with
  M no tile multiple; K = 2304 (both on the LDS-staged kernel of Cout % 128 == 0, forward and input
  gradient); and M = 33020 / 65792 positions, where the direct kernel takes its wider form (64
  positions per wave).
* LayerNorm(F, C) + LeakyReLU [+ frequency pool + keep mask]: forward, dx, d gamma, d beta at 2e-5,
  equal bits on a second launch, a zeroed keep bin, an exact tie in a pooled pair.  The random
  cases zero the cotangent where the fp64 pre-activation is within 1e-4 of the LeakyReLU kink or a
  pooled pair within 1e-4 of a tie: there the derivative is discontinuous and an fp32 and an fp64
  evaluation may fall on different sides (at 4.6 M elements about one does).
* Time pool at T = 2, 5 (odd) and 64."""
import pytest
import torch

import crdnn_front_ref as R
from gpu_utils import need_gpu, rel_err

pytestmark = pytest.mark.gpu

CONV_SHAPES = [(2, 5, 6, 1, 16), (1, 2, 2, 16, 16), (3, 37, 10, 16, 32), (2, 70, 13, 32, 16),
               (1, 40, 120, 128, 128), (1, 33, 60, 256, 256),
               # enough workgroups for the direct kernel's 64-positions-per-wave form, M no tile multiple: the
               # input gradient of the first (N = 16; its forward is the LDS form with one masked K chunk), the
               # forward of the second (N = 64)
               (2, 130, 127, 16, 256), (2, 128, 257, 16, 64)]


@pytest.fixture(autouse=True)
def _bf16_products():
    from mlvae_hip import ops
    with ops.precision("bf16"):
        yield


def _conv_case(B, T, F, Cin, Cout):
    torch.manual_seed(B * 1000 + T * 10 + Cin)
    x = torch.randn(B, T, F) if Cin == 1 else torch.randn(B, T, F, Cin)
    w = torch.randn(Cout, Cin, 3, 3) / (9 * Cin) ** 0.5
    return x, w, torch.randn(Cout), torch.randn(B, T, F, Cout)


@pytest.mark.parametrize("B,T,F,Cin,Cout", CONV_SHAPES)
def test_conv2d_forward_and_gradients(B, T, F, Cin, Cout):
    need_gpu()
    from mlvae_hip import ops
    x, w, b, dy = _conv_case(B, T, F, Cin, Cout)
    xr = x.double().requires_grad_(Cin > 1)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = R.conv3x3(xr, wr, br, bf16=True)
    ref.backward(dy.double())

    def run():
        xd = x.cuda().requires_grad_(Cin > 1)
        wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        y = ops.conv2d_3x3(xd, wd, bd)
        y.backward(dy.cuda())
        torch.cuda.synchronize()
        return y.detach(), xd.grad, wd.grad, bd.grad

    y, dx, dw, db = run()
    assert y.shape == (B, T, F, Cout)
    errs = {"y": rel_err(y, ref), "dw": rel_err(dw, wr.grad), "db": rel_err(db, br.grad)}
    if Cin > 1:
        errs["dx"] = rel_err(dx, xr.grad)
    print(f"conv2d {(B, T, F, Cin, Cout)}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["y"] < 2e-5 and errs["dw"] < 2e-5 and errs["db"] < 1e-5
    assert Cin == 1 or errs["dx"] < 2e-5
    _, dx2, dw2, db2 = run()  # deterministic: a second launch gives the same bits
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and (Cin == 1 or torch.equal(dx, dx2))


def test_conv2d_rejects_what_it_cannot_run():
    need_gpu()
    from mlvae_hip import ops
    x = torch.randn(1, 4, 4, 16, device="cuda")
    with pytest.raises(ValueError):
        ops.conv2d_3x3(x, torch.randn(24, 16, 3, 3, device="cuda"))  # Cout no multiple of 16
    with pytest.raises(ValueError):
        ops.conv2d_3x3(torch.randn(1, 4, 4, 8, device="cuda"), torch.randn(16, 8, 3, 3, device="cuda"))
    with pytest.raises(ValueError):
        ops.conv2d_3x3(x, torch.randn(16, 16, 5, 5, device="cuda"))
    with pytest.raises(ValueError):
        ops.conv2d_3x3(torch.randn(1, 1, 4, 16, device="cuda"), torch.randn(16, 16, 3, 3, device="cuda"))  # T = 1
    with pytest.raises(ValueError):  # the features carry no gradient
        ops.conv2d_3x3(torch.randn(1, 4, 4, device="cuda", requires_grad=True), torch.randn(16, 1, 3, 3, device="cuda"))
    with ops.precision("fp32"), pytest.raises(RuntimeError, match="bf16"):  # never bf16 silently
        ops.conv2d_3x3(x, torch.randn(16, 16, 3, 3, device="cuda"))


def _ln_ref(x, g, b, pool, keep):
    y = R.ln_act(x, g, b)
    return R.freq_pool(y, keep) if pool else y


def _safe_cotangent(x, g, b, pool, dy, margin=1e-4):
    """dy with zeros where the reference's derivative is within `margin` of a discontinuity."""
    with torch.no_grad():
        z = torch.nn.functional.layer_norm(x, tuple(x.shape[2:]), g, b, 1e-5)
        near = z.abs() < margin
        if pool:
            Fo = x.shape[2] // 2
            # LeakyReLU is increasing: the pooled pair ties where its pre-activations do
            z, near = z[:, :, :2 * Fo], near[:, :, :2 * Fo]
            near = near[:, :, 0::2] | near[:, :, 1::2] | ((z[:, :, 0::2] - z[:, :, 1::2]).abs() < margin)
        assert near.sum().item() <= max(2, 1e-3 * near.numel())  # the check still covers the rest
        return torch.where(near, torch.zeros_like(dy), dy)


LN_CASES = [(1, 1, 2, 16, False, False), (2, 1, 2, 16, True, True), (1, 7, 13, 16, False, False),
            (1, 7, 13, 16, True, True), (3, 100, 120, 128, False, False), (3, 100, 120, 128, True, True),
            (2, 3, 13, 16, True, False)]


@pytest.mark.parametrize("B,T,F,C,pool,masked", LN_CASES)
def test_layer_norm_act_pool_dropout(B, T, F, C, pool, masked):
    need_gpu()
    from mlvae_hip import ops
    torch.manual_seed(B + 3 * T + F)
    x = torch.randn(B, T, F, C) * 1.5 + 0.3
    g, b = 1.0 + 0.2 * torch.randn(F, C), 0.2 * torch.randn(F, C)
    keep = None
    if masked:
        keep = (torch.rand(B, F // 2) >= 0.15).float() / 0.85
        keep[0, 0] = 0.0  # a zeroed bin
        keep[-1, -1] = 1.0 / 0.85  # and a kept one
    Fo = F // 2 if pool else F
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, g, b))
    ref = _ln_ref(xr, gr, br, pool, keep)
    dy = _safe_cotangent(x.double(), g.double(), b.double(), pool, torch.randn(B, T, Fo, C, dtype=torch.float64))
    ref.backward(dy)

    def run():
        xd, gd, bd = (t.cuda().requires_grad_(True) for t in (x, g, b))
        y = ops.layer_norm_fc_act(xd, gd, bd, pool=pool, keep=keep.cuda() if keep is not None else None)
        y.backward(dy.float().cuda())
        torch.cuda.synchronize()
        return y.detach(), xd.grad, gd.grad, bd.grad

    y, dx, dg, db = run()
    assert y.shape == (B, T, Fo, C)
    if masked:
        assert torch.count_nonzero(y[0, :, 0]) == 0
    errs = {"y": rel_err(y, ref), "dx": rel_err(dx, xr.grad), "dgamma": rel_err(dg, gr.grad),
            "dbeta": rel_err(db, br.grad)}
    print(f"ln {(B, T, F, C, pool, masked)}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v < 2e-5 for v in errs.values()), errs
    if pool and F % 2:  # the dropped odd bin gets no parameter gradient
        assert torch.count_nonzero(dg[F - 1]) == 0 and torch.count_nonzero(db[F - 1]) == 0
    _, dx2, dg2, db2 = run()
    assert torch.equal(dg, dg2) and torch.equal(db, db2) and torch.equal(dx, dx2)


def test_pool_tie_keeps_the_lower_bin():
    """Both bins of pair 1 hold the same inputs and the same affine: an exact tie in fp32 and in
    fp64.  The gradient goes to the lower bin (torch's max_pool2d keeps the first maximum)."""
    need_gpu()
    from mlvae_hip import ops
    torch.manual_seed(5)
    B, T, F, C = 2, 3, 6, 16
    x = torch.randn(B, T, F, C)
    g, b = 1.0 + 0.2 * torch.randn(F, C), 0.2 * torch.randn(F, C)
    x[:, :, 3], g[3], b[3] = x[:, :, 2], g[2], b[2]
    dy = torch.randn(B, T, F // 2, C, dtype=torch.float64)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, g, b))
    R.freq_pool(R.ln_act(xr, gr, br)).backward(dy)
    xd, gd, bd = (t.cuda().requires_grad_(True) for t in (x, g, b))
    y = ops.layer_norm_fc_act(xd, gd, bd, pool=True)
    y.backward(dy.float().cuda())
    assert torch.count_nonzero(gd.grad[3]) == 0 and torch.count_nonzero(bd.grad[3]) == 0
    assert torch.count_nonzero(bd.grad[2]) == C and torch.count_nonzero(br.grad[3]) == 0
    for got, want in ((xd.grad, xr.grad), (gd.grad, gr.grad), (bd.grad, br.grad)):
        assert rel_err(got, want) < 2e-5


@pytest.mark.parametrize("T", [2, 5, 64])
def test_time_pool(T):
    need_gpu()
    from mlvae_hip import ops
    torch.manual_seed(T)
    B, F, C = 3, 5, 16
    x = torch.randn(B, T, F, C)
    x[:, 1] = torch.where(torch.rand(B, F, C) < 0.3, x[:, 0], x[:, 1])  # exact ties: the earlier frame wins
    dy = torch.randn(B, T // 2, F, C)
    xr = x.double().requires_grad_(True)
    ref = R.time_pool(xr)
    ref.backward(dy.double())
    xd = x.cuda().requires_grad_(True)
    y = ops.time_pool(xd)
    y.backward(dy.cuda())
    assert y.shape == (B, T // 2, F, C)
    assert torch.equal(y.cpu().double(), ref.detach()) and torch.equal(xd.grad.cpu().double(), xr.grad)
