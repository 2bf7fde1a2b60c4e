"""The MD-VAE pi path on the HIP path (csrc/pi.hip through mlvae_hip.ops.pi_sample / pi_nll):

* pi_nll and its gradient against torch.distributions.Categorical(logits).log_prob and autograd
  in fp64 on the same fp32 inputs: outputs 1e-5, gradients 1e-4 relative-max (the fp32 module
  bounds of test_gpu_md.py); exact values at the saturated rows; -1 labels past T_i;
* pi_sample: (u >= p0) with injected uniforms, argmax in eval (a tie gives 0), one-hot rows,
  seed reproducibility, the draw frequency, no flip at saturation;
* the label error word (ValueError) and the C entries' argument checks.
Shapes: one frame, an odd size, one past a 256-thread block, and one past the 4096 x 256 grid
(the grid-stride loop).  Reference ops: ref:src/models/MD_VAE/model.py:119-150."""
import math

import pytest
import torch
from torch.distributions import Categorical

from gpu_utils import P, need_gpu, rel_err, stream
from mlvae_hip import _lib, ops

pytestmark = pytest.mark.gpu

BIG = 2 ** 20 + 5
SHAPES = [(1, 1), (3, 17), (2, 300), (1, BIG)]
FORCED = [(0.0, 0.0), (80.0, -80.0), (-80.0, 80.0)]


def _logits(B, T, seed):
    """randn * 3 with the forced rows (0,0), (80,-80), (-80,80) at the front of the last
    utterance, each twice (one per label), where the shape has room."""
    g = torch.Generator().manual_seed(seed)
    l = torch.randn(B, T, 2, generator=g) * 3
    if T >= 6:
        for j, row in enumerate(FORCED):
            l[B - 1, 2 * j] = torch.tensor(row)
            l[B - 1, 2 * j + 1] = torch.tensor(row)
    elif B * T == 1:
        l[0, 0] = torch.tensor(FORCED[0])
    return l


def _labels(B, T, seed):
    """0/1 labels, -1 past T_i (the first utterance ends early when it can); the forced rows get
    label 0 then 1."""
    g = torch.Generator().manual_seed(seed + 1)
    lab = torch.randint(0, 2, (B, T), generator=g, dtype=torch.int32)
    if B > 1 and T > 2:
        lab[0, T - T // 3:] = -1
    if T >= 6:
        lab[B - 1, 0:6] = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.int32)
    return lab


@pytest.mark.parametrize("B,T", SHAPES)
def test_pi_nll_matches_categorical_fp64(B, T):
    need_gpu()
    l = _logits(B, T, 11 * B + T)
    lab = _labels(B, T, 11 * B + T)
    ref_l = l.double().requires_grad_(True)
    ref = -Categorical(logits=ref_l).log_prob(lab.clamp_min(0).double())
    g = torch.Generator().manual_seed(5)
    dn = torch.randn(B, T, generator=g)
    (dref,) = torch.autograd.grad((ref * dn.double()).sum(), ref_l)

    x = l.cuda().requires_grad_(True)
    nll = ops.pi_nll(x, lab.cuda())
    assert nll.shape == (B, T)
    nll.backward(dn.cuda())
    e_out, e_grad = rel_err(nll, ref), rel_err(x.grad, dref)
    print(f"pi_nll ({B},{T}): out {e_out:.3e} grad {e_grad:.3e}")
    assert e_out < 1e-5
    assert e_grad < 1e-4
    out = nll.detach().cpu()
    if T >= 6:
        got = out[B - 1, :6].tolist()
        assert abs(got[0] - math.log(2)) < 1e-7 and abs(got[1] - math.log(2)) < 1e-7
        assert got[2:] == [0.0, 160.0, 160.0, 0.0]
    elif B * T == 1:
        assert abs(out[0, 0].item() - math.log(2)) < 1e-7


def _p0(l):
    return 1.0 / (1.0 + torch.exp(l[..., 1] - l[..., 0]))  # fp32, as the kernel


@pytest.mark.parametrize("B,T", SHAPES)
def test_pi_sample_injected_uniforms(B, T):
    need_gpu()
    l = _logits(B, T, 7 * B + T)
    g = torch.Generator().manual_seed(3)
    u = torch.rand(B, T, generator=g)
    p0 = _p0(l)
    keep = (u - p0).abs() >= 1e-4  # a last-ulp difference in expf cannot move these
    dropped = 1.0 - keep.float().mean().item()
    assert dropped <= 0.01, dropped
    ref = (u >= p0).float()
    out = ops.pi_sample(l.cuda(), True, u=u.cuda()).cpu()
    assert out.shape == (B, T, 2)
    assert torch.equal(out.sum(-1), torch.ones(B, T)) and bool(((out == 0) | (out == 1)).all())
    assert torch.equal(out[..., 1][keep], ref[keep])
    assert torch.equal(out[..., 0][keep], 1 - ref[keep])
    if T >= 6:  # saturated rows: (80,-80) -> label 0, (-80,80) -> label 1 whatever u is
        assert out[B - 1, 2:6, 1].tolist() == [0.0, 0.0, 1.0, 1.0]


@pytest.mark.parametrize("B,T", SHAPES)
def test_pi_sample_eval_is_argmax(B, T):
    need_gpu()
    l = _logits(B, T, 13 * B + T)
    out = ops.pi_sample(l.cuda(), False).cpu()
    lab = torch.argmax(l, dim=-1).float()
    assert torch.equal(out, torch.stack([1 - lab, lab], dim=2))
    if T >= 6 or B * T == 1:  # the tie row gives label 0
        assert out[B - 1, 0].tolist() == [1.0, 0.0]


def test_pi_sample_seeded_draws():
    need_gpu()
    l = torch.tensor([0.0, 1.0]).repeat(BIG, 1).view(1, BIG, 2).cuda()
    torch.manual_seed(1234)
    a = ops.pi_sample(l, True)
    torch.manual_seed(1234)
    b = ops.pi_sample(l, True)
    assert torch.equal(a, b)
    c = ops.pi_sample(l, True)  # the next seed of the same stream: another draw
    assert not torch.equal(a, c)
    assert torch.equal(a.sum(-1), torch.ones(1, BIG, device="cuda"))
    freq = a[..., 1].mean().item()
    want = torch.softmax(torch.tensor([0.0, 1.0]), 0)[1].item()
    print(f"label-1 frequency {freq:.5f} against softmax {want:.5f}")
    assert abs(freq - want) < 0.01


def test_pi_sample_saturated_rows_never_flip():
    need_gpu()
    n = 4096
    l = torch.empty(2, n, 2)
    l[0] = torch.tensor([-80.0, 80.0])  # l1 - l0 = +160: always label 1
    l[1] = torch.tensor([80.0, -80.0])  # l1 - l0 = -160: always label 0
    l = l.cuda()
    torch.manual_seed(9)
    for _ in range(3):
        out = ops.pi_sample(l, True)
        assert bool((out[0, :, 1] == 1).all()) and bool((out[1, :, 1] == 0).all())
    for val in (0.0, 1.0 - 2.0 ** -24):  # the ends of the draw's range
        out = ops.pi_sample(l, True, u=torch.full((2, n), val, device="cuda"))
        assert bool((out[0, :, 1] == 1).all()) and bool((out[1, :, 1] == 0).all())


def test_pi_nll_label_error_word():
    need_gpu()
    l = _logits(2, 9, 1).cuda()
    lab = _labels(2, 9, 1)
    bad = lab.clone()
    bad[1, 4] = 2
    with pytest.raises(ValueError):
        ops.pi_nll(l, bad.cuda())
    ops.pi_nll(l, lab.cuda())  # the word is cleared: a valid call passes afterwards
    # unread (sync=False), the bit stays until raise_pi_err reads it
    ops.pi_nll(l, bad.cuda(), sync=False)
    with pytest.raises(ValueError):
        ops.raise_pi_err()
    ops.raise_pi_err()


def test_pi_c_entries_check_arguments():
    need_gpu()
    l = _lib.lib()
    x = torch.zeros(4, 2, device="cuda")
    lab = torch.zeros(4, device="cuda", dtype=torch.int32)
    o = torch.zeros(4, 2, device="cuda")
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    assert l.mlvae_pi_sample(4, None, None, 0, 0, 1, P(o), stream()) != 0
    assert "pi_sample" in _lib.last_error()
    assert l.mlvae_pi_sample(4, P(x), None, 0, 0, 1, None, stream()) != 0
    assert l.mlvae_pi_nll_fwd(4, None, lab.data_ptr(), P(o), P(err), stream()) != 0
    assert l.mlvae_pi_nll_fwd(4, P(x), lab.data_ptr(), P(o), None, stream()) != 0
    assert l.mlvae_pi_nll_bwd(4, None, lab.data_ptr(), P(o), P(o), stream()) != 0
    # n == 0 is a no-op, whatever the pointers
    assert l.mlvae_pi_sample(0, None, None, 0, 0, 1, None, stream()) == 0
    assert l.mlvae_pi_nll_fwd(0, None, None, None, None, stream()) == 0
    assert l.mlvae_pi_nll_bwd(0, None, None, None, None, stream()) == 0
    torch.cuda.synchronize()
    assert err.item() == 0
