"""modules.crdnn.CNNFront on the HIP path against the CPU restatement tests/crdnn_front_ref.py:
CNNFront(120, 2, (16, 32), (3, 3), 0.15, True) on B = 3, T = 41 with an injected Dropout2d keep
mask -- the output [3, 20, 30 * 32] against the bf16-operand fp64 restatement (1e-4 in norm), every
parameter gradient against the same restatement's (2e-2: what remains is bf16 ties of fp32 against
fp64 sums and the few LeakyReLU / pool-argmax decisions they flip), and the output against the plain
fp32 restatement (1e-2: bf16 operands) -- the three bounds test_conv_vae_module_matches_oracle
uses, for the same reasons.  Eval mode ignores the dropout."""
import pytest
import torch

import crdnn_front_ref as R
from gpu_utils import need_gpu, norm_rel

pytestmark = pytest.mark.gpu

B, T, F = 3, 41, 120


def _front():
    from modules.crdnn import CNNFront
    torch.manual_seed(7)
    net = CNNFront(F, 2, (16, 32), (3, 3), 0.15, True)
    with torch.no_grad():  # an affine that is not the identity
        for n, p in net.named_parameters():
            if ".norm_" in n:
                p.add_(0.1 * torch.randn_like(p))
    return net


def test_front_matches_the_restatement():
    need_gpu()
    from mlvae_hip import ops
    net = _front()
    params = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x = torch.randn(B, T, F)
    keep = [(torch.rand(B, 60) >= 0.15).float() / 0.85, (torch.rand(B, 30) >= 0.15).float() / 0.85]
    keep[0][1, 7] = 0.0
    cot = torch.randn(B, T // 2, 30 * 32, dtype=torch.float64)
    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    ref = R.front(p64, x, 2, True, keep=keep, bf16=True)
    (ref * cot).sum().backward()
    plain = R.front(params, x, 2, True, keep=keep, dtype=torch.float32)
    net = net.cuda().train()
    with ops.precision("bf16"):
        out = net(x.cuda(), keep=[k.cuda() for k in keep])
        assert out.shape == (B, T // 2, 30 * 32) and net.output_size == 30 * 32
        (out * cot.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    e_ref, e_plain = norm_rel(out, ref), norm_rel(out, plain)
    errs = {k: norm_rel(v.grad, p64[k].grad) for k, v in net.named_parameters()}
    print(f"\n[CNNFront vs bf16-operand fp64] out {e_ref:.2e}; vs plain fp32 {e_plain:.2e}; grads " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert len(errs) == 16
    assert e_ref < 1e-4
    assert e_plain < 1e-2
    for k, v in errs.items():
        assert v < 2e-2, (k, v)


def test_eval_mode_ignores_dropout():
    need_gpu()
    from mlvae_hip import ops
    net = _front().cuda()
    x = torch.randn(2, 10, F, device="cuda")
    with ops.precision("bf16"), torch.no_grad():
        net.eval()
        a, b = net(x), net(x)
        net.train()
        torch.manual_seed(1)
        c = net(x)
        torch.manual_seed(2)
        d = net(x)
    assert torch.equal(a, b)
    assert not torch.equal(c, d) and not torch.equal(a, c)  # training draws a mask per call
    assert (c == 0).all(dim=1).any()  # a dropped (utterance, bin) is zero at every frame
