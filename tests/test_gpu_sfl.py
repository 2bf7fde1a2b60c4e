"""The MD_VAE_sfl kernels on the HIP path (csrc/pi.hip through mlvae_hip.ops.sfl_losses /
pi_sample_k):

* sfl_losses and its gradients against the reference's own expression in torch fp64 on the same
  fp32 inputs (Categorical, the one-hot bmm log-likelihood, .entropy(), F.mse_loss, .mean(-1);
  ref:src/models/MD_VAE_sfl/model.py:170-186): outputs 1e-5, gradients 1e-4 relative-max, the
  bounds of test_gpu_pi.py.  n in {1, 63, 65, 257} (one short of a 64-lane wave, one past it, one
  past a 256-thread block) x K in {1, 2, 5} x (F, Z) in {(1,1), (8,4), (80,32), (83,5)} (the
  float4 row reads and the scalar ones), and n one past the forward's grid-stride cap
  (4096 blocks x 16 frames) with K = 1, F = Z = 3;
* rows with logit gaps of 200 and 1e4: the entropy term exactly +-0, everything finite;
* recon / kld / pi_nll get no gradient, logits and baseline do; a rerun is bit-equal;
* pi_sample_k: K = 1 bit-equal to pi_sample, (u >= p0) per draw with injected uniforms, draw k
  equal to the existing kernel at offset + k n, eval is the argmax and refuses K > 1;
* the C entries' argument checks."""
import pytest
import torch
import torch.nn.functional as F_
from torch.distributions import Categorical

from gpu_utils import P, need_gpu, rel_err, stream
from mlvae_hip import _lib, ops

pytestmark = pytest.mark.gpu

W = (0.7, 0.3, 0.5)
GRID_CAP = 4096 * 16  # frames one pass of the forward's grid covers (csrc/pi.hip grid_sfl)


def _inputs(n, K, F, Z, seed, logits=None):
    g = torch.Generator().manual_seed(seed)
    d = {"logits": torch.randn(1, n, 2, generator=g) * 3 if logits is None else logits.view(1, n, 2)}
    lab = torch.randint(0, 2, (K, 1, n), generator=g).float()
    d["sampled_pi"] = torch.stack([1 - lab, lab], dim=-1)          # [K, 1, n, 2]
    d["recon"] = torch.randn(K, 1, n, F, generator=g) ** 2 + 0.5   # loss-like: positive, O(1)
    d["kld"] = torch.randn(K, 1, n, Z, generator=g) ** 2
    d["pi_nll"] = torch.rand(1, n, generator=g) * 2 + 0.1
    d["baseline"] = torch.randn(1, n, generator=g) - 1.0
    d["d"] = [torch.randn(1, n, generator=g) for _ in range(3)]
    return d


def _reference(d):
    """The reference's loop in fp64: (rif, neg_entropy, baseline_loss), (dlogits, dbaseline)."""
    l = d["logits"].double().requires_grad_(True)
    b = d["baseline"].double().requires_grad_(True)
    K, n = d["sampled_pi"].shape[0], l.shape[1]
    dist = Categorical(logits=l)
    rif = ent = bl = 0
    for k in range(K):
        s = d["sampled_pi"][k].double()
        ll = torch.bmm(dist.logits.reshape(n, 1, 2), s.reshape(n, 2, 1)).reshape(1, n)
        reward = -(W[0] * d["recon"][k].double().mean(-1) + W[1] * d["kld"][k].double().mean(-1)
                   + W[2] * d["pi_nll"].double())
        rif = rif + (reward - b.detach()) * -ll
        ent = ent + -dist.entropy()
        bl = bl + F_.mse_loss(b, reward, reduction="none")
    out = (rif / K, ent / K, bl / K)
    grads = torch.autograd.grad(sum((o * g.double()).sum() for o, g in zip(out, d["d"])), [l, b])
    return [o.detach() for o in out], grads


def _run(d, grad_all=False):
    x = d["logits"].cuda().requires_grad_(True)
    b = d["baseline"].cuda().requires_grad_(True)
    rest = [d[k].cuda().requires_grad_(grad_all) for k in ("recon", "kld", "pi_nll")]
    out = ops.sfl_losses(x, d["sampled_pi"].cuda(), rest[0], rest[1], rest[2], b, *W)
    torch.autograd.backward(out, [g.cuda() for g in d["d"]])
    return out, (x.grad, b.grad), rest


def _check(d, tag):
    ref_out, ref_grad = _reference(d)
    out, grad, _ = _run(d)
    n = d["logits"].shape[1]
    worst_o = worst_g = 0.0
    for name, o, r in zip(("rif", "neg_entropy", "baseline_loss"), out, ref_out):
        assert o.shape == (1, n)
        e = rel_err(o, r)
        worst_o = max(worst_o, e)
        assert e < 1e-5, (tag, name, e)
    for name, o, r in zip(("dlogits", "dbaseline"), grad, ref_grad):
        assert o.shape == r.shape
        e = rel_err(o, r)
        worst_g = max(worst_g, e)
        assert e < 1e-4, (tag, name, e)
    print(f"sfl {tag}: outputs {worst_o:.3e} gradients {worst_g:.3e}")
    return out, grad


@pytest.mark.parametrize("F,Z", [(1, 1), (8, 4), (80, 32), (83, 5)])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_sfl_losses_match_fp64(n, K, F, Z):
    need_gpu()
    _check(_inputs(n, K, F, Z, seed=1000 * n + 10 * K + F), f"n={n} K={K} F={F} Z={Z}")


def test_sfl_losses_past_the_grid_stride_cap():
    need_gpu()
    n = GRID_CAP + 1
    out, grad = _check(_inputs(n, 1, 3, 3, seed=3), f"n={n} K=1 F=3 Z=3")
    # the wrapped frame is written, by the forward and by the backward
    ref_out, _ = _reference(_inputs(n, 1, 3, 3, seed=3))
    assert abs(out[0][0, -1].item() - ref_out[0][0, -1].item()) <= 1e-5 * ref_out[0].abs().max().item()
    assert bool(torch.isfinite(grad[0][0, -1]).all())


def test_sfl_losses_saturated_rows():
    need_gpu()
    rows = [(100.0, -100.0), (-100.0, 100.0), (5000.0, -5000.0), (-5000.0, 5000.0)]
    n = 70
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(n, 2, generator=g)
    for j, row in enumerate(rows):  # each once per label, across the wave boundary
        logits[60 + 2 * j] = torch.tensor(row)
        logits[61 + 2 * j] = torch.tensor(row)
    d = _inputs(n, 2, 8, 4, seed=4, logits=logits)
    lab = d["sampled_pi"][..., 1]
    lab[:, 0, 60:68] = torch.tensor([0.0, 1.0] * 4)
    d["sampled_pi"] = torch.stack([1 - lab, lab], dim=-1)
    out, grad = _check(d, "saturated rows")
    assert bool((out[1][0, 60:68] == 0).all()), out[1][0, 60:68]  # +-0 exactly
    for t in (*out, *grad):
        assert bool(torch.isfinite(t).all())
    # the drawn label on the saturated side costs nothing, the other one the whole gap
    nll_gap = [200.0, 200.0, 1e4, 1e4]
    reward = -(W[0] * d["recon"].mean(-1) + W[1] * d["kld"].mean(-1) + W[2] * d["pi_nll"])
    for j, gap in enumerate(nll_gap):
        for c in (0, 1):
            i = 60 + 2 * j + c
            sat = 0 if j % 2 == 0 else 1  # the class with all of the mass
            want = sum((reward[k, 0, i] - d["baseline"][0, i]) * (0.0 if int(lab[k, 0, i]) == sat else gap)
                       for k in range(2)) / 2
            assert out[0][0, i].item() == pytest.approx(want.item(), rel=1e-5, abs=1e-6)


def test_sfl_losses_gradient_flow():
    need_gpu()
    d = _inputs(65, 2, 8, 4, seed=5)
    _, grad, rest = _run(d, grad_all=True)
    assert all(t.requires_grad and t.grad is None for t in rest)  # recon, kld, pi_nll: detached
    assert grad[0] is not None and grad[1] is not None
    assert bool(grad[0].ne(0).any()) and bool(grad[1].ne(0).any())
    x = d["logits"].cuda().requires_grad_(True)
    out = ops.sfl_losses(x, d["sampled_pi"].cuda(), d["recon"].cuda(), d["kld"].cuda(),
                         d["pi_nll"].cuda(), d["baseline"].cuda(), *W)
    assert all(o.requires_grad for o in out)
    out[2].sum().backward()  # baseline_loss alone sends nothing into the logits
    assert not bool(x.grad.ne(0).any())


def test_sfl_losses_rerun_is_bit_equal():
    need_gpu()
    d = _inputs(257, 5, 83, 5, seed=6)
    a_out, a_grad, _ = _run(d)
    b_out, b_grad, _ = _run(d)
    for a, b in zip((*a_out, *a_grad), (*b_out, *b_grad)):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------- pi_sample_k
def _logits(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 2, generator=g) * 3


def test_pi_sample_k_one_draw_is_pi_sample():
    need_gpu()
    l = _logits(3, 65, 1).cuda()
    torch.manual_seed(77)
    a = ops.pi_sample(l, True)
    torch.manual_seed(77)
    b = ops.pi_sample_k(l, 1, True)
    assert b.shape == (1, 3, 65, 2) and torch.equal(a, b[0])
    assert 0 < a[..., 1].mean().item() < 1
    e = ops.pi_sample_k(l, 1, False)  # eval: the argmax
    lab = torch.argmax(l, dim=-1).float()
    assert torch.equal(e[0], torch.stack([1 - lab, lab], dim=2))
    with pytest.raises(ValueError):
        ops.pi_sample_k(l, 2, False)


@pytest.mark.parametrize("B,T,K", [(1, 1, 2), (3, 65, 5), (2, 300, 3)])
def test_pi_sample_k_injected_uniforms(B, T, K):
    need_gpu()
    l = _logits(B, T, 7 * B + T)
    g = torch.Generator().manual_seed(3)
    u = torch.rand(K, B, T, generator=g)
    p0 = 1.0 / (1.0 + torch.exp(l[..., 1] - l[..., 0]))  # fp32, as the kernel
    keep = (u - p0).abs() >= 1e-4  # a last-ulp difference in expf cannot move these
    dropped = 1.0 - keep.float().mean().item()
    assert dropped < 0.01, dropped
    ref = (u >= p0).float()
    out = ops.pi_sample_k(l.cuda(), K, True, u=u.cuda()).cpu()
    assert out.shape == (K, B, T, 2)
    assert torch.equal(out.sum(-1), torch.ones(K, B, T)) and bool(((out == 0) | (out == 1)).all())
    for k in range(K):
        assert torch.equal(out[k, ..., 1][keep[k]], ref[k][keep[k]])
        assert torch.equal(out[k, ..., 0][keep[k]], 1 - ref[k][keep[k]])
    with pytest.raises(ValueError):
        ops.pi_sample_k(l.cuda(), K, True, u=u[0].cuda())  # one draw's uniforms for K draws


def test_pi_sample_k_draw_k_is_the_stream_at_offset_k_n():
    need_gpu()
    lib = _lib.lib()
    n, K, seed, off = 65, 5, 123456789, 7
    l = _logits(1, n, 9).view(n, 2).cuda()
    out = torch.zeros(K, n, 2, device="cuda")
    assert lib.mlvae_pi_sample_k(n, K, P(l), None, seed, off, 1, P(out), stream()) == 0
    for k in range(K):
        one = torch.zeros(n, 2, device="cuda")
        assert lib.mlvae_pi_sample(n, P(l), None, seed, off + k * n, 1, P(one), stream()) == 0
        assert torch.equal(out[k], one), k
    assert len({tuple(out[k, :, 1].tolist()) for k in range(K)}) == K  # the draws differ


def test_sfl_c_entries_check_arguments():
    need_gpu()
    lib = _lib.lib()
    n, K, F, Z = 4, 2, 3, 2
    z = lambda *s: torch.zeros(*s, device="cuda")
    l, s, rc, kl, nl, b = z(n, 2), z(K, n, 2), z(K, n, F), z(K, n, Z), z(n), z(n)
    rw, o1, o2, o3, dl, db = z(K, n), z(n), z(n), z(n), z(n, 2), z(n)
    # eval with K > 1 is an error status; K < 1 too
    assert lib.mlvae_pi_sample_k(n, 2, P(l), None, 0, 0, 0, P(s), stream()) != 0
    assert "pi_sample_k" in _lib.last_error()
    assert lib.mlvae_pi_sample_k(n, 0, P(l), None, 0, 0, 1, P(s), stream()) != 0
    assert lib.mlvae_pi_sample_k(n, 1, P(l), None, 0, 0, 0, P(s), stream()) == 0
    assert lib.mlvae_pi_sample_k(n, 2, None, None, 0, 0, 1, P(s), stream()) != 0
    assert lib.mlvae_pi_sample_k(n, 2, P(l), None, 0, 0, 1, None, stream()) != 0
    fwd = [P(l), P(s), P(rc), P(kl), P(nl), P(b), 0.7, 0.3, 0.5, P(rw), P(o1), P(o2), P(o3)]
    assert lib.mlvae_sfl_fwd(n, K, F, Z, *fwd, stream()) == 0
    for i in (0, 1, 2, 3, 4, 5, 9, 10, 11, 12):
        a = list(fwd)
        a[i] = None
        assert lib.mlvae_sfl_fwd(n, K, F, Z, *a, stream()) != 0, i
    assert "sfl_fwd" in _lib.last_error()
    for bad in ((0, F, Z), (K, 0, Z), (K, F, 0)):
        assert lib.mlvae_sfl_fwd(n, *bad, *fwd, stream()) != 0
    bwd = [P(l), P(s), P(rw), P(b), P(o1), P(o2), P(o3), P(dl), P(db)]
    assert lib.mlvae_sfl_bwd(n, K, *bwd, stream()) == 0
    for i in range(len(bwd)):
        a = list(bwd)
        a[i] = None
        assert lib.mlvae_sfl_bwd(n, K, *a, stream()) != 0, i
    assert "sfl_bwd" in _lib.last_error()
    assert lib.mlvae_sfl_bwd(n, 0, *bwd, stream()) != 0
    # n == 0 is a no-op, whatever the pointers
    assert lib.mlvae_pi_sample_k(0, 2, None, None, 0, 0, 1, None, stream()) == 0
    assert lib.mlvae_sfl_fwd(0, K, F, Z, *([None] * 6), 0.0, 0.0, 0.0, *([None] * 4), stream()) == 0
    assert lib.mlvae_sfl_bwd(0, K, *([None] * 9), stream()) == 0
    torch.cuda.synchronize()
