"""The random streams over an utterance map (include/mlvae.h; csrc/common.h UttMap): what a
data-parallel shard of an MD recipe draws.

For every drawing entry -- mlvae_randn_rows, mlvae_dropout_rows, mlvae_pi_sample_rows,
mlvae_boundary_fwd_rows / _bwd_rows, mlvae_gmm_latent_fwd_rows --
* the identity map gives the entry it extends, bit for bit;
* the shards [0:2], [2:4] and the uneven [0:3], [3:4] of a global batch of four give the slices of
  the whole-batch call of the existing entry, bit for bit, as plain batches and K-folded
  ([K * B, T, .], MD_VAE_sfl's layout);
* a malformed map is refused; rows past the global batch (fillers) leave the real rows' draws alone.
Then the same through mlvae_hip.ops under an ops.shard context, and masked_mean's global
denominator.  Shapes: B_g = 4, T = 5, rows of 3, 4 and 12 (no multiple of the Philox / dropout
quad, one quad, several), K = 3, dropout 0.15; the boundary and pi logits are near zero so that
both labels occur.  The draws are compared for exact equality; the masked mean's shares add up
to the whole within the fp32 roundings counted in the test."""
import ctypes

import pytest
import torch

from gpu_utils import P, need_gpu, stream
from mlvae_hip import _lib, ops

pytestmark = pytest.mark.gpu

BG, T, K = 4, 5, 3
WIDTHS = [3, 4, 12]
SPLITS = [[(0, 2), (2, 4)], [(0, 3), (3, 4)]]
SHARDS = [s for split in SPLITS for s in split]
SEED = 0x1234567 * 977 + 5
DROP_P = 0.15


def umap(off, seg, stride, total):
    return (ctypes.c_longlong * 4)(off, seg, stride, total)


def plain(lo, hi):
    return umap(lo, hi - lo, hi - lo, BG)


def folded(lo, hi):
    return umap(lo, hi - lo, BG, K * BG)


def fold_slice(whole, lo, hi, lead=0):
    """Rows [lo:hi) of every fold of a [.., K * BG, ...] array whose folded axis is `lead`."""
    sh = whole.shape
    v = whole.reshape(*sh[:lead], K, BG, *sh[lead + 1:])
    idx = [slice(None)] * (lead + 1) + [slice(lo, hi)]
    v = v[tuple(idx)]
    return v.reshape(*sh[:lead], K * (hi - lo), *sh[lead + 1:]).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def ok(rc, what):
    assert rc == 0, f"{what}: status {rc}: {_lib.last_error()}"


# --------------------------------------------------------------------------- randn
def _randn_whole(B, C):
    out = torch.empty(B, T, C, device="cuda")
    ok(_lib.lib().mlvae_randn(out.numel(), SEED, 0, P(out), stream()), "randn")
    return out


def _randn_rows(B, C, m):
    out = torch.full((B, T, C), float("nan"), device="cuda")
    ok(_lib.lib().mlvae_randn_rows(B, T, C, SEED, m, P(out), stream()), "randn_rows")
    return out


@pytest.mark.parametrize("C", WIDTHS)
def test_randn_rows(C):
    need_gpu()
    whole, wholek = _randn_whole(BG, C), _randn_whole(K * BG, C)
    assert torch.equal(_randn_rows(BG, C, umap(0, BG, BG, BG)), whole)
    assert torch.equal(_randn_rows(BG, C, None), whole)
    assert torch.equal(_randn_rows(K * BG, C, umap(0, BG, BG, K * BG)), wholek)
    for lo, hi in SHARDS:
        assert torch.equal(_randn_rows(hi - lo, C, plain(lo, hi)), whole[lo:hi]), (lo, hi)
        assert torch.equal(_randn_rows(K * (hi - lo), C, folded(lo, hi)),
                           fold_slice(wholek, lo, hi)), (lo, hi)
    assert not torch.equal(whole[0:2], whole[2:4])  # the shards differ: an unmapped rank would not


# --------------------------------------------------------------------------- dropout
def _drop_whole(x):
    y = torch.empty_like(x)
    ok(_lib.lib().mlvae_dropout(x.numel(), P(x), P(y), None, SEED, DROP_P, stream()), "dropout")
    return y


def _drop_rows(x, m):
    y = torch.full_like(x, float("nan"))
    B, _, C = x.shape
    ok(_lib.lib().mlvae_dropout_rows(B, T, C, P(x), P(y), SEED, DROP_P, m, stream()), "dropout_rows")
    return y


@pytest.mark.parametrize("C", WIDTHS)
def test_dropout_rows(C):
    need_gpu()
    x, xk = rnd(BG, T, C, seed=C), rnd(K * BG, T, C, seed=C + 1)
    whole, wholek = _drop_whole(x), _drop_whole(xk)
    kept = (wholek != 0).float().mean().item()
    assert 0.6 < kept < 0.99, kept  # both outcomes occur
    assert torch.equal(_drop_rows(x, umap(0, BG, BG, BG)), whole)
    assert torch.equal(_drop_rows(x, None), whole)
    for lo, hi in SHARDS:
        assert torch.equal(_drop_rows(x[lo:hi].contiguous(), plain(lo, hi)), whole[lo:hi]), (lo, hi)
        assert torch.equal(_drop_rows(fold_slice(xk, lo, hi), folded(lo, hi)),
                           fold_slice(wholek, lo, hi)), (lo, hi)
    # in place, as the LSTM backward applies the mask to its input gradient
    y = x[2:4].clone()
    ok(_lib.lib().mlvae_dropout_rows(2, T, C, P(y), P(y), SEED, DROP_P, plain(2, 4), stream()),
       "dropout_rows in place")
    assert torch.equal(y, whole[2:4])


# --------------------------------------------------------------------------- pi
def _pi_whole(logits, k):
    n = logits.numel() // 2
    out = torch.empty(k, *logits.shape, device="cuda")
    ok(_lib.lib().mlvae_pi_sample_k(n, k, P(logits), None, SEED, 0, 1, P(out), stream()), "pi_sample_k")
    return out


def _pi_rows(logits, k, m, train=1):
    out = torch.full((k,) + tuple(logits.shape), float("nan"), device="cuda")
    ok(_lib.lib().mlvae_pi_sample_rows(logits.shape[0], T, k, P(logits), None, SEED, m, train, P(out),
                                       stream()), "pi_sample_rows")
    return out


def test_pi_sample_rows():
    need_gpu()
    l, lk = rnd(BG, T, 2, seed=1, scale=0.1), rnd(K * BG, T, 2, seed=2, scale=0.1)
    whole, wholek = _pi_whole(l, K), _pi_whole(lk, K)
    assert 0.2 < whole[..., 1].mean().item() < 0.8  # both labels occur
    assert torch.equal(_pi_rows(l, K, umap(0, BG, BG, BG)), whole)
    assert torch.equal(_pi_rows(l, K, None), whole)
    # K = 1: mlvae_pi_sample's draw
    one = torch.empty(BG, T, 2, device="cuda")
    ok(_lib.lib().mlvae_pi_sample(BG * T, P(l), None, SEED, 0, 1, P(one), stream()), "pi_sample")
    assert torch.equal(_pi_rows(l, 1, umap(0, BG, BG, BG))[0], one)
    for lo, hi in SHARDS:
        assert torch.equal(_pi_rows(l[lo:hi].contiguous(), K, plain(lo, hi)), whole[:, lo:hi]), (lo, hi)
        assert torch.equal(_pi_rows(l[lo:hi].contiguous(), 1, plain(lo, hi))[0], one[lo:hi]), (lo, hi)
        assert torch.equal(_pi_rows(fold_slice(lk, lo, hi), K, folded(lo, hi)),
                           fold_slice(wholek, lo, hi, lead=1)), (lo, hi)
    # eval: the argmax, nothing drawn
    arg = torch.empty(BG, T, 2, device="cuda")
    ok(_lib.lib().mlvae_pi_sample(BG * T, P(l), None, 0, 0, 0, P(arg), stream()), "pi_sample eval")
    assert torch.equal(_pi_rows(l[2:4].contiguous(), 1, plain(2, 4), train=0)[0], arg[2:4])
    out = torch.empty(K, 2, T, 2, device="cuda")
    assert _lib.lib().mlvae_pi_sample_rows(2, T, K, P(l), None, SEED, plain(0, 2), 0, P(out), stream()) != 0


# --------------------------------------------------------------------------- boundary
def _bnd_inputs(B, seed):
    za, zb = rnd(B, T, seed=seed, scale=0.3), rnd(B, T, seed=seed + 1, scale=0.3)
    g = torch.Generator().manual_seed(seed + 2)
    y = (torch.rand(B, T, generator=g) < 0.4).float().cuda()
    cot = [rnd(B, T, seed=seed + 3 + j) for j in range(3)]
    return za, zb, y, cot


def _bnd(za, zb, y, cot, m, rows):
    l = _lib.lib()
    B = za.shape[0]
    v, bce, kld, dza, dzb = (torch.full_like(za, float("nan")) for _ in range(5))
    if rows:
        ok(l.mlvae_boundary_fwd_rows(B, T, P(za), P(zb), P(y), None, SEED, m, P(v), P(bce), P(kld),
                                     stream()), "boundary_fwd_rows")
        ok(l.mlvae_boundary_bwd_rows(B, T, P(za), P(zb), P(y), None, SEED, m, P(cot[0]), P(cot[1]),
                                     P(cot[2]), P(dza), P(dzb), stream()), "boundary_bwd_rows")
    else:
        ok(l.mlvae_boundary_fwd(B * T, P(za), P(zb), P(y), None, SEED, 0, P(v), P(bce), P(kld),
                                stream()), "boundary_fwd")
        ok(l.mlvae_boundary_bwd(B * T, P(za), P(zb), P(y), None, SEED, 0, P(cot[0]), P(cot[1]),
                                P(cot[2]), P(dza), P(dzb), stream()), "boundary_bwd")
    return torch.stack([v, bce, kld, dza, dzb])  # [5, B, T]


def test_boundary_rows():
    need_gpu()
    za, zb, y, cot = _bnd_inputs(BG, 10)
    zak, zbk, yk, cotk = _bnd_inputs(K * BG, 20)
    whole = _bnd(za, zb, y, cot, None, rows=False)
    wholek = _bnd(zak, zbk, yk, cotk, None, rows=False)
    assert bool(torch.isfinite(whole).all())
    assert 0 < (whole[0] > 0.5).float().mean().item() < 1  # boundary_v on both sides of 0.5
    assert torch.equal(_bnd(za, zb, y, cot, umap(0, BG, BG, BG), rows=True), whole)
    assert torch.equal(_bnd(za, zb, y, cot, None, rows=True), whole)
    for lo, hi in SHARDS:
        c = lambda t: t[lo:hi].contiguous()
        got = _bnd(c(za), c(zb), c(y), [c(t) for t in cot], plain(lo, hi), rows=True)
        assert torch.equal(got, whole[:, lo:hi]), (lo, hi)
        f = lambda t: fold_slice(t, lo, hi)
        got = _bnd(f(zak), f(zbk), f(yk), [f(t) for t in cotk], folded(lo, hi), rows=True)
        assert torch.equal(got, fold_slice(wholek, lo, hi, lead=1)), (lo, hi)
    # the draws differ between the shards: v of equal inputs is not equal
    same = torch.zeros(BG, T, device="cuda")
    w = _bnd(same, same, same, [same + 1] * 3, None, rows=False)
    assert not torch.equal(w[0, 0:2], w[0, 2:4])


# --------------------------------------------------------------------------- GMM latent
def _gmm(Pm, eps, N, Z, m, rows):
    l = _lib.lib()
    B = Pm.shape[0]
    z = torch.full((B, T, N * Z), float("nan"), device="cuda")
    kl = torch.full_like(z, float("nan"))
    w = torch.full((B, T, N), float("nan"), device="cuda")
    ys = torch.full_like(w, float("nan"))
    if rows:
        ok(l.mlvae_gmm_latent_fwd_rows(B, T, N, Z, P(Pm), Pm.shape[-1], P(eps), None, SEED, m, 0.1,
                                       P(z), P(kl), P(w), P(ys), stream()), "gmm_latent_fwd_rows")
    else:
        ok(l.mlvae_gmm_latent_fwd(B * T, N, Z, P(Pm), Pm.shape[-1], P(eps), None, SEED, 0, 0.1,
                                  P(z), P(kl), P(w), P(ys), stream()), "gmm_latent_fwd")
    return torch.cat([z, kl, w, ys], dim=-1)  # [B, T, 2 N Z + 2 N]


@pytest.mark.parametrize("N", WIDTHS)
def test_gmm_latent_rows(N):
    need_gpu()
    Z = 2
    ld = 4 * N * Z + N
    Pm, eps = rnd(BG, T, ld, seed=N, scale=0.2), rnd(BG, T, N * Z, seed=N + 1)
    Pk, epsk = rnd(K * BG, T, ld, seed=N + 2, scale=0.2), rnd(K * BG, T, N * Z, seed=N + 3)
    whole, wholek = _gmm(Pm, eps, N, Z, None, rows=False), _gmm(Pk, epsk, N, Z, None, rows=False)
    hard = wholek[..., 2 * N * Z:2 * N * Z + N].argmax(-1)
    assert hard.unique().numel() > 1  # the Gumbel draws pick more than one component
    assert torch.equal(_gmm(Pm, eps, N, Z, umap(0, BG, BG, BG), rows=True), whole)
    assert torch.equal(_gmm(Pm, eps, N, Z, None, rows=True), whole)
    for lo, hi in SHARDS:
        got = _gmm(Pm[lo:hi].contiguous(), eps[lo:hi].contiguous(), N, Z, plain(lo, hi), rows=True)
        assert torch.equal(got, whole[lo:hi]), (lo, hi)
        got = _gmm(fold_slice(Pk, lo, hi), fold_slice(epsk, lo, hi), N, Z, folded(lo, hi), rows=True)
        assert torch.equal(got, fold_slice(wholek, lo, hi)), (lo, hi)


# --------------------------------------------------------------------------- argument checks
def test_rows_entries_refuse_a_malformed_map():
    need_gpu()
    l = _lib.lib()
    out = torch.zeros(2, T, 4, device="cuda")
    for m in (umap(-1, 2, 2, BG),     # negative offset
              umap(0, 0, 2, BG),      # no utterances per segment
              umap(0, 2, 0, BG),      # no stride between the folds
              umap(0, 2, 2, 0)):      # an empty global batch
        assert l.mlvae_randn_rows(2, T, 4, SEED, m, P(out), stream()) != 0
        assert "map" in _lib.last_error()
        assert l.mlvae_dropout_rows(2, T, 4, P(out), P(out), SEED, DROP_P, m, stream()) != 0
        assert l.mlvae_pi_sample_rows(2, T, 1, P(out), None, SEED, m, 1, P(out), stream()) != 0
        assert l.mlvae_boundary_fwd_rows(2, T, P(out), P(out), P(out), None, SEED, m, P(out), None,
                                         None, stream()) != 0
    assert l.mlvae_randn_rows(0, T, 4, SEED, None, None, stream()) == 0  # empty: a no-op
    assert l.mlvae_randn_rows(2, T, 4, SEED, plain(0, 2), None, stream()) != 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())


def test_filler_rows_past_the_global_batch():
    """A short rank slice: utterance 2 of a global batch of 3 and one filler behind it.  The real
    row draws what the single process draws; the filler's values are finite."""
    need_gpu()
    whole = torch.empty(3, T, 4, device="cuda")
    ok(_lib.lib().mlvae_randn(whole.numel(), SEED, 0, P(whole), stream()), "randn")
    got = torch.full((2, T, 4), float("nan"), device="cuda")
    ok(_lib.lib().mlvae_randn_rows(2, T, 4, SEED, umap(2, 2, 2, 3), P(got), stream()), "randn_rows")
    assert torch.equal(got[0], whole[2]) and bool(torch.isfinite(got[1]).all())
    l3 = rnd(3, T, 2, seed=4, scale=0.1)
    wk = torch.empty(K, 3, T, 2, device="cuda")
    ok(_lib.lib().mlvae_pi_sample_k(3 * T, K, P(l3), None, SEED, 0, 1, P(wk), stream()), "pi_sample_k")
    mine = torch.cat([l3[2:3], torch.zeros(1, T, 2, device="cuda")])
    gk = torch.full((K, 2, T, 2), float("nan"), device="cuda")
    ok(_lib.lib().mlvae_pi_sample_rows(2, T, K, P(mine), None, SEED, umap(2, 2, 2, 3), 1, P(gk), stream()),
       "pi_sample_rows")
    assert torch.equal(gk[:, 0], wk[:, 2]) and bool(torch.isfinite(gk).all())


# --------------------------------------------------------------------------- through mlvae_hip.ops
def _ops_draws(l, za, zb, y, Pm, eps, fold_ctx=None):
    """Every drawing op once, in a fixed order, under torch seed 99."""
    torch.manual_seed(99)
    r = ops.randn((l.shape[0], T, 3))
    p1 = ops.pi_sample(l, True)
    pk = ops.pi_sample_k(l, K, True)
    v, bce, kld = ops.boundary_heads(za, zb, y)
    z, kl, w = ops.GmmLatentFn.apply(Pm, eps, None, 3, 2, 0.1, int(torch.randint(0, 2 ** 62, (1,)).item()))
    return dict(r=r, p1=p1, pk=pk, v=v, bce=bce, kld=kld, z=z, kl=kl, w=w)


def test_ops_shard_context_draws_the_slices():
    need_gpu()
    l = rnd(BG, T, 2, seed=1, scale=0.1)
    za, zb, y, _ = _bnd_inputs(BG, 10)
    Pm, eps = rnd(BG, T, 27, seed=5, scale=0.2), rnd(BG, T, 6, seed=6)
    whole = _ops_draws(l, za, zb, y, Pm, eps)
    assert ops.current_shard() is None
    for lo, hi in SHARDS:
        c = lambda t: t[lo:hi].contiguous()
        with ops.shard(lo, BG):
            got = _ops_draws(c(l), c(za), c(zb), c(y), c(Pm), c(eps))
        assert ops.current_shard() is None
        for k, v in got.items():
            want = whole[k][:, lo:hi] if k == "pk" else whole[k][lo:hi]
            assert torch.equal(v, want), (k, lo, hi)
    # the folded variant: [K * B_l, T, .] rows against the single process's [K * B_g, T, .]
    torch.manual_seed(7)
    wk = ops.randn((K * BG, T, 4))
    for lo, hi in SHARDS:
        torch.manual_seed(7)
        with ops.shard(lo, BG).folded(K):
            got = ops.randn((K * (hi - lo), T, 4))
        assert torch.equal(got, fold_slice(wk, lo, hi)), (lo, hi)
    with ops.shard(0, BG).folded(K):
        with pytest.raises(ValueError):
            ops.randn((K * 2 + 1, T, 4))  # not K folds of a local batch


def test_masked_mean_global_denominator():
    need_gpu()
    loss = rnd(BG, T, 3, seed=3)
    lens = torch.tensor([1.0, 0.6, 0.0, 0.8])  # utterance 2 is a zero-length filler
    whole = ops.masked_mean(loss, lens)
    n = ops.valid_frames(lens, T)
    assert n == 5 + 3 + 0 + 4
    for split in SPLITS + [[(0, 2), (2, 3), (3, 4)]]:  # the last has a shard of the filler alone
        parts = []
        for lo, hi in split:
            x = loss[lo:hi].clone().requires_grad_(True)
            with ops.shard(lo, BG, global_lens=lens):
                s = ops.masked_mean(x, lens[lo:hi])
            assert bool(torch.isfinite(s))
            s.backward()
            parts.append((s.detach(), x.grad))
            assert torch.equal(ops.masked_mean(loss[lo:hi], lens[lo:hi], global_frames=n), s.detach())
        # fp32: each share is rounded twice (the masked sum / B, the rescale), the whole once
        total = sum(p[0].double() for p in parts)
        mag = sum(abs(p[0].item()) for p in parts) + abs(whole.item())
        assert abs(total.item() - whole.item()) <= 4 * 2 ** -24 * mag
        # the gradient 1 / (frames C) per valid element: two roundings against one
        grad = torch.cat([p[1] for p in parts])
        x = loss.clone().requires_grad_(True)
        ops.masked_mean(x, lens).backward()
        assert torch.allclose(grad, x.grad, rtol=4 * 2 ** -24, atol=0)
