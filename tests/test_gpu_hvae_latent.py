"""The fused H-VAE latent kernel (csrc/hvae.hip: mlvae_hvae_latent_fwd / _fwd_rows / _bwd, under
ops.hvae_latent, ops.gmm_collapsed, HierarchicalVAE(fused=True) and GMMVAE.collapsed), fp32.

1. Against the reference's own numbers (tests/golden/make_golden_hvae.py fixtures, draws injected):
   outputs 1e-5 relative-max, parameter / input gradients 1e-4 (test_gpu_hvae.py's bounds); the
   GMM-only mode against apply_weight of the fixture's own outputs, formed on the CPU in float64.
2. Against the composed path on the device (ReparamKLFn + GmmLatentFn + apply_weight + stack), at
   B = 3, T = 33, Z in {5, 32, 70} (8, 32 and 64 lanes per row; 70 loops over the columns), N in
   {1, 3, 5}, soft pi, one case with padded head rows and one with a single row: gmm_weight
   torch.equal, the other outputs 1e-6, dml / dP / dpi 1e-5 (the apply_weight test's bounds: the
   two paths round sums of at most 4 * 70 products differently, ~1e-6 of the largest element).
3. Cotangents left out (NULL in the C ABI): only d_h and d_kl, which is what the recipes send, and
   only d_w.
4. Library draws: the same torch seed gives the same draws fused and composed.
5. mlvae_hvae_latent_fwd_rows over the shards [0:2], [2:3] of three utterances, plain and folded.
6. Bad shapes are refused before any launch."""
import ctypes

import pytest
import torch

from gpu_utils import P, need_gpu, rel_err, stream
from test_oracle_hvae_golden import GMM_CASES, HVAE_CASES, load

pytestmark = pytest.mark.gpu
TAU = 0.1


# --------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("case", HVAE_CASES)
def test_fused_module_matches_reference(case):
    need_gpu()
    from modules.h_vae import HierarchicalVAE
    meta, params, ins, outs, cots, grads, grads_in = load(case)
    m = HierarchicalVAE([meta["F"], meta["E"], meta["E"]], meta["Z"], meta["N"], fused=True)
    m.load_state_dict(dict(params))
    m = m.cuda()
    x = ins["x"].cuda().requires_grad_(True)
    pi = ins["pi"].cuda().requires_grad_(True)
    out = m(x, pi, eps_v=ins["eps_v"].cuda(), eps_g=ins["eps_g"].cuda(), expo=ins["expo"].cuda())
    out = {**{k: v for k, v in out.items() if k != "losses"}, **out["losses"]}
    assert set(out) == set(outs)
    for k, v in outs.items():
        e = rel_err(out[k], v)
        print(f"{case} {k} rel {e:.2e}")
        assert e < 1e-5, k
    sum((out[k] * cots[k].cuda()).sum() for k in outs).backward()
    named = dict(m.named_parameters())
    for k, g in grads.items():
        got = named[k].grad if named[k].grad is not None else torch.zeros_like(named[k])
        e = rel_err(got, g)
        print(f"{case} grad {k} rel {e:.2e}")
        assert e < 1e-4, k
    for k, g in grads_in.items():
        e = rel_err({"x": x, "pi": pi}[k].grad, g)
        print(f"{case} grad_in {k} rel {e:.2e}")
        assert e < 1e-4, k


@pytest.mark.parametrize("case", GMM_CASES)
def test_gmm_only_mode_matches_reference(case):
    need_gpu()
    from modules.gmm_vae import GMMVAE
    meta, params, ins, outs, *_ = load(case)
    N, Z = meta["N"], meta["Z"]
    m = GMMVAE([meta["F"], meta["E"], meta["E"]], Z, N)
    m.load_state_dict(dict(params))
    got = m.cuda().collapsed(ins["x"].cuda(), eps=ins["eps"].cuda(), expo=ins["expo"].cuda())
    assert set(got) == {"weighted_h", "weighted_loss", "gmm_weight"}
    w = outs["gmm_weight"].double()
    lead = w.shape[:-1]
    for key, src in (("weighted_h", "sampled_h"), ("weighted_loss", "loss")):
        want = (w.unsqueeze(-1) * outs[src].double().reshape(*lead, N, Z)).sum(-2)
        e = rel_err(got[key], want)
        print(f"{case} {key} rel {e:.2e}")
        assert e < 1e-5, key
    assert rel_err(got["gmm_weight"], outs["gmm_weight"]) < 1e-5


# --------------------------------------------------------------------------- 2. the composed path
def make_inputs(B, T, Z, N, pad=0, seed=0):
    g = torch.Generator().manual_seed(1000 * Z + 10 * N + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d = {"ml": 0.5 * r(B, T, 2 * Z), "P": 0.5 * r(B, T, 4 * N * Z + N + pad),
         "pi": torch.softmax(r(B, T, 2), -1), "eps_v": r(B, T, Z), "eps_g": r(B, T, N * Z),
         "expo": torch.empty(B, T, N).exponential_(generator=g)}
    d["P"][..., 4 * N * Z:4 * N * Z + N] *= 0.2  # logits near each other: the Gumbel draws decide
    cots = {"mean": r(B, T, Z), "log_var": r(B, T, Z), "sampled_h": r(B, T, Z), "loss": r(B, T, Z),
            "gmm_weight": r(B, T, N)}
    return {k: v.cuda() for k, v in d.items()}, {k: v.cuda() for k, v in cots.items()}


def leaves(d):
    return {k: (v.clone().requires_grad_(True) if k in ("ml", "P", "pi") else v) for k, v in d.items()}


def composed(d, N, Z, seed=0):
    """HierarchicalVAE.forward's unfused stretch on the head outputs."""
    from mlvae_hip import ops
    NZ = N * Z
    ml, Pm = d["ml"], d["P"]
    zv, klv = ops.ReparamKLFn.apply(ml, d["eps_v"])
    z, kl, w = ops.GmmLatentFn.apply(Pm, d["eps_g"], d["expo"], N, Z, TAU, seed)
    v = {"mean": ml[..., :Z], "log_var": ml[..., Z:], "sampled_h": zv, "loss": klv}
    g = {"mean": Pm[..., 2 * NZ:3 * NZ], "log_var": Pm[..., 3 * NZ:4 * NZ], "sampled_h": z, "loss": kl}
    out = {"gmm_weight": w}
    for key in ("mean", "log_var", "sampled_h", "loss"):
        pair = torch.stack([v[key], ops.apply_weight(g[key], w)], dim=2)
        out[key] = ops.apply_weight(pair, d["pi"])
    return out


def fused(d, N, Z, seed=0):
    from mlvae_hip import ops
    mean, log_var, h, kl, w = ops.hvae_latent(d["ml"], d["P"], d["pi"], d["eps_v"], d["eps_g"], d["expo"],
                                              N, Z, TAU, seed)
    return {"gmm_weight": w, "mean": mean, "log_var": log_var, "sampled_h": h, "loss": kl}


def compare(B, T, Z, N, pad=0, keys=("mean", "log_var", "sampled_h", "loss", "gmm_weight")):
    d, cots = make_inputs(B, T, Z, N, pad)
    a, b = leaves(d), leaves(d)
    oa, ob = composed(a, N, Z), fused(b, N, Z)
    assert torch.equal(ob["gmm_weight"], oa["gmm_weight"])
    if B * T > 8 and N > 1:
        assert oa["gmm_weight"].argmax(-1).unique().numel() > 1  # more than one component is drawn
    for k in ("mean", "log_var", "sampled_h", "loss"):
        e = rel_err(ob[k], oa[k])
        print(f"Z={Z} N={N} pad={pad} {k} rel {e:.2e}")
        assert e < 1e-6, k
    sum((oa[k] * cots[k]).sum() for k in keys).backward()
    sum((ob[k] * cots[k]).sum() for k in keys).backward()
    W = 4 * N * Z + N
    # the composed path leaves .grad None where nothing flows (only d_w given): zeros
    ga = {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in a.items() if k in ("ml", "P", "pi")}
    pairs = {"dml": (b["ml"].grad, ga["ml"]), "dP": (b["P"].grad[..., :W], ga["P"][..., :W]),
             "dP heads": (b["P"].grad[..., :4 * N * Z], ga["P"][..., :4 * N * Z]),
             "dpi": (b["pi"].grad, ga["pi"])}
    for k, (got, want) in pairs.items():
        if float(want.abs().max()) == 0.0:  # only d_w given: nothing reaches ml, the heads or pi
            assert float(got.abs().max()) == 0.0, k
            continue
        e = rel_err(got, want)
        print(f"Z={Z} N={N} pad={pad} keys={len(keys)} {k} rel {e:.2e}")
        assert e < 1e-5, k
    if pad:
        assert float(b["P"].grad[..., W:].abs().max()) == 0.0


@pytest.mark.parametrize("Z", [5, 32, 70])
@pytest.mark.parametrize("N", [1, 3, 5])
def test_fused_matches_composed(Z, N):
    need_gpu()
    compare(3, 33, Z, N)


def test_fused_matches_composed_padded_heads():
    need_gpu()
    compare(3, 33, 32, 3, pad=7)


def test_fused_matches_composed_one_row():
    need_gpu()
    compare(1, 1, 32, 3)
    compare(1, 1, 5, 3)


# --------------------------------------------------------------------------- 3. NULL cotangents
@pytest.mark.parametrize("keys", [("sampled_h", "loss"), ("gmm_weight",)])
def test_missing_cotangents(keys):
    need_gpu()
    compare(3, 33, 32, 3, keys=keys)
    compare(3, 33, 5, 5, keys=keys)


def test_gmm_collapsed_backward_matches_composed():
    """The GMM-only mode as test_gmm_vae uses it: d_h and d_kl only."""
    need_gpu()
    from mlvae_hip import ops
    for Z, N in ((32, 3), (5, 5), (70, 1)):
        d, cots = make_inputs(3, 33, Z, N)
        a, b = leaves(d), leaves(d)
        z, kl, w = ops.GmmLatentFn.apply(a["P"], d["eps_g"], d["expo"], N, Z, TAU, 0)
        ha, ka = ops.apply_weight(z, w), ops.apply_weight(kl, w)
        hb, kb, wb = ops.gmm_collapsed(b["P"], d["eps_g"], d["expo"], N, Z, TAU, 0)
        assert torch.equal(wb, w)
        assert rel_err(hb, ha) < 1e-6 and rel_err(kb, ka) < 1e-6
        ((ha * cots["sampled_h"]).sum() + (ka * cots["loss"]).sum()).backward()
        ((hb * cots["sampled_h"]).sum() + (kb * cots["loss"]).sum()).backward()
        e = rel_err(b["P"].grad, a["P"].grad)
        eh = rel_err(b["P"].grad[..., :4 * N * Z], a["P"].grad[..., :4 * N * Z])
        print(f"gmm-only Z={Z} N={N} dP rel {e:.2e} heads {eh:.2e}")
        assert e < 1e-5 and eh < 1e-5


def test_backward_rerun_is_bit_identical():
    """Fixed-order reductions, no floating-point atomics: two runs give the same bits."""
    need_gpu()
    grads = []
    for _ in range(2):
        d, cots = make_inputs(3, 33, 70, 5)
        b = leaves(d)
        ob = fused(b, 5, 70)
        sum((ob[k] * cots[k]).sum() for k in cots).backward()
        grads.append([b[k].grad.clone() for k in ("ml", "P", "pi")])
    assert all(torch.equal(x, y) for x, y in zip(*grads))


# --------------------------------------------------------------------------- 4. library draws
def test_library_draws_are_the_composed_path_s():
    need_gpu()
    from modules.h_vae import HierarchicalVAE
    torch.manual_seed(7)
    a = HierarchicalVAE([12, 16, 16], 32, 3).cuda()
    b = HierarchicalVAE([12, 16, 16], 32, 3, fused=True).cuda()
    b.load_state_dict(a.state_dict())
    x = torch.randn(3, 33, 12).cuda()
    pi = torch.softmax(torch.randn(3, 33, 2), -1).cuda()
    torch.manual_seed(99)
    oa = a(x, pi)
    after_a = torch.randint(0, 2 ** 62, (1,)).item()
    torch.manual_seed(99)
    ob = b(x, pi)
    after_b = torch.randint(0, 2 ** 62, (1,)).item()
    assert after_a == after_b  # torch's RNG was read the same number of times
    assert torch.equal(ob["gmm_weight"], oa["gmm_weight"])
    assert oa["gmm_weight"].argmax(-1).unique().numel() > 1
    e = rel_err(ob["sampled_h"], oa["sampled_h"])
    print(f"library draws: sampled_h rel {e:.2e}")
    assert e < 1e-6
    assert rel_err(ob["losses"]["vae_kld_loss"], oa["losses"]["vae_kld_loss"]) < 1e-6


# --------------------------------------------------------------------------- 5. shards
BG, TS, KF = 3, 5, 2
SHARDS = [(0, 2), (2, 3)]
SEED = 0x1234567 * 977 + 5


def umap(off, seg, stride, total):
    return (ctypes.c_longlong * 4)(off, seg, stride, total)


def fold_slice(whole, lo, hi):
    sh = whole.shape
    return whole.reshape(KF, BG, *sh[1:])[:, lo:hi].reshape(KF * (hi - lo), *sh[1:]).contiguous()


def _fwd(d, N, Z, m, rows):
    """(w, ysoft, h) of one forward call with library draws; rows: the _rows entry with map m."""
    from mlvae_hip import _lib
    B, T = d["P"].shape[:2]
    new = lambda n: torch.full((B, T, n), float("nan"), device="cuda")
    mean, lv, h, kl, w, ys = new(Z), new(Z), new(Z), new(Z), new(N), new(N)
    l = _lib.lib()
    common = (P(d["ml"]), 2 * Z, P(d["P"]), d["P"].shape[-1], P(d["pi"]), P(d["eps_v"]), P(d["eps_g"]), None, SEED)
    outs = (TAU, P(mean), P(lv), P(h), P(kl), P(w), P(ys), stream())
    if rows:
        rc = l.mlvae_hvae_latent_fwd_rows(B, T, N, Z, *common, m, *outs)
    else:
        rc = l.mlvae_hvae_latent_fwd(B * T, N, Z, *common, 0, *outs)
    assert rc == 0, _lib.last_error()
    return w, ys, h


def _cut(d, fn):
    return {k: fn(v) for k, v in d.items()}


@pytest.mark.parametrize("Z,N", [(32, 3), (5, 5)])
def test_rows_entry_reproduces_the_whole_batch(Z, N):
    need_gpu()
    from mlvae_hip import _lib
    d, _ = make_inputs(BG, TS, Z, N)
    dk, _ = make_inputs(KF * BG, TS, Z, N, seed=1)
    whole, wholek = _fwd(d, N, Z, None, rows=False), _fwd(dk, N, Z, None, rows=False)
    assert wholek[0].argmax(-1).unique().numel() > 1
    # the draws are mlvae_gmm_latent_fwd's for the same seed
    z, kl = torch.empty(BG, TS, N * Z, device="cuda"), torch.empty(BG, TS, N * Z, device="cuda")
    w, ys = torch.empty(BG, TS, N, device="cuda"), torch.empty(BG, TS, N, device="cuda")
    assert _lib.lib().mlvae_gmm_latent_fwd(BG * TS, N, Z, P(d["P"]), d["P"].shape[-1], P(d["eps_g"]), None,
                                           SEED, 0, TAU, P(z), P(kl), P(w), P(ys), stream()) == 0
    assert torch.equal(whole[0], w) and torch.equal(whole[1], ys)
    for got in (_fwd(d, N, Z, None, rows=True), _fwd(d, N, Z, umap(0, BG, BG, BG), rows=True)):
        assert all(torch.equal(x, y) for x, y in zip(got, whole))
    for lo, hi in SHARDS:
        got = _fwd(_cut(d, lambda v: v[lo:hi].contiguous()), N, Z, umap(lo, hi - lo, hi - lo, BG), rows=True)
        assert all(torch.equal(x, y[lo:hi]) for x, y in zip(got, whole)), (lo, hi)
        got = _fwd(_cut(dk, lambda v: fold_slice(v, lo, hi)), N, Z, umap(lo, hi - lo, BG, KF * BG), rows=True)
        assert all(torch.equal(x, fold_slice(y, lo, hi)) for x, y in zip(got, wholek)), (lo, hi)
    assert not torch.equal(whole[0][0:1], whole[0][2:3])  # an unmapped shard would repeat utterance 0


def test_ops_take_the_rows_entry_under_a_shard():
    need_gpu()
    from mlvae_hip import ops
    Z, N = 32, 3
    d, _ = make_inputs(BG, TS, Z, N)
    d["expo"] = None
    whole = fused(d, N, Z, seed=SEED)
    for lo, hi in SHARDS:
        part = _cut(d, lambda v: None if v is None else v[lo:hi].contiguous())
        with ops.shard(lo, BG):
            got = fused(part, N, Z, seed=SEED)
            gw = ops.gmm_collapsed(part["P"], part["eps_g"], None, N, Z, TAU, SEED)[2]
        assert torch.equal(got["gmm_weight"], whole["gmm_weight"][lo:hi]), (lo, hi)
        assert torch.equal(got["sampled_h"], whole["sampled_h"][lo:hi]), (lo, hi)
        assert torch.equal(gw, whole["gmm_weight"][lo:hi]), (lo, hi)


# --------------------------------------------------------------------------- 6. bad shapes
def test_bad_shapes_are_refused():
    need_gpu()
    from mlvae_hip import _lib
    l = _lib.lib()
    Z, N = 4, 3
    d, _ = make_inputs(1, 2, Z, N)
    ld = 4 * N * Z + N
    o = torch.zeros(2, 64, device="cuda")

    def fwd(N_=N, ldp=ld, ldml=2 * Z, ml=P(d["ml"]), pi=P(d["pi"])):
        return l.mlvae_hvae_latent_fwd(2, N_, Z, ml, ldml, P(d["P"]), ldp, pi, P(d["eps_v"]), P(d["eps_g"]),
                                       P(d["expo"]), 0, 0, TAU, P(o), P(o), P(o), P(o), P(o), P(o), stream())

    def bwd(N_=N, ldp=ld, ldml=2 * Z, ml=P(d["ml"]), pi=P(d["pi"]), lddp=ld):
        return l.mlvae_hvae_latent_bwd(2, N_, Z, ml, ldml, P(d["P"]), ldp, pi, P(d["eps_v"]), P(d["eps_g"]),
                                       P(o), P(o), TAU, None, None, None, None, None, P(o), P(o), lddp,
                                       None, stream())

    for call in (fwd, bwd):
        assert call(N_=0) != 0 and call(N_=65) != 0
        assert call(ldp=ld - 1) != 0
        assert call(ldml=2 * Z - 1) != 0
        assert call(ml=None) != 0 and "go together" in _lib.last_error()
        assert call(pi=None) != 0
    assert bwd(lddp=ld - 1) != 0
    assert l.mlvae_hvae_latent_fwd_rows(1, 2, 0, Z, None, 0, None, ld, None, None, None, None, 0, None, TAU,
                                        None, None, None, None, None, None, stream()) != 0
    assert l.mlvae_hvae_latent_fwd_rows(1, 2, N, Z, None, 0, P(d["P"]), ld, None, None, P(d["eps_g"]), None, 0,
                                        umap(0, 0, 1, 1), TAU, None, None, P(o), P(o), P(o), P(o), stream()) != 0
    assert "map" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((o == 0).all())  # nothing was launched
    assert fwd() == 0  # the same call with good shapes runs
    torch.cuda.synchronize()
