"""csrc/elbo.hip kernel by kernel through the C ABI, against the fp64 references of
tests/elbo_optim_ref.py: reparameterisation + KL and its backward, the reconstruction kernel's
three modes and two loss types, the fp64 finalize, the frame count, the masked means past the
golden shapes and lrelu_bwd -- at one element, at odd sizes, and just past the 1024 x 256 grid
cap where the grid-stride loop takes its second pass.  Tolerances: elbo_optim_ref.TOL (4x the
fp32 noise of the same formula on a CPU); counters, sentinels, masked zeros and lrelu_bwd exact."""
import functools

import numpy as np
import pytest
import torch

import elbo_optim_ref as R
from gpu_utils import P, need_gpu, rel_err, stream
from mlvae_hip._lib import last_error, lib

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def dev(t):
    return t.contiguous().cuda()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def ok(rc):
    assert rc == 0, last_error()
    torch.cuda.synchronize()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def scalar_rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------- reparam + KL
@functools.lru_cache(maxsize=None)
def reparam_case(B, T, Z):
    d = R.reparam_inputs(B, T, Z)
    z, kl, ksum = R.reparam_kl(d["ml"], d["eps"], d["lens"], T)
    return d, z, kl, float(ksum)


@pytest.mark.parametrize("want_kl,want_parts", [(1, 1), (0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("B,T,Z", R.REPARAM_SHAPES)
def test_reparam_kl_fwd(B, T, Z, want_kl, want_parts):
    need_gpu()
    l = lib()
    d, zref, klref, ksum = reparam_case(B, T, Z)
    N = B * T
    ml, eps, lens = dev(d["ml"].reshape(N, 2 * Z)), dev(d["eps"]), dev(d["lens"])
    npart = l.mlvae_elbo_partials_count(B, T, Z)
    assert npart == min((N * Z + 255) // 256, 1024)
    z, kl, parts = nans(B, T, Z), nans(B, T, Z), nans(npart)

    def launch(ml_):
        ok(l.mlvae_reparam_kl_fwd(B, T, Z, P(ml_), 2 * Z, P(eps), P(lens), P(z), P(kl) if want_kl else None,
                                  P(parts) if want_parts else None, stream()))
    launch(ml)
    ez = rel_err(z, zref)
    print(f"z {ez:.3e} (TOL {R.TOL['z']:.3e})")
    assert ez <= R.TOL["z"]
    if want_kl:
        ek = rel_err(kl, klref)
        print(f"kl {ek:.3e} (TOL {R.TOL['kl']:.3e})")
        assert ek <= R.TOL["kl"]
    else:
        assert torch.isnan(kl).all()
    if not want_parts:
        assert torch.isnan(parts).all()
        return
    assert not torch.isnan(parts).any()          # every block wrote its partial
    es = scalar_rel(parts.double().sum(), ksum)
    print(f"kl_sum {es:.3e} (TOL {R.TOL['kl_sum']:.3e})")
    assert es <= R.TOL["kl_sum"]
    if B > 1:   # the zero-length utterance's rows never reach the sum: change them, same bits
        first = parts.clone()
        ml2 = ml.clone().view(B, T, 2 * Z)
        ml2[1] += 3.0
        launch(ml2)
        assert torch.equal(bits(parts), bits(first))


@pytest.mark.parametrize("mode", ["dkl", "mask", "count", "nodz"])
@pytest.mark.parametrize("B,T,Z", R.REPARAM_SHAPES)
def test_reparam_kl_bwd(B, T, Z, mode):
    need_gpu()
    d = reparam_case(B, T, Z)[0]
    N, ld = B * T, 2 * Z + 4
    kw = dict(dz=None if mode == "nodz" else d["dz"])
    if mode == "dkl":
        kw["dkl"] = d["dkl"]
    else:
        kw.update(kl_scale=d["kl_scale"], count=2 * B * T if mode == "count" else None)
    ref = R.reparam_kl_bwd(d["ml"], d["eps"], d["lens"], T, **kw)
    ml, eps, lens = dev(d["ml"].reshape(N, 2 * Z)), dev(d["eps"]), dev(d["lens"])
    dz = dev(d["dz"]) if kw["dz"] is not None else None
    dkl = dev(d["dkl"]) if mode == "dkl" else None
    cnt = i32(2 * B * T) if mode == "count" else None
    dml = torch.full((N, ld), SENTINEL, device="cuda")
    ok(lib().mlvae_reparam_kl_bwd(B, T, Z, P(ml), 2 * Z, P(eps), P(lens), P(cnt) if cnt is not None else None,
                                  P(dz) if dz is not None else None, P(dkl) if dkl is not None else None,
                                  float(kw.get("kl_scale", 0.0)), P(dml), ld, stream()))
    assert (dml[:, 2 * Z:] == SENTINEL).all()     # the padding columns of lddml = 2Z + 4
    got = dml[:, :2 * Z].reshape(B, T, 2 * Z)
    e = rel_err(got, ref)
    print(f"dml[{mode}] {e:.3e} (TOL {R.TOL['dml']:.3e})")
    assert e <= R.TOL["dml"]
    if mode == "nodz" and B > 1:                  # s = 0 on the zero-length utterance and past each length
        m = R.frame_mask(d["lens"], T)
        assert (got.cpu()[~m] == 0).all() and (got.cpu()[1] == 0).all()
        assert (got.cpu()[m][:, :Z] != 0).all()


# ------------------------------------------------------------------------------- reconstruction
@functools.lru_cache(maxsize=None)
def recon_case(B, T, F, loss_type, mode):
    d = R.recon_inputs(B, T, F)
    w = {"fwd": None, "drec": d["drec"],
         "fused": R.mask_weight(d["lens"], T, d["rec_scale"], F),
         "fused_count": R.mask_weight(d["lens"], T, d["rec_scale"], F, count=2 * B * T)}[mode]
    rec, rsum, dmu, dlv = R.recon(d["mu"], d["lv"], d["x"], d["lens"], T, loss_type, weight=w)
    return d, rec, float(rsum), dmu, dlv


@pytest.mark.parametrize("mode", ["fwd", "fused", "fused_count", "drec"])
@pytest.mark.parametrize("loss_type", [0, 1])
@pytest.mark.parametrize("B,T,F", R.RECON_SHAPES)
def test_recon(B, T, F, loss_type, mode):
    need_gpu()
    l = lib()
    d, rec_ref, rsum, dmu_ref, dlv_ref = recon_case(B, T, F, loss_type, mode)
    N, ldx = B * T, F + 3
    buf = dev(torch.cat([d["mu"], d["lv"]], -1).reshape(N, 2 * F))   # mu | lv halves of one buffer
    x = torch.full((N, ldx), 1e6, device="cuda")
    x[:, :F] = dev(d["x"].reshape(N, F))
    lens = dev(d["lens"])
    nll = loss_type == 0
    npart = l.mlvae_elbo_partials_count(B, T, F)
    rec, parts = nans(B, T, F), nans(npart)
    dbuf = torch.full((N, 2 * F), SENTINEL, device="cuda")
    drec = dev(d["drec"]) if mode == "drec" else None
    cnt = i32(2 * B * T) if mode == "fused_count" else None
    grads = mode != "fwd"
    want_rec = mode in ("fwd", "drec")              # the fused training call keeps only the partials
    ok(l.mlvae_recon(B, T, F, loss_type, P(buf), 2 * F, P(buf, F) if nll else None, 2 * F, P(x), ldx,
                     P(lens), P(cnt) if cnt is not None else None, P(rec) if want_rec else None, P(parts),
                     P(drec) if drec is not None else None, float(d["rec_scale"]),
                     P(dbuf) if grads else None, P(dbuf, F) if grads and nll else None, stream()))
    if want_rec:
        e = rel_err(rec, rec_ref)
        print(f"rec {e:.3e} (TOL {R.TOL['rec']:.3e})")
        assert e <= R.TOL["rec"]
    else:
        assert torch.isnan(rec).all()
    assert not torch.isnan(parts).any()
    es = scalar_rel(parts.double().sum(), rsum)
    print(f"rec_sum {es:.3e} (TOL {R.TOL['rec_sum']:.3e})")
    assert es <= R.TOL["rec_sum"]
    if not grads:
        assert (dbuf == SENTINEL).all()
        return
    dmu = dbuf[:, :F].reshape(B, T, F)
    e = rel_err(dmu, dmu_ref)
    print(f"dmu {e:.3e} (TOL {R.TOL['dmu']:.3e})")
    assert e <= R.TOL["dmu"]
    if nll:
        dlv = dbuf[:, F:].reshape(B, T, F)
        e = rel_err(dlv, dlv_ref)
        print(f"dlv {e:.3e} (TOL {R.TOL['dlv']:.3e})")
        assert e <= R.TOL["dlv"]
    else:
        assert (dbuf[:, F:] == SENTINEL).all()     # MSE has no log-variance gradient to write
    if mode.startswith("fused") and B > 1:          # masked frames get exactly zero
        m = R.frame_mask(d["lens"], T)
        assert (dmu.cpu()[~m] == 0).all() and (dmu.cpu()[1] == 0).all()


def test_recon_rejects_an_unknown_loss_type():
    need_gpu()
    B, T, F = R.RECON_SHAPES[1]
    d = R.recon_inputs(B, T, F)
    mu, lv, x, lens = dev(d["mu"]), dev(d["lv"]), dev(d["x"]), dev(d["lens"])
    rec = nans(B, T, F)
    rc = lib().mlvae_recon(B, T, F, 2, P(mu), F, P(lv), F, P(x), F, P(lens), None, P(rec), None, None, 0.0,
                           None, None, stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert "Invalid loss type: 2" in last_error()
    assert torch.isnan(rec).all()


# ------------------------------------------------------------------------------- finalize
@pytest.mark.parametrize("given_count", [0, 1])
@pytest.mark.parametrize("nk,nr", R.FINALIZE_CASES)
def test_elbo_finalize(nk, nr, given_count):
    need_gpu()
    d = R.finalize_inputs(nk, nr)
    B, T, Z, F = d["B"], d["T"], d["Z"], d["F"]
    own = int(R.valid_frames(d["lens"], T).sum())
    count = 3 * own + 1 if given_count else own
    kld, rec, _ = R.finalize(d["pk"].double().sum(), d["pr"].double().sum(), count, Z, F, d["w_kl"], d["w_rec"])
    pk, pr, lens = dev(d["pk"]), dev(d["pr"]), dev(d["lens"])
    cnt = i32(count) if given_count else None
    out = nans(3)
    ok(lib().mlvae_elbo_finalize(P(pk), nk, P(pr), nr, P(lens), P(cnt) if given_count else None, B, T, Z, F,
                                 d["w_kl"], d["w_rec"], P(out), stream()))
    o = out.cpu().numpy()
    e0, e1 = scalar_rel(o[0], kld), scalar_rel(o[1], rec)
    print(f"finalize {e0:.3e} {e1:.3e} (TOL {R.TOL['finalize']:.3e})")
    assert e0 <= R.TOL["finalize"] and e1 <= R.TOL["finalize"]
    # total = 0 + w_kl * kld, then + w_rec * rec, each product and sum rounded to fp32
    tot = np.float32(0) + np.float32(d["w_kl"]) * o[0]
    tot = tot + np.float32(d["w_rec"]) * o[1]
    assert tot.dtype == np.float32
    assert o[2].tobytes() == tot.tobytes(), (o[2], tot)


@pytest.mark.parametrize("B,T", R.COUNT_CASES)
def test_count_frames(B, T):
    need_gpu()
    lens = R.count_lens(B, T)
    out, dlens = i32(-7), dev(lens)
    ok(lib().mlvae_count_frames(P(dlens), B, T, P(out), stream()))
    assert out.item() == int(R.valid_frames(lens, T).sum())


# ------------------------------------------------------------------------------- masked means
@pytest.mark.parametrize("red", [0, 1, 2])
@pytest.mark.parametrize("B,T,C", R.MASKED_MEAN_SHAPES)
def test_masked_mean_fwd_bwd(B, T, C, red):
    need_gpu()
    d = R.masked_mean_inputs(B, T, C)
    name = R.REDUCTIONS[red]
    ref = R.masked_mean(d["loss"], d["lens"], name).reshape(-1)
    loss, lens = dev(d["loss"]), dev(d["lens"])
    out = nans(2 * B)
    ok(lib().mlvae_masked_mean(B, T, C, P(loss), P(lens), red, P(out), stream()))
    got = out[:ref.numel()]
    e = rel_err(got, ref)
    print(f"masked_mean[{name}] {e:.3e} (TOL {R.TOL['masked_mean']:.3e})")
    assert e <= R.TOL["masked_mean"]
    g = d["gB"] if red == 2 else d["g1"]
    gref = R.masked_mean_bwd(g, (B, T, C), d["lens"], name)
    dloss, dg = nans(B, T, C), dev(g)
    ok(lib().mlvae_masked_mean_bwd(B, T, C, P(lens), red, P(dg), P(dloss), stream()))
    e = rel_err(dloss, gref)
    print(f"masked_mean_bwd[{name}] {e:.3e} (TOL {R.TOL['masked_mean_bwd']:.3e})")
    assert e <= R.TOL["masked_mean_bwd"]
    m = R.frame_mask(d["lens"], T)
    assert (dloss.cpu()[~m] == 0).all() and (dloss.cpu()[m] != 0).all()


# ------------------------------------------------------------------------------- lrelu_bwd
@pytest.mark.parametrize("n", R.LRELU_SIZES)
def test_lrelu_bwd_bit_equal(n):
    need_gpu()
    d = R.lrelu_inputs(n)
    ref = R.lrelu_bwd(d["dy"], d["y"], dtype=torch.float32)   # a select and one fp32 multiply
    dx, dy, y = nans(n), dev(d["dy"]), dev(d["y"])
    ok(lib().mlvae_lrelu_bwd(n, P(dy), P(y), P(dx), stream()))
    assert torch.equal(bits(dx), bits(ref))
