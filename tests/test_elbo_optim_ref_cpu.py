"""The references of tests/elbo_optim_ref.py, proved without a GPU: each one against torch
autograd, torch.optim.Adam, clip_grad_norm_ or the oracle, and the tolerance table against the
float32 noise it is derived from."""
import numpy as np
import pytest
import torch

import elbo_optim_ref as R
from oracle import vae_cpu as O

F64 = torch.float64


def _rel(a, b):
    """gpu_utils.rel_err: max-abs error over max-abs reference."""
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------- lengths
@pytest.mark.parametrize("lens,T,want", [
    ([127 / 500], 500, [128]),                  # fp32(127/500) * 500 > 127: one more frame
    ([0.0, -0.5], 17, [0, 0]),
    ([1.0, 1.3, float("inf")], 17, [17, 17, 17]),
    ([float("nan")], 17, [0]),
    ([0.5 / 17, 254 / 500], 17, [1, 9]),
])
def test_valid_frames_quirks_agree_with_ops(lens, T, want):
    from mlvae_hip import ops
    vf = R.valid_frames(lens, T)
    assert vf.tolist() == want
    assert R.frame_mask(lens, T).sum(1).tolist() == want
    assert ops.valid_frames(torch.tensor(lens), T) == sum(want)
    m = O.length_to_mask(torch.tensor(lens), T)
    assert torch.equal(m.bool(), R.frame_mask(lens, T))


def test_quirk_len_really_is_one():
    for T in (343, 500):
        r = R.quirk_len(T)
        k = round(r * T)
        assert R.valid_frames([r], T)[0] == k + 1


@pytest.mark.parametrize("B,T", R.COUNT_CASES)
def test_count_lens_agree_with_ops(B, T):
    from mlvae_hip import ops
    lens = R.count_lens(B, T)
    assert int(R.valid_frames(lens, T).sum()) == ops.valid_frames(lens, T)


# ------------------------------------------------------------------------------- autograd ties
@pytest.mark.parametrize("B,T,Z", R.REPARAM_SHAPES[:2])
@pytest.mark.parametrize("mode", ["dkl", "mask", "count", "nodz"])
def test_reparam_kl_bwd_is_autograd_of_fwd(B, T, Z, mode):
    d = R.reparam_inputs(B, T, Z)
    ml = d["ml"].double().requires_grad_(True)
    z, kl = R.reparam_kl_terms(ml[..., :Z], ml[..., Z:], d["eps"].double())
    kw = dict(dz=None if mode == "nodz" else d["dz"])
    if mode == "dkl":
        kw["dkl"] = d["dkl"]
        s = d["dkl"].double()
    else:
        kw["kl_scale"] = d["kl_scale"]
        kw["count"] = 29 if mode == "count" else None
        cnt = 29 if mode == "count" else int(R.valid_frames(d["lens"], T).sum())
        s = R.frame_mask(d["lens"], T).double().unsqueeze(-1) * d["kl_scale"] / (cnt * Z)
    obj = (s * kl).sum() + (0 if mode == "nodz" else (d["dz"].double() * z).sum())
    (want,) = torch.autograd.grad(obj, ml)
    got = R.reparam_kl_bwd(d["ml"], d["eps"], d["lens"], T, **kw)
    torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-15)
    # forward: the masked sum leaves the zero-length utterance out
    _, kl2, ksum = R.reparam_kl(d["ml"], d["eps"], d["lens"], T)
    vf = R.valid_frames(d["lens"], T)
    want_sum = sum(kl2[b, :vf[b]].sum() for b in range(B))
    assert abs(ksum - want_sum) <= 1e-12 * abs(want_sum)


@pytest.mark.parametrize("loss_type", [0, 1])
def test_recon_matches_the_closed_form_gradient_and_torch(loss_type):
    B, T, F = R.RECON_SHAPES[1]
    d = R.recon_inputs(B, T, F)
    rec, rsum, dmu, dlv = R.recon(d["mu"], d["lv"], d["x"], d["lens"], T, loss_type)
    mu, lv, x = d["mu"].double(), d["lv"].double(), d["x"].double()
    if loss_type == 0:
        # the Gaussian negative log-likelihood with variance exp(lv) + 1e-5, log-term on lv
        ev = lv.exp() + 1e-5
        want = 0.5 * (R.LOG_2PI + lv + (x - mu) ** 2 / ev)
        torch.testing.assert_close(dmu, -(x - mu) / ev, rtol=1e-12, atol=0)
        torch.testing.assert_close(dlv, 0.5 * (1 - (x - mu) ** 2 * lv.exp() / ev ** 2), rtol=1e-10, atol=1e-12)
    else:
        want = torch.nn.functional.mse_loss(x, mu, reduction="none")
        torch.testing.assert_close(dmu, -2 * (x - mu), rtol=1e-14, atol=0)
        assert dlv.abs().max() == 0
    torch.testing.assert_close(rec, want, rtol=1e-14, atol=0)
    lm = O.apply_lens_to_loss(rec, d["lens"], "mean")
    cnt = int(R.valid_frames(d["lens"], T).sum())
    assert abs(rsum / (cnt * F) - lm) <= 1e-13 * abs(lm)
    # weighted: the gradient of the masked mean the fused mode produces
    w = R.mask_weight(d["lens"], T, d["rec_scale"], F)
    _, _, dmu_w, _ = R.recon(d["mu"], d["lv"], d["x"], d["lens"], T, loss_type, weight=w)
    mu_g = mu.clone().requires_grad_(True)
    obj = d["rec_scale"] * O.apply_lens_to_loss(R.recon_terms(mu_g, lv, x, loss_type), d["lens"], "mean")
    (want_g,) = torch.autograd.grad(obj, mu_g)
    torch.testing.assert_close(dmu_w, want_g, rtol=1e-12, atol=1e-18)


@pytest.mark.parametrize("B,T,C", R.MASKED_MEAN_SHAPES[:2])
@pytest.mark.parametrize("reduction", R.REDUCTIONS)
def test_masked_mean_is_the_oracles_and_its_bwd_is_autograd(B, T, C, reduction):
    d = R.masked_mean_inputs(B, T, C)
    loss = d["loss"].double().requires_grad_(True)
    want = O.apply_lens_to_loss(loss, d["lens"], reduction)
    got = R.masked_mean(d["loss"], d["lens"], reduction)
    torch.testing.assert_close(got, want.detach(), rtol=1e-14, atol=0)
    g = d["gB"] if reduction == "batch" else d["g1"]
    (want_g,) = torch.autograd.grad((want * g.double().reshape(want.shape)).sum(), loss)
    got_g = R.masked_mean_bwd(g, (B, T, C), d["lens"], reduction)
    torch.testing.assert_close(got_g, want_g, rtol=1e-13, atol=0)
    vf = R.valid_frames(d["lens"], T)
    assert vf[0] == T and vf[1] == 1 and vf.min() >= 1


def test_finalize_is_the_weighted_masked_means():
    B, T, Z, F = 3, 17, 5, 13
    dk, dr = R.reparam_inputs(B, T, Z), R.recon_inputs(B, T, F)
    _, kl, ksum = R.reparam_kl(dk["ml"], dk["eps"], dk["lens"], T)
    rec, rsum, _, _ = R.recon(dr["mu"], dr["lv"], dr["x"], dr["lens"], T, 0)
    cnt = int(R.valid_frames(dk["lens"], T).sum())
    kld, rc, tot = R.finalize(ksum, rsum, cnt, Z, F, 1e-3, 1.0)
    a = O.apply_lens_to_loss(kl, dk["lens"], "mean").item()
    b = O.apply_lens_to_loss(rec, dr["lens"], "mean").item()
    assert abs(kld - a) <= 1e-13 * abs(a) and abs(rc - b) <= 1e-13 * abs(b)
    assert abs(tot - (1e-3 * a + b)) <= 1e-13 * abs(tot)


def test_lrelu_bwd_is_leaky_relus_autograd_at_both_zeros():
    d = R.lrelu_inputs(255)
    x = d["y"].double().requires_grad_(True)   # LeakyReLU keeps the sign: y <= 0 iff x <= 0
    (want,) = torch.autograd.grad((torch.nn.functional.leaky_relu(x, R.NEG_SLOPE) * d["dy"].double()).sum(), x)
    assert torch.equal(R.lrelu_bwd(d["dy"], d["y"]), want)
    z = torch.tensor([0.0, -0.0, 1e-40, -1e-40])
    assert R.lrelu_bwd(torch.ones(4), z).tolist() == [0.01, 0.01, 1.0, 0.01]
    assert (d["y"] == 0).sum() >= 2 and ((d["y"] != 0) & (d["y"].abs() < 1e-38)).any()


# ------------------------------------------------------------------------------- optimizer ties
def test_adam_step_is_torch_optim_adam_over_ten_steps():
    n = 185
    d = R.adam_inputs(n)
    h = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
    p = torch.nn.Parameter(d["p"].double().clone())
    opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"])
    q, m, v = d["p"].double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for t in range(1, 11):
        g = R.grad_inputs(n, scale=t)
        p.grad = g.double()
        opt.step()
        q, m, v = R.adam_step(q, m, v, g, t, **h)
        torch.testing.assert_close(q, p.detach(), rtol=1e-13, atol=1e-15)
    st = opt.state[p]
    torch.testing.assert_close(m, st["exp_avg"], rtol=1e-13, atol=1e-18)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-13, atol=1e-18)


@pytest.mark.parametrize("max_norm", [0.5, 1e4, float("inf")])
def test_clip_coef_and_sumsq_are_clip_grad_norm(max_norm):
    gs = [R.grad_inputs(n) for n in R.CLIP_SIZES]
    ps = [torch.nn.Parameter(torch.zeros(g.numel(), dtype=F64)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.double().clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    mine = float(sum(R.sumsq(g) for g in gs)) ** 0.5
    assert abs(mine - total.item()) <= 1e-13 * mine
    coef = R.clip_coef(mine, max_norm)
    assert (coef == 1.0) == (max_norm > 1)
    for p, g in zip(ps, gs):
        torch.testing.assert_close(g.double() * coef, p.grad, rtol=1e-13, atol=0)


def test_clip_coef_nan_total_poisons_like_torch():
    p = torch.nn.Parameter(torch.zeros(4, dtype=F64))
    p.grad = torch.tensor([1.0, float("nan"), 2.0, 3.0], dtype=F64)
    total = torch.nn.utils.clip_grad_norm_([p], 5.0)
    assert torch.isnan(total) and torch.isnan(p.grad).all()
    assert np.isnan(R.clip_coef(float("nan"), 5.0))


def test_colsum_beta():
    d = R.colsum_inputs(15, 3, 3)
    x = d["x"].double()
    assert torch.equal(R.colsum(d["x"]), x.sum(0))
    torch.testing.assert_close(R.colsum(d["x"], 1.0, d["out0"]), d["out0"].double() + x.sum(0))


# ------------------------------------------------------------------------------- the fp32 noise
def fp32_errors():
    """Worst max-abs-over-max-abs error, per quantity, of the float32 evaluation of each reference
    against its float64 evaluation, over every input the GPU tests use."""
    f32 = torch.float32
    err = {}

    def note(key, a, b):
        err[key] = max(err.get(key, 0.0), _rel(a, b))

    for B, T, Z in R.REPARAM_SHAPES:
        d = R.reparam_inputs(B, T, Z)
        a, b = R.reparam_kl(d["ml"], d["eps"], d["lens"], T, dtype=f32), R.reparam_kl(d["ml"], d["eps"], d["lens"], T)
        for key, x, y in zip(("z", "kl", "kl_sum"), a, b):
            note(key, x, y)
        for kw in (dict(dz=d["dz"], dkl=d["dkl"]), dict(dz=d["dz"], kl_scale=d["kl_scale"]),
                   dict(dz=None, kl_scale=d["kl_scale"]), dict(dz=d["dz"], kl_scale=d["kl_scale"], count=2 * B * T)):
            note("dml", R.reparam_kl_bwd(d["ml"], d["eps"], d["lens"], T, dtype=f32, **kw),
                 R.reparam_kl_bwd(d["ml"], d["eps"], d["lens"], T, **kw))
    for B, T, F in R.RECON_SHAPES:
        d = R.recon_inputs(B, T, F)
        for lt in (0, 1):
            for w in (None, d["drec"], R.mask_weight(d["lens"], T, d["rec_scale"], F),
                      R.mask_weight(d["lens"], T, d["rec_scale"], F, count=2 * B * T)):
                a = R.recon(d["mu"], d["lv"], d["x"], d["lens"], T, lt, weight=w, dtype=f32)
                b = R.recon(d["mu"], d["lv"], d["x"], d["lens"], T, lt, weight=w)
                for key, x, y in zip(("rec", "rec_sum", "dmu", "dlv"), a, b):
                    if not (key == "dlv" and lt == 1):
                        note(key, x, y)
    for nk, nr in R.FINALIZE_CASES:
        d = R.finalize_inputs(nk, nr)
        own = int(R.valid_frames(d["lens"], d["T"]).sum())
        for cnt in (own, 3 * own + 1):
            want = R.finalize(d["pk"].double().sum(), d["pr"].double().sum(), cnt, d["Z"], d["F"], d["w_kl"], d["w_rec"])
            c32 = torch.tensor(float(cnt), dtype=f32)
            note("finalize", d["pk"].sum() / (c32 * d["Z"]), want[0])
            note("finalize", d["pr"].sum() / (c32 * d["F"]), want[1])
    for B, T, C in R.MASKED_MEAN_SHAPES:
        d = R.masked_mean_inputs(B, T, C)
        for red in R.REDUCTIONS:
            note("masked_mean", R.masked_mean(d["loss"], d["lens"], red, dtype=f32), R.masked_mean(d["loss"], d["lens"], red))
            g = d["gB"] if red == "batch" else d["g1"]
            note("masked_mean_bwd", R.masked_mean_bwd(g, (B, T, C), d["lens"], red, dtype=f32),
                 R.masked_mean_bwd(g, (B, T, C), d["lens"], red))
    gs = [R.grad_inputs(n) for n in R.CLIP_SIZES]
    total = float(sum(R.sumsq(g) for g in gs)) ** 0.5
    tot32 = float(sum(R.sumsq(g, dtype=f32) for g in gs).sqrt())
    for g in gs:
        note("clip_g", g * R.clip_coef(tot32, R.CLIP_MAX_NORM, dtype=f32), g.double() * R.clip_coef(total, R.CLIP_MAX_NORM))
    h = R.ADAM_HYPER
    for n in R.ADAM_SIZES:
        d = R.adam_inputs(n)
        norm, norm32 = float(R.sumsq(d["g"])) ** 0.5, float(R.sumsq(d["g"], dtype=f32).sqrt())
        for t0 in R.ADAM_STEPS0:
            for max_norm in (R.ADAM_MAX_NORM, float("inf")):
                a = R.adam_step(d["p"], d["m"], d["v"], d["g"], t0 + 1, dtype=f32,
                                coef=R.clip_coef(norm32, max_norm, dtype=f32), **h)
                b = R.adam_step(d["p"], d["m"], d["v"], d["g"], t0 + 1, coef=R.clip_coef(norm, max_norm), **h)
                for key, x, y in zip(("adam_p", "adam_m", "adam_v"), a, b):
                    note(key, x, y)
    a, b = R.adam_trajectory(f32), R.adam_trajectory(F64)
    for key, x, y in zip(("adam_p", "adam_m", "adam_v"), a, b):
        note(key, x, y)
    for N, C, ld in R.COLSUM_SHAPES:
        d = R.colsum_inputs(N, C, ld)
        x = d["x"][:, :C]
        note("colsum", R.colsum(x, dtype=f32), R.colsum(x))
        note("colsum", R.colsum(x, 1.0, d["out0"], dtype=f32), R.colsum(x, 1.0, d["out0"]))
        xb = x.to(torch.bfloat16)
        note("colsum", R.colsum(xb, dtype=f32), R.colsum(xb))
    return err


def test_fp32_noise_is_within_a_quarter_of_tol():
    nt = torch.get_num_threads()
    torch.set_num_threads(1)   # a full fp32 sum's order does not depend on the machine's cores
    try:
        err = fp32_errors()
    finally:
        torch.set_num_threads(nt)
    for k in sorted(err):
        print(f"    {k!r}: {err[k]:.3e},   # TOL {R.TOL.get(k, float('nan')):.3e}")
    assert set(err) == set(R.MEASURED) == set(R.TOL)
    for k, e in err.items():
        assert R.TOL[k] == 4.0 * R.MEASURED[k]
        assert e <= R.TOL[k] / 4, (k, e, R.TOL[k])
        # ... and the table has not drifted up from its justification either
        assert e >= 0.5 * R.MEASURED[k], (k, e, R.MEASURED[k])
