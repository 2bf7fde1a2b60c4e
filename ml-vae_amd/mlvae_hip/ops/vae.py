"""The VAE losses and latents: reparameterisation + KL, reconstruction, masked means, and the
GMM-VAE / H-VAE latent blocks (csrc/elbo.hip, csrc/gmm.hip, csrc/hvae.hip)."""
import torch

from .._lib import check, lib
from ._core import _bt, current_shard, _need, _p, _rows, _stream, _ws


# --------------------------------------------------------------------------- ELBO part 1
class ReparamKLFn(torch.autograd.Function):
    """z = eps*exp(lv/2) + mu and per-element KL (ref:src/modules/vanilla_vae.py:37-45);
    ml = [mu | log_var] along the last dim."""

    @staticmethod
    def forward(ctx, ml, eps):
        ml, eps = _need(ml, "ml"), _need(eps, "eps")
        Z = ml.shape[-1] // 2
        N = _rows(ml)
        z = torch.empty(*ml.shape[:-1], Z, device=ml.device, dtype=torch.float32)
        kl = torch.empty_like(z)
        # rows are independent: pass them as B=N utterances of T=1 frame (mask all-valid)
        ones = _ones(N)
        check(lib().mlvae_reparam_kl_fwd(N, 1, Z, _p(ml), 2 * Z, _p(eps), _p(ones), _p(z), _p(kl),
                                         None, _stream()), "reparam_kl_fwd")
        ctx.save_for_backward(ml, eps)
        return z, kl

    @staticmethod
    def backward(ctx, dz, dkl):
        ml, eps = ctx.saved_tensors
        Z = ml.shape[-1] // 2
        N = _rows(ml)
        dz = _need(dz, "dz") if dz is not None else torch.zeros(*ml.shape[:-1], Z, device=ml.device)
        dkl = _need(dkl, "dkl") if dkl is not None else torch.zeros_like(dz)
        dml = torch.empty_like(ml)
        check(lib().mlvae_reparam_kl_bwd(N, 1, Z, _p(ml), 2 * Z, _p(eps), _p(_ones(N)), None,
                                         _p(dz), _p(dkl), 0.0, _p(dml), 2 * Z, _stream()),
              "reparam_kl_bwd")
        return dml, None


def _ones(n):
    dev = torch.cuda.current_device()
    o = _ws.get((dev, "ones"))
    if o is None or o.numel() < n:
        o = torch.ones(max(n, 1024), device="cuda", dtype=torch.float32)
        _ws[(dev, "ones")] = o
    return o


def randn(shape, generator=None):
    """N(0,1) from the library's Philox stream; the seed is drawn from torch's (CPU) RNG so
    torch.manual_seed (ref:src/config/run.yaml:2-3) makes it reproducible."""
    seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())
    out = torch.empty(*shape, device="cuda", dtype=torch.float32)
    sh = current_shard()
    if sh is not None:
        B, T, C = _bt(out.shape, "randn")
        check(lib().mlvae_randn_rows(B, T, C, seed, sh.map(B), _p(out), _stream()), "randn_rows")
        return out
    check(lib().mlvae_randn(out.numel(), seed, 0, _p(out), _stream()), "randn")
    return out


# --------------------------------------------------------------------------- ELBO part 2
LOSS = {"likelihood": 0, "mse": 1}


class ReconFn(torch.autograd.Function):
    """Per-element reconstruction loss (ref:src/modules/decoder.py:37-53)."""

    @staticmethod
    def forward(ctx, mux, lvx, x, loss_type):
        mux, x = _need(mux, "mean"), _need(x, "target")
        lt = LOSS[loss_type]
        lvx = _need(lvx, "log_var") if lt == 0 else mux
        F = mux.shape[-1]
        N = _rows(mux)
        rec = torch.empty_like(mux)
        check(lib().mlvae_recon(N, 1, F, lt, _p(mux), F, _p(lvx), F, _p(x), F, _p(_ones(N)), None,
                                _p(rec), None, None, 0.0, None, None, _stream()), "recon")
        ctx.save_for_backward(mux, lvx, x)
        ctx.lt = lt
        return rec

    @staticmethod
    def backward(ctx, drec):
        mux, lvx, x = ctx.saved_tensors
        drec = _need(drec, "recon grad")
        F, N = mux.shape[-1], _rows(mux)
        dmux = torch.empty_like(mux)
        dlvx = torch.empty_like(mux) if ctx.lt == 0 else None
        check(lib().mlvae_recon(N, 1, F, ctx.lt, _p(mux), F, _p(lvx), F, _p(x), F, _p(_ones(N)),
                                None, None, None, _p(drec), 0.0, _p(dmux),
                                _p(dlvx) if dlvx is not None else None, _stream()), "recon_bwd")
        return dmux, dlvx, None, None


def recon_loss(mean, log_var, target, loss_type):
    if loss_type not in LOSS:
        raise ValueError(f"Invalid loss type: {loss_type}")  # ref:src/modules/decoder.py:50-51
    return ReconFn.apply(mean, log_var if loss_type == "likelihood" else mean, target, loss_type)


# --------------------------------------------------------------------------- masked mean
RED = {"mean": 0, "batchmean": 1, "batch": 2}


class MaskedMeanFn(torch.autograd.Function):
    """apply_lens_to_loss (ref:src/utils/data_utils.py:67-104)."""

    @staticmethod
    def forward(ctx, loss, lens, reduction):
        loss = _need(loss, "loss")
        lens = _need(lens.to(loss.device, torch.float32), "lens")
        B, T = loss.shape[0], loss.shape[1]
        C = loss.numel() // (B * T) if B * T else 1
        out = torch.empty(2 * B if B else 2, device=loss.device, dtype=torch.float32)
        check(lib().mlvae_masked_mean(B, T, C, _p(loss), _p(lens), RED[reduction], _p(out),
                                      _stream()), "masked_mean")
        ctx.save_for_backward(lens)
        ctx.shape, ctx.red = loss.shape, RED[reduction]
        return out[:B].clone() if reduction == "batch" else out[0].clone()

    @staticmethod
    def backward(ctx, g):
        (lens,) = ctx.saved_tensors
        B, T = ctx.shape[0], ctx.shape[1]
        C = 1
        for d in ctx.shape[2:]:
            C *= d
        g = _need(g.reshape(-1), "grad")
        dloss = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        check(lib().mlvae_masked_mean_bwd(B, T, C, _p(lens), ctx.red, _p(g), _p(dloss), _stream()),
              "masked_mean_bwd")
        return dloss, None, None


def masked_mean(loss, lens, reduction="mean", global_frames=None):
    """global_frames: the valid frames of the global batch this batch is a shard of (default
    inside an ops.shard context that carries global_lens: its count).  The "mean" is then this
    shard's share of the global mean -- local masked sum / (global_frames * C), so the shares
    of all shards add up to the single-process mean -- and a shard of fillers alone gives 0."""
    if reduction not in RED:
        raise ValueError(f"unknown reduction {reduction}")
    sh = current_shard()
    if global_frames is None and sh is not None and reduction == "mean" and loss.dim() >= 2:
        global_frames = sh.global_frames(loss.shape[1])
    if global_frames is None:
        return MaskedMeanFn.apply(loss, lens, reduction)
    if reduction != "mean":
        raise ValueError("masked_mean: a global denominator belongs to reduction 'mean'")
    B, T = loss.shape[0], loss.shape[1]
    C = loss.numel() // (B * T) if B * T else 1
    if global_frames < 1:
        raise ValueError("masked_mean: the global batch has no valid frame")
    # batchmean = masked sum / B (no local count in it): rescaled to sum / (global frames * C)
    return MaskedMeanFn.apply(loss, lens, "batchmean") * (float(B) / (float(global_frames) * C))


# --------------------------------------------------------------------------- GMM-VAE / H-VAE
class GmmLatentFn(torch.autograd.Function):
    """GMM-VAE latent block on the stacked head output P = [pm | plv | m | lv | logits]
    (ref:src/modules/gmm_vae.py:24-67): returns z, per-element KL and the straight-through
    hard Gumbel-softmax weights.  expo = the Exp(1) draws [.., N] (None: library Philox)."""

    @staticmethod
    def forward(ctx, P, eps, expo, N, Z, tau, seed):
        P, eps = _need(P, "gmm heads"), _need(eps, "eps")
        expo = _need(expo, "expo") if expo is not None else None
        rows = _rows(P)
        z = torch.empty(*P.shape[:-1], N * Z, device=P.device, dtype=torch.float32)
        kl = torch.empty_like(z)
        w = torch.empty(*P.shape[:-1], N, device=P.device, dtype=torch.float32)
        ysoft = torch.empty_like(w)
        sh = current_shard() if expo is None else None
        if sh is not None:
            B, T, _ = _bt(P.shape, "gmm_latent")
            check(lib().mlvae_gmm_latent_fwd_rows(B, T, N, Z, _p(P), P.shape[-1], _p(eps), None, seed,
                                                  sh.map(B), tau, _p(z), _p(kl), _p(w), _p(ysoft),
                                                  _stream()), "gmm_latent_fwd_rows")
            ctx.save_for_backward(P, eps, ysoft)
            ctx.shape = (N, Z, tau)
            return z, kl, w
        check(lib().mlvae_gmm_latent_fwd(rows, N, Z, _p(P), P.shape[-1], _p(eps),
                                         _p(expo) if expo is not None else None, seed, 0, tau,
                                         _p(z), _p(kl), _p(w), _p(ysoft), _stream()),
              "gmm_latent_fwd")
        ctx.save_for_backward(P, eps, ysoft)
        ctx.shape = (N, Z, tau)
        return z, kl, w

    @staticmethod
    def backward(ctx, dz, dkl, dw):
        P, eps, ysoft = ctx.saved_tensors
        N, Z, tau = ctx.shape
        opt = lambda t, n: _need(t, n) if t is not None else None
        dz, dkl, dw = opt(dz, "dz"), opt(dkl, "dkl"), opt(dw, "dw")
        dP = torch.empty_like(P)
        nz = lambda t: _p(t) if t is not None else None
        check(lib().mlvae_gmm_latent_bwd(_rows(P), N, Z, _p(P), P.shape[-1], _p(eps), _p(ysoft),
                                         tau, nz(dz), nz(dkl), nz(dw), _p(dP), P.shape[-1],
                                         _stream()), "gmm_latent_bwd")
        return dP, None, None, None, None, None, None


class ApplyWeightFn(torch.autograd.Function):
    """y[.., c] = sum_n w[.., n] x[.., n*C + c] (ref:src/utils/data_utils.py:32-64)."""

    @staticmethod
    def forward(ctx, x, w):
        x, w = _need(x, "apply_weight x"), _need(w, "apply_weight weight")
        N = w.shape[-1]
        C = x.shape[-1] // N
        rows = _rows(w)
        if x.numel() != rows * N * C:
            raise ValueError(f"apply_weight: x {tuple(x.shape)} does not match weight {tuple(w.shape)}")
        y = torch.empty(*w.shape[:-1], C, device=x.device, dtype=torch.float32)
        check(lib().mlvae_apply_weight_fwd(rows, N, C, _p(x), N * C, _p(w), _p(y), C, _stream()),
              "apply_weight_fwd")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _need(dy, "apply_weight grad")
        N = w.shape[-1]
        C = x.shape[-1] // N
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        check(lib().mlvae_apply_weight_bwd(_rows(w), N, C, _p(x), N * C, _p(w), _p(dy), C,
                                           _p(dx) if dx is not None else None, N * C,
                                           _p(dw) if dw is not None else None, _stream()),
              "apply_weight_bwd")
        return dx, dw


def apply_weight(x, weight):
    """(B,T,N*C) or (B,T,N,C) weighted by (B,T,N) -> (B,T,C)."""
    B, T, N = weight.shape
    return ApplyWeightFn.apply(x.reshape(B, T, -1), weight)


class HvaeLatentFn(torch.autograd.Function):
    """The H-VAE's latent stretch in one launch (csrc/hvae.hip; ref:src/modules/h_vae.py:21-72):
    ml = [mean_v | log_var_v], P = the GMM's stacked heads, pi [.., 2] -> the mixed (mean, log_var,
    sampled_h, kl) [.., Z] and the hard Gumbel-softmax weights [.., N].  ml = pi = None is the
    GMM-only mode: (None, None, collapsed h, collapsed kl, weights).  expo = the Exp(1) draws
    [.., N] (None: library Philox under `seed`, mapped inside an ops.shard context)."""

    @staticmethod
    def forward(ctx, ml, P, pi, eps_v, eps_g, expo, N, Z, tau, seed):
        hier = ml is not None
        ctx.set_materialize_grads(False)  # an unused output's cotangent reaches the kernel as NULL
        P, eps_g = _need(P, "gmm heads"), _need(eps_g, "eps_g")
        expo = _need(expo, "expo") if expo is not None else None
        if hier:
            ml, pi, eps_v = _need(ml, "ml"), _need(pi, "pi"), _need(eps_v, "eps_v")
        rows = _rows(P)
        lead = P.shape[:-1]
        new = lambda n: torch.empty(*lead, n, device=P.device, dtype=torch.float32)
        h, kl, w, ysoft = new(Z), new(Z), new(N), new(N)
        mean, log_var = (new(Z), new(Z)) if hier else (None, None)
        nz = lambda t: _p(t) if t is not None else None
        ldml = ml.shape[-1] if hier else 0
        sh = current_shard() if expo is None else None
        if sh is not None:
            B, T, _ = _bt(P.shape, "hvae_latent")
            check(lib().mlvae_hvae_latent_fwd_rows(
                B, T, N, Z, nz(ml), ldml, _p(P), P.shape[-1], nz(pi), nz(eps_v), _p(eps_g), None, seed,
                sh.map(B), tau, nz(mean), nz(log_var), _p(h), _p(kl), _p(w), _p(ysoft), _stream()),
                "hvae_latent_fwd_rows")
        else:
            check(lib().mlvae_hvae_latent_fwd(
                rows, N, Z, nz(ml), ldml, _p(P), P.shape[-1], nz(pi), nz(eps_v), _p(eps_g), nz(expo),
                seed, 0, tau, nz(mean), nz(log_var), _p(h), _p(kl), _p(w), _p(ysoft), _stream()),
                "hvae_latent_fwd")
        ctx.hier = hier
        ctx.save_for_backward(*((ml, pi, eps_v) if hier else ()), P, eps_g, w, ysoft)
        ctx.shape = (N, Z, tau)
        return mean, log_var, h, kl, w

    @staticmethod
    def backward(ctx, d_mean, d_log_var, d_h, d_kl, d_w):
        if ctx.hier:
            ml, pi, eps_v, P, eps_g, w, ysoft = ctx.saved_tensors
        else:
            (P, eps_g, w, ysoft), ml, pi, eps_v = ctx.saved_tensors, None, None, None
        N, Z, tau = ctx.shape
        nz = lambda t: _p(t) if t is not None else None
        keep =[None if t is None else _need(t, "grad") for t in (d_mean, d_log_var, d_h, d_kl, d_w)]
        dP = torch.empty_like(P)
        if P.shape[-1] > 4 * N * Z + N:
            dP[..., 4 * N * Z + N:] = 0  # columns past the heads: never written by the kernel
        dml = torch.empty(*P.shape[:-1], 2 * Z, device=P.device, dtype=torch.float32) if ctx.hier else None
        dpi = torch.empty_like(pi) if ctx.hier and ctx.needs_input_grad[2] else None
        check(lib().mlvae_hvae_latent_bwd(
            _rows(P), N, Z, nz(ml), ml.shape[-1] if ctx.hier else 0, _p(P), P.shape[-1], nz(pi),
            nz(eps_v), _p(eps_g), _p(w), _p(ysoft), tau, *[nz(t) for t in keep], nz(dml), _p(dP),
            P.shape[-1], nz(dpi), _stream()), "hvae_latent_bwd")
        if ctx.hier and ml.shape[-1] != 2 * Z:
            wide = torch.zeros_like(ml)
            wide[..., :2 * Z] = dml
            dml = wide
        return dml, dP, dpi, None, None, None, None, None, None, None


def _latent_shapes(what, P, eps_g, expo, N, Z):
    if not (1 <= N <= 64) or Z < 1:
        raise ValueError(f"{what}: N must be in [1, 64] and Z >= 1, got N={N} Z={Z}")
    if P.shape[-1] < 4 * N * Z + N:
        raise ValueError(f"{what}: the stacked heads need {4 * N * Z + N} columns, got {tuple(P.shape)}")
    lead = tuple(P.shape[:-1])
    if tuple(eps_g.shape) != lead + (N * Z,):
        raise ValueError(f"{what}: eps_g {tuple(eps_g.shape)} is not {lead + (N * Z,)}")
    if expo is not None and tuple(expo.shape) != lead + (N,):
        raise ValueError(f"{what}: expo {tuple(expo.shape)} is not {lead + (N,)}")
    return lead


def hvae_latent(ml, P, pi, eps_v, eps_g, expo, N, Z, tau, seed):
    """(mean, log_var, sampled_h, kl) [.., Z] and gmm_weight [.., N] of the Hierarchical VAE from
    its two encoders' head outputs, one launch each way (HvaeLatentFn)."""
    lead = _latent_shapes("hvae_latent", P, eps_g, expo, N, Z)
    if ml is None or pi is None or eps_v is None:
        raise ValueError("hvae_latent: ml, pi and eps_v are required (gmm_collapsed is the GMM-only form)")
    if tuple(ml.shape[:-1]) != lead or ml.shape[-1] < 2 * Z:
        raise ValueError(f"hvae_latent: ml {tuple(ml.shape)} is not {lead} + (>= {2 * Z},)")
    if tuple(pi.shape) != lead + (2,):
        raise ValueError(f"hvae_latent: pi {tuple(pi.shape)} is not {lead + (2,)}")
    if tuple(eps_v.shape) != lead + (Z,):
        raise ValueError(f"hvae_latent: eps_v {tuple(eps_v.shape)} is not {lead + (Z,)}")
    return HvaeLatentFn.apply(ml, P, pi, eps_v, eps_g, expo, N, Z, tau, seed)


def gmm_collapsed(P, eps, expo, N, Z, tau, seed):
    """(weighted_h, weighted_loss) [.., Z] and gmm_weight [.., N] of the GMM-VAE: apply_weight of
    GmmLatentFn's sampled_h and loss with its own weights, in one launch each way."""
    _latent_shapes("gmm_collapsed", P, eps, expo, N, Z)
    return HvaeLatentFn.apply(None, P, None, None, eps, expo, N, Z, tau, seed)[2:]
