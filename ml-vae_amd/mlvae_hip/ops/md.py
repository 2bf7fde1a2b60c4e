"""The MD recipes' heads and losses: the upstream losses, the pi path, MD_VAE_sfl's score-function
terms and LSTM_FC's frame-level head (csrc/md.hip, csrc/pi.hip, csrc/flvl.hip)."""
import torch

from .._lib import check, lib
from ._core import _bt, current_shard, _md_err, _need, _p, raise_err, _rows, _stream, _workspace, _ws_bytes


# --------------------------------------------------------------------------- MD-VAE upstream losses
def _raise_md(err):
    """The recogniser-target bits of the word `err` (one host sync): the reference's AssertionError."""
    raise_err(err, "md")


class PhnBceFn(torch.autograd.Function):
    """PhonemeRecognizer.compute_losses on libmlvae (ref:src/modules/phoneme_recognizer.py:35-81):
    [B,T,C] BCE-with-logits against the boundary-expanded canonical phoneme sequence."""

    @staticmethod
    def forward(ctx, out, feat_lens, phn, phn_lens, boundary):
        out = _need(out, "recogniser output")
        B, T, C = out.shape
        fl = _need(feat_lens.to(out.device, torch.float32), "feat_lens")
        pl = _need(phn_lens.to(out.device, torch.float32), "phn_lens")
        bnd = _need(boundary.to(out.device, torch.float32), "boundary_seqs")
        ids = phn.to(out.device, torch.int64).contiguous()
        loss = torch.empty_like(out)
        err = _md_err()
        check(lib().mlvae_phn_bce(B, T, C, _p(out), C, _p(fl), ids.data_ptr(), ids.shape[1], _p(pl),
                                  _p(bnd), _p(loss), None, None, _p(err), _stream()), "phn_bce")
        _raise_md(err)  # the reference asserts on the host too (one sync per batch, not per utterance)
        ctx.save_for_backward(out, fl, ids, pl, bnd)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        out, fl, ids, pl, bnd = ctx.saved_tensors
        B, T, C = out.shape
        dloss = _need(dloss, "grad")
        dout = torch.empty_like(out)
        err = _md_err()
        check(lib().mlvae_phn_bce(B, T, C, _p(out), C, _p(fl), ids.data_ptr(), ids.shape[1], _p(pl),
                                  _p(bnd), None, _p(dloss), _p(dout), _p(err), _stream()), "phn_bce_bwd")
        return dout, None, None, None, None


def phn_bce(out, feat_lens, phn, phn_lens, boundary):
    return PhnBceFn.apply(out, feat_lens, phn, phn_lens, boundary)


class BoundaryHeadsFn(torch.autograd.Function):
    """BoundaryDetector after its FC heads (ref:src/modules/boundary_detector.py:42-97): Softplus
    + 1e-5, Beta(1, 9) KL, ten Kumaraswamy draws; returns (boundary_v, bce, kld).  u = the ten
    U(0,1) draws [10, B, T] (None: Philox keyed by seed and element index)."""

    @staticmethod
    def forward(ctx, za, zb, y, u, seed):
        za, zb = _need(za, "alpha head"), _need(zb, "beta head")
        y = _need(y.to(za.device, torch.float32), "boundary_seqs")
        u = _need(u, "uniforms") if u is not None else None
        v, bce, kld = torch.empty_like(za), torch.empty_like(za), torch.empty_like(za)
        sh = current_shard() if u is None else None  # injected draws are the shard's own
        if sh is not None:
            B, T, _ = _bt(za.shape, "boundary_heads")
            check(lib().mlvae_boundary_fwd_rows(B, T, _p(za), _p(zb), _p(y), None, seed, sh.map(B),
                                                _p(v), _p(bce), _p(kld), _stream()), "boundary_fwd_rows")
        else:
            check(lib().mlvae_boundary_fwd(za.numel(), _p(za), _p(zb), _p(y), _p(u) if u is not None else None,
                                           seed, 0, _p(v), _p(bce), _p(kld), _stream()), "boundary_fwd")
        ctx.save_for_backward(za, zb, y, *([u] if u is not None else []))
        ctx.seed, ctx.has_u, ctx.shard = seed, u is not None, sh
        return v, bce, kld

    @staticmethod
    def backward(ctx, dv, dbce, dkld):
        t = ctx.saved_tensors
        za, zb, y = t[:3]
        u = t[3] if ctx.has_u else None
        grads = [None if g is None else _need(g, "grad") for g in (dv, dbce, dkld)]
        dza, dzb = torch.empty_like(za), torch.empty_like(zb)
        gp = [(_p(g) if g is not None else None) for g in grads]
        if ctx.shard is not None:
            B, T, _ = _bt(za.shape, "boundary_heads")
            check(lib().mlvae_boundary_bwd_rows(B, T, _p(za), _p(zb), _p(y), None, ctx.seed,
                                                ctx.shard.map(B), *gp, _p(dza), _p(dzb), _stream()),
                  "boundary_bwd_rows")
            return dza, dzb, None, None, None
        check(lib().mlvae_boundary_bwd(za.numel(), _p(za), _p(zb), _p(y), _p(u) if u is not None else None,
                                       ctx.seed, 0, *gp, _p(dza), _p(dzb), _stream()), "boundary_bwd")
        return dza, dzb, None, None, None


def boundary_heads(za, zb, boundary, u=None):
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if u is None else 0
    return BoundaryHeadsFn.apply(za, zb, boundary, u, seed)


# --------------------------------------------------------------------------- MD-VAE pi path
def raise_pi_err():
    """Read the device error word's pi bit (one host sync): ValueError as
    Categorical.log_prob raises for a label outside its support."""
    raise_err(_md_err(), "pi")


class PiSampleFn(torch.autograd.Function):
    """sampled_pi of the MD-VAE forward (ref:src/models/MD_VAE/model.py:122-127): the one-hot
    [1 - label, label] of a Categorical(logits) draw (train) or the argmax (eval).  u = the
    U(0,1) draw per frame (None: Philox keyed by seed and frame index)."""

    @staticmethod
    def forward(ctx, logits, train, u, seed):
        logits = _need(logits, "pi_logits")
        if logits.shape[-1] != 2:
            raise ValueError(f"pi_sample: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        n = _rows(logits)
        if u is not None:
            u = _need(u, "uniforms")
            if u.numel() != n:
                raise ValueError(f"pi_sample: {u.numel()} uniforms for {n} frames")
        out = torch.empty_like(logits)
        sh = current_shard() if (train and u is None) else None
        if sh is not None:
            B, T, _ = _bt(logits.shape, "pi_sample")
            check(lib().mlvae_pi_sample_rows(B, T, 1, _p(logits), None, seed, sh.map(B), 1, _p(out),
                                             _stream()), "pi_sample_rows")
            ctx.mark_non_differentiable(out)
            return out
        check(lib().mlvae_pi_sample(n, _p(logits), _p(u) if u is not None else None, seed, 0,
                                    1 if train else 0, _p(out), _stream()), "pi_sample")
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        return None, None, None, None


def pi_sample(logits, train, u=None):
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (train and u is None) else 0
    return PiSampleFn.apply(logits, bool(train), u, seed)


class PiNllFn(torch.autograd.Function):
    """pi_nll_loss = -Categorical(logits).log_prob(labels) (ref:src/models/MD_VAE/model.py:145-149)
    on the decode kernel's int32 frame labels [.., T] (-1 past T_i counts as 0)."""

    @staticmethod
    def forward(ctx, logits, labels):
        logits = _need(logits, "pi_logits")
        if logits.shape[-1] != 2:
            raise ValueError(f"pi_nll: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        if not (labels.is_cuda and labels.dtype == torch.int32):
            raise TypeError(f"pi_nll labels: expected an int32 HIP tensor, got {labels.dtype} on "
                            f"{labels.device}")
        labels = labels.contiguous()
        n = _rows(logits)
        if labels.numel() != n:
            raise ValueError(f"pi_nll: {labels.numel()} labels for {n} frames")
        nll = torch.empty(logits.shape[:-1], device=logits.device, dtype=torch.float32)
        check(lib().mlvae_pi_nll_fwd(n, _p(logits), labels.data_ptr(), _p(nll), _p(_md_err()),
                                     _stream()), "pi_nll_fwd")
        ctx.save_for_backward(logits, labels)
        ctx.mark_non_differentiable(labels)
        return nll

    @staticmethod
    def backward(ctx, dnll):
        logits, labels = ctx.saved_tensors
        dnll = _need(dnll, "pi_nll grad")
        dlogits = torch.empty_like(logits)
        check(lib().mlvae_pi_nll_bwd(_rows(logits), _p(logits), labels.data_ptr(), _p(dnll),
                                     _p(dlogits), _stream()), "pi_nll_bwd")
        return dlogits, None


def pi_nll(logits, labels, sync=True):
    """sync=False leaves the error word unread (no host sync): the caller reads it with
    raise_pi_err() where it syncs anyway (the MD-VAE recipe: at the stage's end)."""
    nll = PiNllFn.apply(logits, labels)
    if sync:
        raise_pi_err()
    return nll


# --------------------------------------------------------------------------- MD_VAE_sfl
class PiSampleKFn(torch.autograd.Function):
    """K Categorical(logits) draws per frame (ref:src/models/MD_VAE_sfl/model.py:147-152) as
    one-hot rows [K, .., 2]; draw k of frame i uses uniform k n + i of u [K, ..] or of the
    Philox stream.  Eval (train false) is the argmax: K must be 1."""

    @staticmethod
    def forward(ctx, logits, K, train, u, seed):
        if K < 1 or (not train and K != 1):
            raise ValueError(f"pi_sample_k: K must be >= 1 in train and 1 in eval (the argmax), got {K}")
        if logits.shape[-1] != 2:
            raise ValueError(f"pi_sample_k: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        logits = _need(logits, "pi_logits")
        n = _rows(logits)
        if u is not None:
            u = _need(u, "uniforms")
            if u.numel() != K * n:
                raise ValueError(f"pi_sample_k: {u.numel()} uniforms for {K} draws of {n} frames")
        out = torch.empty((K,) + tuple(logits.shape), device=logits.device, dtype=torch.float32)
        sh = current_shard() if (train and u is None) else None
        if sh is not None:
            B, T, _ = _bt(logits.shape, "pi_sample_k")
            check(lib().mlvae_pi_sample_rows(B, T, K, _p(logits), None, seed, sh.map(B), 1, _p(out),
                                             _stream()), "pi_sample_rows")
            ctx.mark_non_differentiable(out)
            return out
        check(lib().mlvae_pi_sample_k(n, K, _p(logits), _p(u) if u is not None else None, seed, 0,
                                      1 if train else 0, _p(out), _stream()), "pi_sample_k")
        ctx.mark_non_differentiable(out)
        return out

    @staticmethod
    def backward(ctx, dout):
        return None, None, None, None, None


def pi_sample_k(logits, K, train, u=None):
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if (train and u is None) else 0
    return PiSampleKFn.apply(logits, int(K), bool(train), u, seed)


class SflLossesFn(torch.autograd.Function):
    """The score-function terms of MD_VAE_sfl (ref:src/models/MD_VAE_sfl/model.py:170-186), the K
    draws summed and divided by K: rif = (reward - baseline) * nll of the draw, the negative
    entropy of Categorical(logits), and the baseline's squared error against the reward
    -(w_recon mean(recon) + w_kld mean(kld) + w_nll pi_nll).  Gradients go to logits and baseline
    only: the reference detaches the reward, and the baseline inside rif."""

    @staticmethod
    def forward(ctx, logits, sampled_pi, recon, kld, pi_nll, baseline, w_recon, w_kld, w_nll):
        if logits.shape[-1] != 2:
            raise ValueError(f"sfl_losses: pi_logits must end in 2 classes, got {tuple(logits.shape)}")
        frames = tuple(logits.shape[:-1])
        if sampled_pi.dim() != logits.dim() + 1 or tuple(sampled_pi.shape[1:]) != tuple(logits.shape):
            raise ValueError(f"sfl_losses: sampled_pi must be [K, {', '.join(map(str, logits.shape))}], "
                             f"got {tuple(sampled_pi.shape)}")
        K = sampled_pi.shape[0]
        if K < 1:
            raise ValueError("sfl_losses: no draws (K = 0)")
        for name, t in (("recon_loss", recon), ("vae_kld_loss", kld)):
            if tuple(t.shape[:-1]) != (K,) + frames or t.shape[-1] < 1:
                raise ValueError(f"sfl_losses: {name} must be [K, .., C] over {(K,) + frames}, "
                                 f"got {tuple(t.shape)}")
        for name, t in (("pi_nll_loss", pi_nll), ("baseline", baseline)):
            if tuple(t.shape) != frames:
                raise ValueError(f"sfl_losses: {name} must be {frames}, got {tuple(t.shape)}")
        logits, sampled_pi = _need(logits, "pi_logits"), _need(sampled_pi, "sampled_pi")
        recon, kld = _need(recon, "recon_loss"), _need(kld, "vae_kld_loss")
        pi_nll, baseline = _need(pi_nll, "pi_nll_loss"), _need(baseline, "baseline")
        n = _rows(logits)
        reward = torch.empty((K,) + frames, device=logits.device, dtype=torch.float32)
        rif, ent, bl = (torch.empty(frames, device=logits.device, dtype=torch.float32) for _ in range(3))
        check(lib().mlvae_sfl_fwd(n, K, recon.shape[-1], kld.shape[-1], _p(logits), _p(sampled_pi),
                                  _p(recon), _p(kld), _p(pi_nll), _p(baseline), float(w_recon),
                                  float(w_kld), float(w_nll), _p(reward), _p(rif), _p(ent), _p(bl),
                                  _stream()), "sfl_fwd")
        ctx.save_for_backward(logits, sampled_pi, reward, baseline)
        return rif, ent, bl

    @staticmethod
    def backward(ctx, d_rif, d_ent, d_bl):
        logits, sampled_pi, reward, baseline = ctx.saved_tensors
        d_rif, d_ent, d_bl = (_need(g, "sfl_losses grad") for g in (d_rif, d_ent, d_bl))
        dlogits, dbaseline = torch.empty_like(logits), torch.empty_like(baseline)
        check(lib().mlvae_sfl_bwd(_rows(logits), sampled_pi.shape[0], _p(logits), _p(sampled_pi),
                                  _p(reward), _p(baseline), _p(d_rif), _p(d_ent), _p(d_bl),
                                  _p(dlogits), _p(dbaseline), _stream()), "sfl_bwd")
        return dlogits, None, None, None, None, dbaseline, None, None, None


def sfl_losses(logits, sampled_pi, recon, kld, pi_nll, baseline, w_recon, w_kld, w_nll):
    """(rif, neg_entropy, baseline_loss), each shaped like logits[..., 0]."""
    return SflLossesFn.apply(logits, sampled_pi, recon, kld, pi_nll, baseline, w_recon, w_kld, w_nll)


# --------------------------------------------------------------------------- LSTM_FC frame-level head
def raise_flvl_err():
    """Read the device error word's frame-label bit (one host sync): ValueError as
    MDMetricStats raises for a non-binary label sequence."""
    raise_err(_md_err(), "flvl")


class FlvlMdHeadFn(torch.autograd.Function):
    """The LSTM_FC recipe after the FCBlock's last hidden layer (ref:src/models/LSTM_FC/
    model.py:30-61): logits = h W^T + b, the class-weighted BCE-with-logits per frame and class
    against [1 - label, label], the argmax (-1 past each length) and the per-utterance MD counts
    (both correct, both mispronounced, missed, false alarm), one kernel; the backward is one
    kernel and the fixed-order sum of its partials."""

    @staticmethod
    def forward(ctx, h, weight, bias, labels, lens, pw0, pw1):
        if h.dim() != 3:
            raise ValueError(f"flvl_md_head: h must be [B, T, E], got {tuple(h.shape)}")
        B, T, E = h.shape
        if E < 1:
            raise ValueError("flvl_md_head: h has no features (E = 0)")
        if tuple(weight.shape) != (2, E) or tuple(bias.shape) != (2,):
            raise ValueError(f"flvl_md_head: weight must be [2, {E}] and bias [2], got "
                             f"{tuple(weight.shape)} and {tuple(bias.shape)}")
        if tuple(labels.shape) != (B, T):
            raise ValueError(f"flvl_md_head: labels must be [{B}, {T}], got {tuple(labels.shape)}")
        if tuple(lens.shape) != (B,):
            raise ValueError(f"flvl_md_head: lens must be [{B}], got {tuple(lens.shape)}")
        if labels.device != h.device:
            raise TypeError(f"flvl_md_head labels: on {labels.device}, h on {h.device}")
        h, weight, bias = _need(h, "flvl_md_head h"), _need(weight, "flvl_md_head weight"), \
            _need(bias, "flvl_md_head bias")
        labels = _need(labels.to(torch.float32), "flvl_md_head labels")
        lens = _need(lens.to(h.device, torch.float32), "flvl_md_head lens")
        logits = torch.empty(B, T, 2, device=h.device, dtype=torch.float32)
        loss_e = torch.empty_like(logits)
        pred = torch.empty(B, T, device=h.device, dtype=torch.int32)
        counts = torch.empty(B, 4, device=h.device, dtype=torch.int32)
        check(lib().mlvae_flvl_head_fwd(B, T, E, _p(h), _p(weight), _p(bias), _p(labels), _p(lens),
                                        pw0, pw1, _p(logits), _p(loss_e), pred.data_ptr(),
                                        counts.data_ptr(), _p(_md_err()), _stream()), "flvl_head_fwd")
        ctx.save_for_backward(h, weight, logits, labels)
        ctx.pw = (pw0, pw1)
        ctx.mark_non_differentiable(logits, pred, counts)
        return logits, loss_e, pred, counts

    @staticmethod
    def backward(ctx, dlogits, dloss_e, dpred, dcounts):
        h, weight, logits, labels = ctx.saved_tensors
        B, T, E = h.shape
        dloss_e = _need(dloss_e, "flvl_md_head grad")
        dh, dw = torch.empty_like(h), torch.empty_like(weight)
        db = torch.empty(2, device=h.device, dtype=torch.float32)
        if B * T == 0:
            return dh, dw.zero_(), db.zero_(), None, None, None, None
        l = lib()
        ws = _workspace(l.mlvae_flvl_head_workspace_size(B, T, E), "flvl")
        check(l.mlvae_flvl_head_bwd(B, T, E, _p(h), _p(weight), _p(logits), _p(labels), _p(dloss_e),
                                    ctx.pw[0], ctx.pw[1], _p(dh), _p(dw), _p(db), _p(ws),
                                    _ws_bytes(ws), _stream()), "flvl_head_bwd")
        return dh, dw, db, None, None, None, None


def flvl_md_head(h, weight, bias, labels, lens, pos_weight):
    """(logits [B,T,2], loss_e [B,T,2], pred int32 [B,T], counts int32 [B,4]) from h [B,T,E], the
    final Linear's weight [2,E] and bias [2], the frame labels [B,T] (0 / 1) and the relative
    lengths [B]; pos_weight = (class 0, class 1).  Gradients reach h, weight and bias through
    loss_e only.  A label outside {0, 1} in a valid frame sets a bit of the device error word:
    raise_flvl_err() reads it (where the counts are read, not per batch)."""
    pw0, pw1 = (float(v) for v in pos_weight)
    return FlvlMdHeadFn.apply(h, weight, bias, labels, lens, pw0, pw1)
