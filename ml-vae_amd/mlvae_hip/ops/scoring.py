"""Per-utterance scoring of the upstream modules on the device (csrc/score.hip)."""
import torch

from .._lib import check, lib
from ._core import _md_err, _need, _p, raise_err, _score_lens, _stream


# --------------------------------------------------------------------------- upstream-module scoring
def raise_score_err():
    """Read the device error word's scoring bits (one host sync) and clear them alone:
    AssertionError as plvl_phn_acc_scoring's asserts, RuntimeError as torch.topk's (the
    segments error first)."""
    raise_err(_md_err(), "score")


def _score_seq(x, shape, dev, dtype, what):
    if tuple(x.shape) != shape:
        raise ValueError(f"{what} must be {list(shape)}, got {tuple(x.shape)}")
    if x.device != dev:
        raise TypeError(f"{what}: on {x.device}, the scored output on {dev}")
    return x.to(dtype).contiguous()


def phn_acc_counts(out, feat_lens, flvl_targets, plvl_targets=None, phn_lens=None, boundary_seqs=None):
    """int32 [B, 4] = (flvl_correct, T_i, plvl_correct, L_i) per utterance of the recogniser
    output out [B, T, C]: what PhnAccMetricStats.append_counts takes.  flvl_targets [B, T] and
    plvl_targets [B, L] are phoneme ids, boundary_seqs [B, T] the 0/1 flags that open the phoneme
    segments; plvl_targets None gives (.., .., 0, 0).  Stays on the device; a bad flag count sets
    a bit of the device error word (raise_score_err)."""
    if out.dim() != 3 or out.shape[2] < 1:
        raise ValueError(f"phn_acc_counts: out must be [B, T, C] with C >= 1, got {tuple(out.shape)}")
    out = _need(out.detach(), "phn_acc_counts out")
    B, T, C = out.shape
    dev = out.device
    fl = _score_lens(feat_lens, B, dev, "phn_acc_counts feat")
    ft = _score_seq(flvl_targets, (B, T), dev, torch.int64, "phn_acc_counts flvl_targets")
    pt = pl = bnd = None
    L = 0
    if plvl_targets is not None:
        if boundary_seqs is None or phn_lens is None:
            raise ValueError("boundary_seqs must be provided when plvl_targets is not None")
        if plvl_targets.dim() != 2:
            raise ValueError(f"phn_acc_counts plvl_targets must be [B, L], got {tuple(plvl_targets.shape)}")
        L = plvl_targets.shape[1]
        pt = _score_seq(plvl_targets, (B, L), dev, torch.int64, "phn_acc_counts plvl_targets")
        pl = _score_lens(phn_lens, B, dev, "phn_acc_counts phoneme")
        bnd = _score_seq(boundary_seqs, (B, T), dev, torch.float32, "phn_acc_counts boundary_seqs")
    counts = torch.zeros(B, 4, device=dev, dtype=torch.int32)
    check(lib().mlvae_phn_acc(B, T, C, L, _p(out), C, _p(fl), ft.data_ptr(),
                              pt.data_ptr() if pt is not None else None,
                              _p(pl) if pl is not None else None,
                              _p(bnd) if bnd is not None else None, counts.data_ptr(),
                              _p(_md_err()), _stream()), "phn_acc")
    return counts


def boundary_topk(boundary_v, feat_lens, fa_boundary_seqs):
    """pred int32 [B, T]: 1 at the k_i largest of boundary_v[i, :T_i] (0 elsewhere, -1 past T_i),
    k_i = the ones of fa_boundary_seqs[i] -- the reference's per-utterance torch.topk, for the
    whole batch on the device.  k_i > T_i sets a bit of the device error word (raise_score_err)."""
    if boundary_v.dim() != 2:
        raise ValueError(f"boundary_topk: boundary_v must be [B, T], got {tuple(boundary_v.shape)}")
    v = _need(boundary_v.detach(), "boundary_topk boundary_v")
    B, T = v.shape
    limit = lib().mlvae_boundary_topk_max_frames()
    if T > limit:
        raise ValueError(f"boundary_topk: {T} frames, the kernel ranks a row of at most {limit}")
    fl = _score_lens(feat_lens, B, v.device, "boundary_topk feat")
    fa = _score_seq(fa_boundary_seqs, (B, T), v.device, torch.float32, "boundary_topk fa_boundary_seqs")
    pred = torch.empty(B, T, device=v.device, dtype=torch.int32)
    k = torch.empty(B, device=v.device, dtype=torch.int32)
    check(lib().mlvae_boundary_topk(B, T, _p(v), _p(fl), _p(fa), pred.data_ptr(), k.data_ptr(),
                                    _p(_md_err()), _stream()), "boundary_topk")
    return pred


def boundary_counts(pred, targets, feat_lens):
    """int32 [B, 3] = (correct, n_pred, n_target) per utterance: boundary_scoring's two-pointer
    walk of the frames with pred == 1 (int32 [B, T]) over the segments of the 0/1 targets [B, T].
    What BoundaryMetricStats.append_counts takes; stays on the device."""
    if pred.dim() != 2 or pred.dtype != torch.int32 or not pred.is_cuda:
        raise TypeError(f"boundary_counts: pred must be an int32 [B, T] HIP tensor, got {pred.dtype} "
                        f"{tuple(pred.shape)} on {pred.device}")
    pred = pred.contiguous()
    B, T = pred.shape
    fl = _score_lens(feat_lens, B, pred.device, "boundary_counts feat")
    tgt = _score_seq(targets, (B, T), pred.device, torch.float32, "boundary_counts targets")
    counts = torch.zeros(B, 3, device=pred.device, dtype=torch.int32)
    check(lib().mlvae_boundary_score(B, T, pred.data_ptr(), _p(tgt), _p(fl), counts.data_ptr(),
                                     _stream()), "boundary_score")
    return counts
