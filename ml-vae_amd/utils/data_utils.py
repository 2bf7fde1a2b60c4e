"""Loss masking helpers (ref:src/utils/data_utils.py:67-104) on libmlvae."""
import torch

from mlvae_hip import ops


def length_to_mask(length, max_len=None, dtype=None, device=None):
    """SpeechBrain 0.5 semantics (un-vendored in the reference): arange(T) < length (fp32).
    Host-side helper for bookkeeping; the kernels apply the same rule on the device."""
    if max_len is None:
        max_len = int(length.max().long().item())
    mask = torch.arange(max_len, device=length.device, dtype=length.dtype).expand(
        len(length), max_len) < length.unsqueeze(1)
    return mask.to(dtype=dtype or length.dtype, device=device or length.device)


def apply_lens_to_loss(loss, lens, reduction='mean'):
    """sum(loss * mask) / sum(mask) ('mean'), / B ('batchmean') or per utterance ('batch'),
    mask = frames t < lens*T (relative lengths, fp32 compare as SpeechBrain's length_to_mask)."""
    return ops.masked_mean(loss, lens, reduction)


def boundary_seq_to_seg_seq(boundary_seq):
    """0/1 boundary flags [T] -> segments [L, 2] of (start, end) frame indices, one per flag
    (ref:src/utils/data_utils.py:159-181).  The last segment's end is the NUMBER of boundaries,
    not T, as in the reference (its T-terminated variant is commented out there): the MD
    scores' IoU of the last phoneme is computed against that value, and stays comparable."""
    idx = torch.where(boundary_seq == 1)[0]
    segs = [[idx[i], idx[i + 1]] for i in range(len(idx) - 1)]
    segs.append([idx[-1], len(idx)])
    return torch.tensor(segs)


def undo_padding(batch, lengths):
    """Padded [B, Lmax] + relative lengths [B] -> list of per-utterance lists (SpeechBrain's
    undo_padding: int(round(len * Lmax)) items each)."""
    n = batch.shape[1]
    return [batch[i, :int(torch.round(l * n))].tolist() for i, l in enumerate(lengths)]


def apply_weight(x, weight):
    """Mixture weighting as one HIP launch (ref:src/utils/data_utils.py:32-64).

    x: (B, T, N, C) or (B, T, N * C); weight: (B, T, N) -> (B, T, C)."""
    return ops.apply_weight(x, weight)
