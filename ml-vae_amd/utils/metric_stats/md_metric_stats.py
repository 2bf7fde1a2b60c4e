"""Mispronunciation-detection scores (semantics of ref:src/utils/metric_stats/md_metric_stats.py,
for the arguments the MD-VAE recipe passes; the PER branch is not part of this build).

Labels: 0 = pronounced correctly, 1 = mispronounced; the positive class of PRE / REC / F1 is the
mispronounced one.  Every ratio carries the reference's eps = 1e-6 and is a percentage; all sums
are torch int32 / fp32, so the numbers equal the reference's to the last bit."""
import numpy as np
import torch

from utils.data_utils import boundary_seq_to_seg_seq
from utils.metric_stats.base_metric_stats import BaseMetricStats, CountsMixin, drop_pad

EPS = 1e-6


class MDMetricStats(CountsMixin, BaseMetricStats):
    """append_counts takes the [B, 4] integer counts (both correct, both mispronounced, missed,
    false alarm; ops.flvl_md_head's), kept on the device and read once by summarize() / state()."""
    n_counts = 4

    def __init__(self):
        super().__init__(metric_fn=batch_seq_md_scoring)
        self.saved_seqs = {}

    def append(self, ids, batch_index=None, **kwargs):
        self._require_fn()
        ids, kwargs = drop_pad(ids, kwargs)
        if not ids:  # a rank slice of fillers alone
            self._batches += 1
            return
        scores, seqs = self.metric_fn(**kwargs)
        self._extend(ids, scores, batch_index)
        seqs["utt_ids"] = ids
        if not self.saved_seqs:
            self.saved_seqs = seqs
        else:
            for key in self.saved_seqs:
                self.saved_seqs[key].extend(seqs[key])

    def state(self):
        st = super().state()
        st["saved_seqs"] = self.saved_seqs
        return st

    def merge(self, states):
        perm = super().merge(states)
        seqs = [st.get("saved_seqs") or {} for st in states]
        keys = next((list(s) for s in seqs if s), [])
        self.saved_seqs = {k: [seqs[r][k][n] for r, n in perm] for k in keys}
        return perm

    def summarize(self, field=None):
        means = super().summarize()
        # F1 of the corpus = F1 of the mean PRE and the mean REC, not the mean of the F1s
        pre, rec = means["PRE"], means["REC"]
        means["F1"] = (2 * pre * rec) / (pre + rec + EPS)
        means = {k: round(v.item(), 2) for k, v in means.items()}
        return means if field is None else means[field]


def _binary_1d(x):
    """list / ndarray / tensor of 0s and 1s -> 1-D int32 tensor."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    elif isinstance(x, list):
        x = torch.Tensor(x)
    elif not isinstance(x, torch.Tensor):
        raise TypeError(f"Unsupported input type: {type(x).__name__}")
    x = x.int().squeeze()
    if x.ndim > 1:
        raise ValueError("Only one-dimension input is allowed")
    if not bool(((x == 0) | (x == 1)).all()):
        raise ValueError("Only binary input values are supported")
    return x


def _counts(pred, gt):
    """(both correct, both mispronounced, missed, false alarm)."""
    return (torch.sum((1 - pred) * (1 - gt)), torch.sum(pred * gt),
            torch.sum((1 - pred) * gt), torch.sum(pred * (1 - gt)))


def binary_seq_md_scoring(prediction, target):
    """ACC / PRE / REC / F1 of one utterance's predicted against true MD labels."""
    pred, gt = _binary_1d(prediction), _binary_1d(target)
    if len(pred) != len(gt):
        raise ValueError("Inconsistent lengths for prediction and target sequences: "
                         f"{len(pred)} != {len(gt)}")
    ok, hit, miss, fa = _counts(pred, gt)
    acc = (ok + hit) / (ok + hit + miss + fa + EPS) * 100
    pre = hit / (hit + fa + EPS) * 100
    rec = hit / (hit + miss + EPS) * 100
    return {"ACC": acc, "PRE": pre, "REC": rec, "F1": 2 * pre * rec / (pre + rec + EPS)}


def counts_md_scoring(counts):
    """binary_seq_md_scoring from the four counts of each utterance ([B, 4] integers, in the order
    of _counts): one score dict per utterance, in the same torch int32 / fp32 arithmetic, so
    equal to the last bit to scoring the sequences themselves."""
    counts = torch.as_tensor(counts).to("cpu", torch.int32)
    if counts.dim() != 2 or counts.shape[1] != 4:
        raise ValueError(f"counts must be [B, 4], got {tuple(counts.shape)}")
    scores = []
    for ok, hit, miss, fa in counts:
        acc = (ok + hit) / (ok + hit + miss + fa + EPS) * 100
        pre = hit / (hit + fa + EPS) * 100
        rec = hit / (hit + miss + EPS) * 100
        scores.append({"ACC": acc, "PRE": pre, "REC": rec, "F1": 2 * pre * rec / (pre + rec + EPS)})
    return scores


MDMetricStats.counts_fn = staticmethod(counts_md_scoring)


def compute_boundary_iou(pred_seg_seq, gt_seg_seq):
    """Intersection over union of each predicted segment with its true one ([L, 2] each)."""
    assert len(pred_seg_seq) == len(gt_seg_seq)
    ious = []
    for (ps, pe), (gs, ge) in zip(pred_seg_seq, gt_seg_seq):
        inter = max(0, min(pe, ge) - max(ps, gs))
        union = max(pe, ge) - min(ps, gs)
        iou = inter / (union + 1e-5)
        assert torch.isfinite(iou)
        ious.append(iou)
    return torch.tensor(ious)


def boundary_md_scoring(pred_boundary_seq, gt_boundary_seq, pred_md_lbl_seq, gt_md_lbl_seq, tol=5):
    """MD scores in which a hit counts by the IoU of its segment ("soft"), and the mean IoU over
    all / the correct / the mispronounced phonemes.  tol is accepted and unused, as in the
    reference."""
    pb, gb = _binary_1d(pred_boundary_seq), _binary_1d(gt_boundary_seq)
    pred, gt = _binary_1d(pred_md_lbl_seq), _binary_1d(gt_md_lbl_seq)
    assert len(pb) == len(gb)
    assert int((pb == 1).sum()) == int((gb == 1).sum()) == len(pred) == len(gt)

    iou = compute_boundary_iou(boundary_seq_to_seg_seq(pb), boundary_seq_to_seg_seq(gb))

    def mean_where(lbl):
        sel = iou[torch.where(gt == lbl)[0]]
        return torch.mean(sel) * 100 if len(sel) > 0 else torch.tensor(0.0)

    correct_iou, misp_iou = mean_where(0), mean_where(1)
    assert torch.isfinite(correct_iou) and torch.isfinite(misp_iou)

    ok, hit, miss, fa = _counts(pred, gt)
    soft_ok = torch.sum((1 - pred) * (1 - gt) * iou)
    soft_hit = torch.sum(pred * gt * iou)
    pre = soft_hit / (hit + fa + EPS) * 100
    rec = soft_hit / (hit + miss + EPS) * 100
    return {
        "soft_ACC": (soft_ok + soft_hit) / (ok + hit + miss + fa + EPS) * 100,
        "soft_PRE": pre,
        "soft_REC": rec,
        "soft_F1": 2 * pre * rec / (pre + rec + EPS),
        "ave_iou": torch.mean(iou) * 100,
        "correct_iou": correct_iou,
        "misp_iou": misp_iou,
    }


def batch_seq_md_scoring(pred_md_lbl_seqs=None, gt_md_lbl_seqs=None, pred_boundary_seqs=None,
                         gt_boundary_seqs=None, boundary_md_scoring_tol=5):
    """Scores of a batch: (one dict per utterance, the sequences kept for the result file).
    With boundary sequences given, the soft scores join the plain ones."""
    for x in (pred_md_lbl_seqs, gt_md_lbl_seqs):
        if not isinstance(x, list):
            raise TypeError(f"Input type must be list, not {type(x).__name__}")
    if len(pred_md_lbl_seqs) != len(gt_md_lbl_seqs):
        raise ValueError(f"Inconsistent batch size: {len(pred_md_lbl_seqs)} != {len(gt_md_lbl_seqs)}")
    scores = []
    for i, (pred, gt) in enumerate(zip(pred_md_lbl_seqs, gt_md_lbl_seqs)):
        s = binary_seq_md_scoring(pred, gt)
        if pred_boundary_seqs is not None:
            s.update(boundary_md_scoring(pred_boundary_seqs[i], gt_boundary_seqs[i], pred, gt,
                                         boundary_md_scoring_tol))
        scores.append(s)
    # no phoneme sequences in this recipe: the reference fills them with its 'sil' id
    sil = [[7] * len(p) for p in pred_md_lbl_seqs]
    seqs = {
        "gt_phn_seqs": [list(s) for s in sil],
        "gt_cnncl_seqs": [list(s) for s in sil],
        "gt_md_lbl_seqs": list(gt_md_lbl_seqs),
        "pred_phn_seqs": [list(s) for s in sil],
        "pred_md_lbl_seqs": list(pred_md_lbl_seqs),
    }
    return scores, seqs
