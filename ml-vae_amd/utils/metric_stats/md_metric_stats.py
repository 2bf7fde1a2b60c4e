"""Mispronunciation-detection scores (semantics of ref:src/utils/metric_stats/md_metric_stats.py).
Two ways in: MD label sequences (the MD-VAE recipes), or phoneme sequences aligned to the canonical
one -- the PER branch the CRDNN_CTC recipes use: the MD labels follow from ``!= canonical`` and
correct_per / misp_per (per_scoring) join the scores.  The aligned path also comes as device
tensors (``append_aligned``: ops.ctc_md_counts' integers and the sequences behind them), kept on
the device and read once per stage.

Labels: 0 = pronounced correctly, 1 = mispronounced; the positive class of PRE / REC / F1 is the
mispronounced one.  Every ratio carries the reference's eps = 1e-6 and is a percentage; all sums
are torch int32 / fp32, so the numbers equal the reference's to the last bit."""
import numpy as np
import torch

from utils.data_utils import boundary_seq_to_seg_seq
from utils.metric_stats.base_metric_stats import PAD_ID, BaseMetricStats, CountsMixin, drop_pad

EPS = 1e-6
SEQ_KEYS = ("gt_phn_seqs", "gt_cnncl_seqs", "gt_md_lbl_seqs", "pred_phn_seqs", "pred_md_lbl_seqs")


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

    def clear(self):
        super().clear()
        self._aligned = []

    def append_aligned(self, ids, counts, ali, phns, cnncls, pred_boundary=None, gt_boundary=None,
                       batch_index=None):
        """The PER branch from device tensors, nothing read here: counts [B, 8] int32
        (ops.ctc_md_counts), ali [B, L] int32 (the prediction aligned to the pronounced sequence,
        -1 = deleted), phns / cnncls [B, L] ids; the utterance's length is counts[:, 4] +
        counts[:, 6].  With pred_boundary [B, T] int32 (ops.ctc_viterbi: -1 past T_i) and
        gt_boundary [B, T] the soft scores of boundary_md_scoring join, as in append."""
        B = len(ids)
        if counts.dim() != 2 or tuple(counts.shape) != (B, 8):
            raise ValueError(f"counts must be [{B}, 8], got {tuple(counts.shape)}")
        for name, x in (("ali", ali), ("phns", phns), ("cnncls", cnncls)):
            if x.dim() != 2 or x.shape[0] != B or x.shape[1] != ali.shape[1]:
                raise ValueError(f"{name} must be [{B}, {ali.shape[1]}], got {tuple(x.shape)}")
        if (pred_boundary is None) != (gt_boundary is None):
            raise ValueError("pred_boundary and gt_boundary come together")
        if pred_boundary is not None and (pred_boundary.dim() != 2 or pred_boundary.shape[0] != B or
                                          tuple(gt_boundary.shape) != tuple(pred_boundary.shape)):
            raise ValueError(f"pred_boundary and gt_boundary must both be [{B}, T], got "
                             f"{tuple(pred_boundary.shape)} and {tuple(gt_boundary.shape)}")
        self._aligned.append((list(ids), [None if x is None else x.detach() for x in
                                          (counts, ali, phns, cnncls, pred_boundary, gt_boundary)],
                              batch_index))

    def _flush_counts(self):
        super()._flush_counts()
        pending, self._aligned = self._aligned, []
        for ids, tensors, batch_index in pending:
            counts, ali, phns, cnncls, pb, gb = (None if x is None else x.cpu() for x in tensors)
            keep = [i for i, u in enumerate(ids) if u != PAD_ID]
            scores = counts_md_scoring(counts[:, :4])
            seqs = {k: [] for k in SEQ_KEYS}
            for i in keep:
                n = int(counts[i, 4] + counts[i, 6])
                hyp, phn, cn = (x[i, :n].tolist() for x in (ali, phns, cnncls))
                pred_md, gt_md = [int(h != c) for h, c in zip(hyp, cn)], [int(p != c) for p, c in zip(phn, cn)]
                if pb is not None:
                    Tb = int((pb[i] >= 0).sum())
                    if int((pb[i, :Tb] == 1).sum()) != n or int((gb[i, :Tb] == 1).sum()) != n:
                        raise ValueError(f"{ids[i]}: {int((pb[i, :Tb] == 1).sum())} predicted and "
                                         f"{int((gb[i, :Tb] == 1).sum())} true boundaries for {n} phonemes "
                                         f"in {Tb} frames (an utterance too short for its CTC chain?)")
                    scores[i].update(boundary_md_scoring(pb[i, :Tb], gb[i, :Tb], pred_md, gt_md))
                scores[i].update(counts_per_scoring(counts[i, 4:8]))
                for k, v in zip(SEQ_KEYS, (phn, cn, gt_md, hyp, pred_md)):
                    seqs[k].append(v)
            ids = [ids[i] for i in keep]
            self._extend(ids, [scores[i] for i in keep], batch_index)
            if ids:
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

    def write_seqs_to_file(self, path):
        """One block per utterance: its id, then the pronounced, canonical and aligned predicted
        phoneme ids (-1 = deleted) and the true and predicted MD labels, a row each."""
        self._flush_counts()
        s = self.saved_seqs
        rows = (("phn", "gt_phn_seqs"), ("cnncl", "gt_cnncl_seqs"), ("pred_phn", "pred_phn_seqs"),
                ("md_lbl", "gt_md_lbl_seqs"), ("pred_md_lbl", "pred_md_lbl_seqs"))
        with open(path, "w") as f:
            for i, u in enumerate(s.get("utt_ids", [])):
                f.write(f"ID: {u}\n")
                for name, key in rows:
                    f.write(f"{name}: " + " ".join(str(int(v)) for v in s[key][i]) + "\n")
                f.write("\n")

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


def _int_1d(x):
    """list / ndarray / tensor of ids -> 1-D int32 tensor."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    elif isinstance(x, list):
        x = torch.Tensor(x)
    elif not isinstance(x, torch.Tensor):
        raise TypeError(f"Unsupported input type: {type(x).__name__}")
    x = x.int().squeeze()
    if x.ndim > 1:
        raise ValueError("Only one-dimension input is allowed")
    return x.reshape(-1)


def _per(wrong, n):
    return wrong / (n + 1e-5) * 100


def per_scoring(pred_phn_seq, gt_phn_seq, gt_cnncl_seq):
    """Error rate of the aligned prediction against the pronounced phonemes, over the positions
    pronounced canonically (correct_per) and over the mispronounced ones (misp_per); eps = 1e-5."""
    pred, gt, cn = _int_1d(pred_phn_seq), _int_1d(gt_phn_seq), _int_1d(gt_cnncl_seq)
    if not len(gt) == len(cn) == len(pred):
        raise ValueError(f"Inconsistent lengths: {len(gt)}, {len(cn)}, {len(pred)}")
    ok, bad = torch.where(gt == cn)[0], torch.where(gt != cn)[0]
    return {"correct_per": _per(torch.sum(pred[ok] != gt[ok]), len(ok)),
            "misp_per": _per(torch.sum(pred[bad] != gt[bad]), len(bad))}


def counts_per_scoring(c):
    """per_scoring from (canonical positions, of them wrong, mispronounced positions, of them
    wrong): the same int64 / fp32 arithmetic."""
    n_ok, w_ok, n_bad, w_bad = (int(v) for v in c)
    return {"correct_per": _per(torch.tensor(w_ok), n_ok), "misp_per": _per(torch.tensor(w_bad), n_bad)}


def _md_labels(phn_seqs, cnncl_seqs):
    if phn_seqs is None or cnncl_seqs is None:
        raise ValueError("MD labels need either label sequences or phoneme and canonical sequences")
    if len(phn_seqs) != len(cnncl_seqs):
        raise ValueError(f"Inconsistent batch size: {len(phn_seqs)} != {len(cnncl_seqs)}")
    out = []
    for p, c in zip(phn_seqs, cnncl_seqs):
        if len(p) != len(c):
            raise ValueError(f"Inconsistent sequence lengths: {len(p)} != {len(c)}")
        out.append([int(a != b) for a, b in zip(p, c)])  # 0 = pronounced correctly, 1 = mispronounced
    return out


def batch_seq_md_scoring(pred_md_lbl_seqs=None, gt_md_lbl_seqs=None, pred_boundary_seqs=None,
                         gt_boundary_seqs=None, boundary_md_scoring_tol=5, pred_phn_seqs=None,
                         gt_phn_seqs=None, gt_cnncl_seqs=None):
    """Scores of a batch: (one dict per utterance, the sequences kept for the result file).
    With boundary sequences given, the soft scores join the plain ones.  MD label sequences that
    are not given follow from the (aligned) phoneme sequences against the canonical one; with all
    three phoneme sequences given, correct_per / misp_per join too."""
    for x in (pred_phn_seqs, gt_phn_seqs, gt_cnncl_seqs):
        if x is not None and not isinstance(x, list):
            raise TypeError(f"Input type must be list, not {type(x).__name__}")
    if pred_md_lbl_seqs is None and pred_phn_seqs is not None:
        pred_md_lbl_seqs = _md_labels(pred_phn_seqs, gt_cnncl_seqs)
    if gt_md_lbl_seqs is None and gt_phn_seqs is not None:
        gt_md_lbl_seqs = _md_labels(gt_phn_seqs, gt_cnncl_seqs)
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
        if pred_phn_seqs is not None and gt_phn_seqs is not None and gt_cnncl_seqs is not None:
            s.update(per_scoring(pred_phn_seqs[i], gt_phn_seqs[i], gt_cnncl_seqs[i]))
        scores.append(s)
    # a phoneme sequence that is not given: the reference fills it with its 'sil' id
    sil = [[7] * len(p) for p in pred_md_lbl_seqs]

    def kept(x):
        return [list(s) for s in (sil if x is None else x)]

    seqs = {
        "gt_phn_seqs": kept(gt_phn_seqs),
        "gt_cnncl_seqs": kept(gt_cnncl_seqs),
        "gt_md_lbl_seqs": list(gt_md_lbl_seqs),
        "pred_phn_seqs": kept(pred_phn_seqs),
        "pred_md_lbl_seqs": list(pred_md_lbl_seqs),
    }
    return scores, seqs
