"""Boundary-detection scores (semantics of ref:src/utils/metric_stats/boundary_metric_stats.py):
per-utterance precision / recall / F1 (percent, eps = 1e-6) of the predicted boundary frames
against the true segments, and the R-value."""
import numpy as np
import torch

from utils.metric_stats.base_metric_stats import BaseMetricStats, CountsMixin

EPS = 1e-6


class BoundaryMetricStats(CountsMixin, BaseMetricStats):
    """append scores lists of sequences on the host; append_counts takes the [B, 3] device counts
    of ops.boundary_counts and reads them once, in summarize() / state()."""
    n_counts = 3

    def __init__(self):
        super().__init__(metric_fn=batch_boundary_scoring)

    def summarize(self, field=None):
        means = {k: round(v.item(), 2) for k, v in super().summarize().items()}
        return means if field is None else means[field]


def _as_1d(x):
    if isinstance(x, list):
        x = torch.tensor(x)
    elif isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    elif not isinstance(x, torch.Tensor):
        raise ValueError(f"invalid input type: {type(x)}")
    if x.ndim != 1:
        raise ValueError("only one-dimensional inputs are supported")
    return x


def boundary_scoring(prediction, target):
    """A predicted boundary is correct when it falls inside the next unmatched true segment
    [start, next start] (both ends included; the last segment ends at T); each true segment
    matches at most one prediction, both walked in time order."""
    pred, gt = _as_1d(prediction), _as_1d(target)
    if len(pred) != len(gt):
        raise ValueError(f"inconsistent input lengths: {len(pred)} != {len(gt)}")
    hyp = torch.where(pred == 1)[0].tolist()
    starts = torch.where(gt == 1)[0].tolist() + [len(gt)]
    segments = list(zip(starts[:-1], starts[1:]))

    correct = h = s = 0
    while s < len(segments) and h < len(hyp):
        left, right = segments[s]
        if hyp[h] < left:      # before the segment: a spurious boundary
            h += 1
        elif hyp[h] <= right:  # inside: matched
            correct += 1
            h += 1
            s += 1
        else:                  # past it: the segment was missed
            s += 1

    pre = (correct / (torch.sum(pred) + EPS) * 100).item()
    rec = (correct / (torch.sum(gt) + EPS) * 100).item()
    return _scores(pre, rec)


def _scores(pre, rec):
    """f1 and the R-value from the precision and the recall (percent), in double."""
    f1 = 2 * pre * rec / (pre + rec + EPS)
    # R-value (Rasanen et al. 2009) from the recall and the over-segmentation
    over = pre / (rec + EPS) - 1
    r1 = np.sqrt((100 - rec) ** 2 + over ** 2)
    r2 = np.abs(rec - over - 100) / np.sqrt(2)
    return {"pre": pre, "rec": rec, "f1": f1, "r_value": (1 - (r1 + r2) / 200) * 100}


def counts_boundary_scoring(counts):
    """boundary_scoring from (correct, n_pred, n_target) of each utterance ([B, 3] integers): pre
    and rec are the same fp32 tensor ratios (a sum of 0/1 flags is the exact integer), f1 and the
    R-value the same double arithmetic, so the scores equal the sequences' to the last bit."""
    counts = torch.as_tensor(counts).to("cpu", torch.int32)
    if counts.dim() != 2 or counts.shape[1] != 3:
        raise ValueError(f"counts must be [B, 3], got {tuple(counts.shape)}")
    scores = []
    for correct, n_pred, n_target in counts.tolist():
        pre = (correct / (torch.tensor(n_pred, dtype=torch.float32) + EPS) * 100).item()
        rec = (correct / (torch.tensor(n_target, dtype=torch.float32) + EPS) * 100).item()
        scores.append(_scores(pre, rec))
    return scores


BoundaryMetricStats.counts_fn = staticmethod(counts_boundary_scoring)


def batch_boundary_scoring(predictions, targets):
    for x in (predictions, targets):
        if type(x) is not list:
            raise TypeError(f"Input type must be list, not {type(x).__name__}")
    if len(predictions) != len(targets):
        raise ValueError(f"Inconsistent batch size: {len(predictions)} != {len(targets)}")
    return [boundary_scoring(p, t) for p, t in zip(predictions, targets)]
