"""Phoneme-classification accuracy (semantics of ref:src/utils/metric_stats/
phn_acc_metric_stats.py): per utterance, the share (percent) of frames whose argmax over the
classes is the canonical phoneme (flvl_acc), and the share of phoneme segments whose summed
outputs' argmax is (plvl_acc).

``append`` scores lists of unpadded tensors on the host as the reference does.  ``append_counts``
takes the [B, 4] integers (flvl_correct, T_i, plvl_correct, L_i) that ops.phn_acc_counts leaves
on the device and reads them once, in summarize() / state(): the fp32 mean of 0/1 values is the
exact integer sum and one division, so both routes give the same numbers to the last bit."""
import torch

from utils.metric_stats.base_metric_stats import BaseMetricStats, CountsMixin


class PhnAccMetricStats(CountsMixin, BaseMetricStats):
    n_counts = 4

    def __init__(self):
        super().__init__(metric_fn=batch_phn_acc_scoring)

    def summarize(self, field=None):
        means = {k: round(v.item(), 2) for k, v in super().summarize().items()}
        return means if field is None else means[field]


def flvl_phn_acc_scoring(prediction, target):
    """prediction [T, N] model output, target [T] ids -> accuracy in percent."""
    if prediction.ndim != 2 or target.ndim != 1:
        raise ValueError("Prediction must have two dimensions, and target must have one dimension")
    if prediction.shape[0] != target.shape[0]:
        raise ValueError(f"Inconsistent input lengths: {prediction.shape[0]} != {target.shape[0]}")
    arg = torch.argmax(prediction, dim=-1)
    return (arg == target.type(arg.dtype)).float().mean().item() * 100


def plvl_phn_acc_scoring(prediction, target, boundary_seq):
    """prediction [T, N], target [L] ids, boundary_seq [T] 0/1 flags that open the L segments:
    the outputs are summed over each segment, then scored as frames are."""
    assert torch.sum(boundary_seq) == len(target)
    idx = torch.where(boundary_seq == 1)[0]
    idx = torch.cat([idx, idx.new_full((1,), len(boundary_seq))])
    durations = idx[1:] - idx[:-1]
    assert torch.sum(durations) == prediction.shape[0]
    sums = [torch.sum(p, dim=0) for p in torch.split(prediction, durations.tolist())]
    assert len(sums) == len(target)
    return flvl_phn_acc_scoring(torch.stack(sums, dim=0), target)


def batch_phn_acc_scoring(predictions, flvl_targets, plvl_targets=None, boundary_seqs=None):
    """One {'flvl_acc', 'plvl_acc'} per utterance; plvl_acc is 0 without phoneme targets."""
    for x in (predictions, flvl_targets, plvl_targets, boundary_seqs):
        if x is not None and type(x) is not list:
            raise TypeError(f"Input type must be list, not {type(x).__name__}")
    for x in (flvl_targets, plvl_targets, boundary_seqs):
        if x is not None and len(x) != len(predictions):
            raise ValueError(f"Inconsistent batch size: {len(x)} != {len(predictions)}")
    if plvl_targets is not None and boundary_seqs is None:
        raise ValueError("boundary_seqs must be provided when plvl_targets is not None")
    scores = []
    for i, pred in enumerate(predictions):
        plvl = 0
        if plvl_targets is not None:
            plvl = plvl_phn_acc_scoring(pred, plvl_targets[i], boundary_seqs[i])
        scores.append({"flvl_acc": flvl_phn_acc_scoring(pred, flvl_targets[i]), "plvl_acc": plvl})
    return scores


def counts_phn_acc_scoring(counts):
    """batch_phn_acc_scoring from (flvl_correct, T_i, plvl_correct, L_i) of each utterance
    ([B, 4] integers): the fp32 ratio is what .float().mean() computes.  L_i == 0 with
    plvl_correct == 0 is an utterance scored without phoneme targets: plvl_acc 0."""
    counts = torch.as_tensor(counts).to("cpu", torch.int32)
    if counts.dim() != 2 or counts.shape[1] != 4:
        raise ValueError(f"counts must be [B, 4], got {tuple(counts.shape)}")
    c = counts.to(torch.float32)
    flvl, plvl = c[:, 0] / c[:, 1], c[:, 2] / c[:, 3]
    return [{"flvl_acc": flvl[i].item() * 100, "plvl_acc": plvl[i].item() * 100 if counts[i, 3] else 0}
            for i in range(len(counts))]


PhnAccMetricStats.counts_fn = staticmethod(counts_phn_acc_scoring)
