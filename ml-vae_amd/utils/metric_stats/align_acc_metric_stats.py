"""Alignment accuracy of the HMM_DNN_ALI recipe (ref:src/models/HMM_DNN_ALI/model.py:21-23,89:
SpeechBrain's MetricStats over HMMAligner.calc_accuracy): per utterance, the share (percent) of
frames whose aligned state belongs to the phoneme of the ground-truth segment that holds the
frame; ``summarize("average")`` is the mean over the utterances -- the recipe's accuracy.average.

``append_counts`` takes the [B, 2] integers (frames correct, T_i) that ops.align_counts leaves on
the device and reads them once, in summarize() / state(): no host sync per batch."""
import torch

from utils.metric_stats.base_metric_stats import BaseMetricStats, CountsMixin


def counts_align_acc_scoring(counts):
    """[B, 2] integers (frames correct, T_i) -> one {'average': percent} per utterance (fp32)."""
    counts = torch.as_tensor(counts).to("cpu", torch.int32)
    if counts.dim() != 2 or counts.shape[1] != 2:
        raise ValueError(f"counts must be [B, 2], got {tuple(counts.shape)}")
    c = counts.to(torch.float32)
    acc = c[:, 0] / c[:, 1] * 100
    return [{"average": acc[i].item()} for i in range(len(counts))]


class AlignAccMetricStats(CountsMixin, BaseMetricStats):
    n_counts = 2
    counts_fn = staticmethod(counts_align_acc_scoring)

    def __init__(self):
        super().__init__(metric_fn=None)

    def summarize(self, field=None):
        means = {k: v.item() for k, v in super().summarize().items()}
        return means if field is None else means[field]
