"""Per-utterance score accumulator (semantics of ref:src/utils/metric_stats/base_metric_stats.py):
``append`` scores a batch with ``metric_fn`` (a list of {key: score} per utterance), ``summarize``
averages every key over the utterances seen (torch fp32 mean)."""
import torch


class BaseMetricStats:
    def __init__(self, metric_fn=None):
        self.metric_fn = metric_fn
        self.clear()

    def clear(self):
        self.ids, self.scores_list, self.metric_keys = [], [], []

    def _require_fn(self):
        if self.metric_fn is None:
            raise ValueError("No metric_fn has been provided")

    def _extend(self, ids, scores):
        self.ids.extend(ids)
        self.scores_list.extend(scores)
        if not self.metric_keys:
            self.metric_keys = list(self.scores_list[0].keys())

    def append(self, ids, **kwargs):
        self._require_fn()
        self._extend(ids, self.metric_fn(**kwargs))

    def summarize(self, field=None):
        if not self.metric_keys:
            raise ValueError("No metrics saved yet")
        means = {k: torch.mean(torch.tensor([s[k] for s in self.scores_list]))
                 for k in self.metric_keys}
        return means if field is None else means[field]

    def write_stats(self, f):
        f.write("\t".join(str(v) for v in self.summarize().values()) + "\n")
