"""Per-utterance score accumulator (semantics of ref:src/utils/metric_stats/base_metric_stats.py):
``append`` scores a batch with ``metric_fn`` (a list of {key: score} per utterance), ``summarize``
averages every key over the utterances seen (torch fp32 mean).

Data parallel: the zero-length fillers of a short rank slice (id ``__pad__``, utils/data_io.py)
are rows of the batch, not utterances: ``append`` drops them before scoring.  Each rank scores
its own utterances; ``state()`` is what a rank sends to rank 0 and ``merge(states)`` puts the
ranks' entries into the order (global batch index, rank, position in the batch) -- the order the
single process sees the utterances in -- so ``summarize`` returns the single-process numbers (a
torch fp32 mean depends on the order of its terms)."""
import torch

PAD_ID = "__pad__"


def drop_pad(ids, kwargs):
    """(ids, kwargs) without the filler rows: every list argument as long as ids loses them."""
    keep = [i for i, u in enumerate(ids) if u != PAD_ID]
    if len(keep) == len(ids):
        return list(ids), kwargs
    out = {k: ([v[i] for i in keep] if isinstance(v, list) and len(v) == len(ids) else v)
           for k, v in kwargs.items()}
    return [ids[i] for i in keep], out


class BaseMetricStats:
    def __init__(self, metric_fn=None):
        self.metric_fn = metric_fn
        self.clear()

    def clear(self):
        self.ids, self.scores_list, self.metric_keys = [], [], []
        self.order = []  # (global batch index, position in the batch) of every entry
        self._batches = 0

    def _require_fn(self):
        if self.metric_fn is None:
            raise ValueError("No metric_fn has been provided")

    def _extend(self, ids, scores, batch_index=None):
        """batch_index: the global batch the ids come from (default: the count of appends)."""
        b = self._batches if batch_index is None else int(batch_index)
        self._batches += 1
        self.ids.extend(ids)
        self.scores_list.extend(scores)
        self.order.extend((b, j) for j in range(len(ids)))
        if not self.metric_keys and self.scores_list:
            self.metric_keys = list(self.scores_list[0].keys())

    def append(self, ids, batch_index=None, **kwargs):
        self._require_fn()
        ids, kwargs = drop_pad(ids, kwargs)
        self._extend(ids, self.metric_fn(**kwargs) if ids else [], batch_index)

    def state(self):
        """What merge() needs from this rank (plain lists and numbers: picklable)."""
        return {"ids": list(self.ids), "order": list(self.order),
                "scores": [{k: float(v) for k, v in s.items()} for s in self.scores_list]}

    @staticmethod
    def merged_order(states):
        """[(rank, index in that rank's lists)] sorted by (batch index, rank, position)."""
        keys = [(b, r, j, n) for r, st in enumerate(states) for n, (b, j) in enumerate(st["order"])]
        return [(r, n) for _, r, _, n in sorted(keys)]

    def merge(self, states):
        """Replace this accumulator's entries by the ranks' (states[r] = rank r's state())."""
        perm = self.merged_order(states)
        self.clear()
        self.ids = [states[r]["ids"][n] for r, n in perm]
        self.scores_list = [{k: torch.tensor(v) for k, v in states[r]["scores"][n].items()}
                            for r, n in perm]
        self.order = [tuple(states[r]["order"][n]) for r, n in perm]
        if self.scores_list:
            self.metric_keys = list(self.scores_list[0].keys())
        return perm

    def summarize(self, field=None):
        if not self.metric_keys:
            raise ValueError("No metrics saved yet")
        means = {k: torch.mean(torch.tensor([s[k] for s in self.scores_list]))
                 for k in self.metric_keys}
        return means if field is None else means[field]

    def write_stats(self, f):
        f.write("\t".join(str(v) for v in self.summarize().values()) + "\n")


class CountsMixin:
    """append_counts for a stats class whose scores follow from a few integers per utterance that
    a kernel left on the device ([B, n_counts] int32): the tensor is kept as it is and read once,
    by summarize() / state() -- no host sync per batch.  The class names ``n_counts`` and
    ``counts_fn`` ([b, n_counts] CPU int32 -> one score dict per utterance).  Filler rows
    (``__pad__``) are dropped; batch_index orders the entries for merge() as append's does."""
    n_counts = 0
    counts_fn = None

    def clear(self):
        super().clear()
        self._pending = []

    def append_counts(self, ids, counts, batch_index=None):
        if counts.dim() != 2 or counts.shape[1] != self.n_counts or counts.shape[0] != len(ids):
            raise ValueError(f"counts must be [{len(ids)}, {self.n_counts}], got {tuple(counts.shape)}")
        self._pending.append((list(ids), counts.detach(), batch_index))

    def _flush_counts(self):
        pending, self._pending = self._pending, []
        for ids, counts, batch_index in pending:
            keep = [i for i, u in enumerate(ids) if u != PAD_ID]
            counts = counts.cpu()
            if len(keep) < len(ids):  # the fillers of a short rank slice are not utterances
                ids, counts = [ids[i] for i in keep], counts[keep]
            self._extend(ids, type(self).counts_fn(counts) if ids else [], batch_index)

    def state(self):
        self._flush_counts()
        return super().state()

    def summarize(self, field=None):
        self._flush_counts()
        return super().summarize(field)
