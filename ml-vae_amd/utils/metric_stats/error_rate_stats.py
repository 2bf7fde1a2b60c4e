"""Phoneme error rate of the CRDNN_CTC recipes (the summary keys of SpeechBrain's ErrorRateStats
that the reference reads, ref:src/models/CRDNN_CTC/model.py:26-27,73-87, keyed phn_per /
cnncl_per): ``append_counts`` takes the [B, 4] integers (insertions, deletions, substitutions,
reference tokens) that ops.edit_align leaves on the device, keeps the tensor as it is and reads it
once, in summarize() / state() -- no host sync per batch.

error_rate = 100 (I + D + S) / sum L_a over the utterances of the stage (a corpus-level ratio of
integer sums, so it does not depend on the order of the utterances); 0 for a stage without
reference tokens.  state() / merge() as the other stats: the ranks' rows are put into the
single-process order; the zero-length fillers of a short rank slice are dropped."""
import torch

from utils.metric_stats.base_metric_stats import PAD_ID, BaseMetricStats

KEYS = ("error_rate", "insertions", "deletions", "substitutions", "num_ref_tokens")


class ErrorRateStats:
    def __init__(self):
        self.clear()

    def clear(self):
        self.ids, self.rows, self.order = [], [], []  # rows: [I, D, S, L_a] per utterance
        self._pending = []
        self._batches = 0

    def append_counts(self, ids, counts, batch_index=None):
        if counts.dim() != 2 or counts.shape[1] != 4 or counts.shape[0] != len(ids):
            raise ValueError(f"counts must be [{len(ids)}, 4], got {tuple(counts.shape)}")
        self._pending.append((list(ids), counts.detach(), batch_index))

    def _flush(self):
        pending, self._pending = self._pending, []
        for ids, counts, batch_index in pending:
            b = self._batches if batch_index is None else int(batch_index)
            self._batches += 1
            for j, (u, row) in enumerate(zip(ids, counts.cpu().tolist())):
                if u == PAD_ID:  # the fillers of a short rank slice are not utterances
                    continue
                self.ids.append(u)
                self.rows.append([int(v) for v in row])
                self.order.append((b, j))

    def state(self):
        self._flush()
        return {"ids": list(self.ids), "order": list(self.order), "rows": [list(r) for r in self.rows]}

    def merge(self, states):
        perm = BaseMetricStats.merged_order(states)
        self.clear()
        self.ids = [states[r]["ids"][n] for r, n in perm]
        self.rows = [list(states[r]["rows"][n]) for r, n in perm]
        self.order = [tuple(states[r]["order"][n]) for r, n in perm]
        return perm

    def summarize(self, field=None):
        self._flush()
        if not self.rows:
            raise ValueError("No metrics saved yet")
        ins, dele, sub, ref = (int(v) for v in torch.tensor(self.rows, dtype=torch.int64).sum(0))
        out = {"error_rate": 100.0 * (ins + dele + sub) / ref if ref else 0.0, "insertions": ins,
               "deletions": dele, "substitutions": sub, "num_ref_tokens": ref}
        return out if field is None else out[field]

    def write_stats(self, f):
        s = self.summarize()
        f.write("\t".join(f"{k}: {s[k]}" for k in KEYS) + "\n")
        for u, (ins, dele, sub, ref) in zip(self.ids, self.rows):
            f.write(f"{u}\t{ins}\t{dele}\t{sub}\t{ref}\n")
