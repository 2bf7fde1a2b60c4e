"""Golden fixture for the MD and boundary metrics (utils/metric_stats/{md,boundary}_metric_stats.py).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs it.  It reuses the
import shims of ``make_golden.py`` and calls the reference's own scoring functions and stats
classes from the reference checkout (``make_golden.REF_SRC``); only ``md_metrics.json`` (data) is written.

Reference code exercised (read-only):
  * ``binary_seq_md_scoring``, ``boundary_md_scoring``, ``MDMetricStats``
                                    ref:src/utils/metric_stats/md_metric_stats.py
  * ``boundary_scoring``, ``BoundaryMetricStats``
                                    ref:src/utils/metric_stats/boundary_metric_stats.py

Six seeded utterances, each with L phonemes over T frames: predicted / true boundary flags (frame
0 set, exactly L ones each) and predicted / true MD labels; utterance 1 has no mispronunciation,
utterance 2 has every phoneme mispronounced.  The stats classes are fed in two batches, as the
recipe feeds them.

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_md_metrics.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402,F401  (generator-only shims, reference src on sys.path)
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats, boundary_scoring  # noqa: E402
from utils.metric_stats.md_metric_stats import (MDMetricStats, binary_seq_md_scoring,  # noqa: E402
                                                boundary_md_scoring)

OUT_DIR = make_golden.OUT_DIR


def _boundaries(T, L, g):
    idx = torch.cat([torch.zeros(1, dtype=torch.int64),
                     1 + torch.randperm(T - 1, generator=g)[:L - 1].sort().values])
    seq = torch.zeros(T, dtype=torch.int64)
    seq[idx] = 1
    return seq


def _floats(d):
    return {k: float(v) for k, v in d.items()}


def main():
    g = torch.Generator().manual_seed(41)
    utts = []
    for i, (T, L) in enumerate([(30, 5), (24, 4), (40, 7), (18, 3), (55, 9), (33, 6)]):
        gt_md = (torch.rand(L, generator=g) < 0.35).long()
        if i == 1:
            gt_md = torch.zeros(L, dtype=torch.int64)
        if i == 2:
            gt_md = torch.ones(L, dtype=torch.int64)
        pred_md = torch.where(torch.rand(L, generator=g) < 0.3, 1 - gt_md, gt_md)
        utts.append({"id": f"utt{i}", "pred_boundary": _boundaries(T, L, g).tolist(),
                     "gt_boundary": [float(v) for v in _boundaries(T, L, g).tolist()],
                     "pred_md": pred_md.tolist(), "gt_md": gt_md.tolist()})
    md_stats, bnd_stats = MDMetricStats(), BoundaryMetricStats()
    for u in utts:
        # the recipe's types: decoded boundaries int64 ndarray, decoded labels int lists, ground
        # truth as undo_padding's lists
        pb = np.asarray(u["pred_boundary"], dtype=np.int64)
        u["binary"] = _floats(binary_seq_md_scoring(u["pred_md"], u["gt_md"]))
        u["boundary_md"] = _floats(boundary_md_scoring(pb, u["gt_boundary"], u["pred_md"], u["gt_md"]))
        u["boundary"] = _floats(boundary_scoring(pb, u["gt_boundary"]))
    for lo, hi in ((0, 4), (4, 6)):
        part = utts[lo:hi]
        pbs = [np.asarray(u["pred_boundary"], dtype=np.int64) for u in part]
        md_stats.append(ids=[u["id"] for u in part], pred_md_lbl_seqs=[u["pred_md"] for u in part],
                        gt_md_lbl_seqs=[u["gt_md"] for u in part], pred_boundary_seqs=pbs,
                        gt_boundary_seqs=[u["gt_boundary"] for u in part])
        bnd_stats.append(ids=[u["id"] for u in part], predictions=pbs,
                         targets=[u["gt_boundary"] for u in part])
    out = {"utterances": utts, "batches": [[0, 4], [4, 6]],
           "md_summary": md_stats.summarize(), "md_F1": md_stats.summarize("F1"),
           "boundary_summary": bnd_stats.summarize(), "boundary_f1": bnd_stats.summarize("f1")}
    path = os.path.join(OUT_DIR, "md_metrics.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path, out["md_summary"], out["boundary_summary"])


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
