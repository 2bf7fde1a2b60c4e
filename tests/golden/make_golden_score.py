"""Golden fixture for the per-utterance scoring kernels (csrc/score.hip) and the count forms of
PhnAccMetricStats / BoundaryMetricStats: ``score_cases.npz``.

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs
it.  It reuses the import shims of ``make_golden_md_recipe.py`` and scores single utterances with
the reference's own ``boundary_scoring``, ``flvl_phn_acc_scoring`` and ``plvl_phn_acc_scoring``,
the predicted boundaries built as the reference recipe builds them (ref:src/models/
test_b_ind_classifier/model.py:58-63: ``torch.topk`` with k = the sum of the fa row).  Only data is
written: each case's padded inputs and the reference's outputs (the chosen frames, ``correct`` and
every score as float64).

Cases: T <= 64 frames padded to 64, C = 7 classes, at most 16 phonemes.  Twelve are written by
hand (k = 0, k = T_i, k = 1, T = 1, a target without a flag at frame 0, a prediction on a shared
segment edge, several predictions in one segment, no predictions, no targets, one-frame segments,
a last segment that ends at T_i, predictions past a segment), the others are random.  The padding
holds NaN, inf and stray ones (the fa row alone is zero-padded: the reference sums the whole row).
A case is accepted only if every valid frame's and every segment sum's top-2 gap is >= 1e-3 of the
largest magnitude and the k-th and (k+1)-th largest boundary_v differ by >= 1e-3 relative.

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_score.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_md_recipe as R  # noqa: E402,F401  (generator-only shims, reference src on sys.path)
from utils.metric_stats.boundary_metric_stats import boundary_scoring  # noqa: E402  (reference)
from utils.metric_stats.phn_acc_metric_stats import (  # noqa: E402  (reference)
    flvl_phn_acc_scoring, plvl_phn_acc_scoring)

TP, C, LP = 64, 7, 16
GAP = 1e-3

# (T_i, predicted frames, true boundary frames)
HAND = [
    (12, [], [0, 5, 9]),                 # k = 0: no predictions
    (6, [0, 1, 2, 3, 4, 5], [0, 3]),     # k = T_i
    (10, [4], [0, 4, 8]),                # k = 1, on the edge two segments share
    (1, [0], [0]),                       # T = 1
    (1, [], []),                         # T = 1, nothing at all
    (10, [0, 1, 5, 8], [3, 7]),          # no flag at frame 0: predictions before the first segment
    (12, [4, 8], [0, 4, 8]),             # each on a shared edge: matched by the earlier segment
    (16, [1, 2, 3, 12], [0, 10]),        # several predictions in one segment
    (8, [2, 5], []),                     # no targets
    (8, [0, 2, 3, 6], [0, 1, 2, 3, 7]),  # one-frame segments
    (9, [8], [0, 6]),                    # the last segment ends at T_i
    (8, [5, 7], [0, 2, 4, 6]),           # predictions past a segment: it is missed
]


def _gap_ok(x):
    """top-2 gap of every row of x [n, C] >= GAP of the largest magnitude."""
    top = torch.topk(x, 2, dim=-1).values
    return bool(((top[:, 0] - top[:, 1]) >= GAP * x.abs().max()).all())


def _case(Ti, pred_frames, gt_frames, g):
    # boundary part: v puts the wanted frames on top, fa carries k ones
    k = len(pred_frames)
    v = 0.4 * torch.rand(Ti, generator=g)
    v[pred_frames] = 0.6 + 0.4 * torch.rand(k, generator=g)
    fa = torch.zeros(Ti)
    fa[torch.randperm(Ti, generator=g)[:k]] = 1.0
    gt = torch.zeros(Ti)
    gt[gt_frames] = 1.0
    srt = torch.sort(v, descending=True).values
    if 0 < k < Ti and not (srt[k - 1] - srt[k]) >= GAP * srt[k - 1].abs():
        return None
    # as the recipe does
    num_segments = torch.sum(fa).int()
    pred = torch.zeros_like(v)
    _, indices = torch.topk(v, k=num_segments)
    pred[indices] = 1
    scores = boundary_scoring(pred, gt)
    # the function returns no count: correct = pre (n_pred + eps) / 100, an integer to ~1e-6
    correct = int(round(scores["pre"] * (float(pred.sum()) + 1e-6) / 100))
    # phoneme part: Li segments from frame 0
    Li = int(torch.randint(1, min(Ti, LP) + 1, (1,), generator=g))
    pb = torch.zeros(Ti)
    pb[0] = 1.0
    if Li > 1:
        pb[torch.randperm(Ti - 1, generator=g)[:Li - 1] + 1] = 1.0
    logits = 3.0 * torch.randn(Ti, C, generator=g)
    starts = torch.where(pb == 1)[0].tolist() + [Ti]
    sums = torch.stack([logits[a:b].sum(0) for a, b in zip(starts[:-1], starts[1:])])
    if not (_gap_ok(logits) and _gap_ok(sums)):
        return None
    seg = torch.cumsum(pb, 0).long() - 1
    keep_f = torch.rand(Ti, generator=g) < 0.6
    flvl_tgt = torch.where(keep_f, logits.argmax(-1), torch.randint(0, C, (Ti,), generator=g))
    keep_p = torch.rand(Li, generator=g) < 0.6
    plvl_tgt = torch.where(keep_p, sums.argmax(-1), torch.randint(0, C, (Li,), generator=g))
    flvl_acc = flvl_phn_acc_scoring(logits, flvl_tgt)
    plvl_acc = plvl_phn_acc_scoring(logits, plvl_tgt, pb)
    return dict(Ti=Ti, Li=Li, k=k, v=v, fa=fa, gt=gt, chosen=pred, correct=correct,
                n_pred=int(pred.sum()), n_target=int(gt.sum()), scores=scores, logits=logits,
                flvl_tgt=flvl_tgt, plvl_tgt=plvl_tgt, pb=pb, seg=seg, flvl_acc=flvl_acc, plvl_acc=plvl_acc,
                flvl_correct=int((logits.argmax(-1) == flvl_tgt).sum()),
                plvl_correct=int((sums.argmax(-1) == plvl_tgt).sum()))


def _accepted(spec, g):
    for _ in range(50):
        c = _case(*spec, g)
        if c is not None:
            return c
    raise SystemExit(f"no accepted draw for {spec}")


def main():
    g = torch.Generator().manual_seed(20240)
    specs = list(HAND)
    while len(specs) < 40:
        Ti = int(torch.randint(2, TP + 1, (1,), generator=g))
        k = int(torch.randint(0, max(Ti // 3, 1) + 1, (1,), generator=g))
        n = int(torch.randint(1, max(Ti // 3, 1) + 1, (1,), generator=g))
        pf = sorted(torch.randperm(Ti, generator=g)[:k].tolist())
        gf = sorted(set(torch.randperm(Ti, generator=g)[:n].tolist()) |
                    ({0} if float(torch.rand(1, generator=g)) < 0.8 else set()))
        specs.append((Ti, pf, gf))
    cases = [_accepted(s, g) for s in specs]
    N = len(cases)
    nan, inf = float("nan"), float("inf")
    rec = {
        "T": np.array([c["Ti"] for c in cases], np.int32),
        "L": np.array([c["Li"] for c in cases], np.int32),
        "k": np.array([c["k"] for c in cases], np.int32),
        "feat_lens": np.array([c["Ti"] / TP for c in cases], np.float32),
        "phn_lens": np.array([c["Li"] / LP for c in cases], np.float32),
        "logits": np.full((N, TP, C), nan, np.float32),
        "flvl_tgt": np.zeros((N, TP), np.int64),
        "plvl_tgt": np.zeros((N, LP), np.int64),
        "phn_boundary": np.ones((N, TP), np.float32),   # stray ones past T_i
        "boundary_v": np.full((N, TP), inf, np.float32),
        "fa_boundary": np.zeros((N, TP), np.float32),   # zero padding: the reference sums the row
        "gt_boundary": np.ones((N, TP), np.float32),
        "chosen": np.full((N, TP), -1, np.int32),
    }
    for key in ("correct", "n_pred", "n_target", "flvl_correct", "plvl_correct"):
        rec[key] = np.array([c[key] for c in cases], np.int32)
    for key in ("pre", "rec", "f1", "r_value"):
        rec[key] = np.array([c["scores"][key] for c in cases], np.float64)
    for key in ("flvl_acc", "plvl_acc"):
        rec[key] = np.array([c[key] for c in cases], np.float64)
    for i, c in enumerate(cases):
        Ti, Li = c["Ti"], c["Li"]
        assert int(torch.round(torch.tensor(rec["feat_lens"][i]) * TP)) == Ti
        assert int(torch.round(torch.tensor(rec["phn_lens"][i]) * LP)) == Li
        rec["logits"][i, :Ti] = c["logits"].numpy()
        rec["logits"][i, Ti:, 0::2] = inf  # NaN and inf past T_i
        rec["flvl_tgt"][i, :Ti] = c["flvl_tgt"].numpy()
        rec["flvl_tgt"][i, Ti:] = 3
        rec["plvl_tgt"][i, :Li] = c["plvl_tgt"].numpy()
        rec["plvl_tgt"][i, Li:] = 3
        rec["phn_boundary"][i, :Ti] = c["pb"].numpy()
        rec["boundary_v"][i, :Ti] = c["v"].numpy()
        rec["boundary_v"][i, Ti + 1::2] = nan
        rec["fa_boundary"][i, :Ti] = c["fa"].numpy()
        rec["gt_boundary"][i, :Ti] = c["gt"].numpy()
        rec["chosen"][i, :Ti] = c["chosen"].numpy().astype(np.int32)
    # at least one utterance strictly between 0 and 100 at each level, and for the boundaries
    for key in ("flvl_acc", "plvl_acc", "pre", "rec"):
        assert ((rec[key] > 0) & (rec[key] < 100)).any(), key
    path = os.path.join(R.OUT_DIR, "score_cases.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes,", N, "cases")


if __name__ == "__main__":
    torch.set_num_threads(1)
    main()
