"""Timings of the upstream-module recipes' scoring tail on the device, at the recipes' shape
(B = 8, T = 500, C = n_phonemes + 2 = 41; DESIGN.md, the upstream-module recipes).

    python tools/score_step.py [--runs 5] [--iters 100] [--steps 10]

1. The scoring tail of one batch, both recipes: the device form (ops.phn_acc_counts, or
   ops.boundary_topk + ops.boundary_counts, and append_counts: the counts stay on the device) --
   against the host-list form the reference runs on every batch: undo_padding_tensor of every
   sequence, torch.topk per utterance, and the stats object's list append (which scores on the
   host).  The host-list form exists in the stats classes for parity and in this tool.
2. A full training step (forward, objectives, backward, Adam) of models/test_phn_classifier and
   models/test_b_ind_classifier at the yamls' 2 x 512 LSTM, with the device scoring and with the
   host-list tail.

Each pair runs on the same build in alternating runs; the medians over the runs and the spread
(min .. max) are printed, one JSON line per measurement.  Times are host clocks around work that
ends in a device synchronise (the host-list form synchronises by itself)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ml-vae_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(forms, runs, iters, warmup):
    """{name: [ms per call, one per run]}: the forms take turns, run after run."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    out = {name: [] for name in forms}
    for _ in range(runs):
        for name, fn in forms.items():
            out[name].append(timed(fn, iters))
    return out


def report(what, ms, extra=None):
    rec = {"measurement": what}
    for name, v in ms.items():
        rec[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "runs": len(v)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)


def undo_padding_tensor(batch, lengths):
    """Padded [B, T, ...] + relative lengths -> the list of unpadded tensors (one host read of a
    length per utterance, as the reference's helper)."""
    n = batch.shape[1]
    return [seq.narrow(0, 0, int(torch.round(l * n))) for seq, l in zip(batch, lengths)]


def host_phn(stats, ids, out, feat_lens, flvl, plvl, plvl_lens, boundary):
    stats.append(ids, predictions=undo_padding_tensor(out, feat_lens),
                 flvl_targets=undo_padding_tensor(flvl, feat_lens),
                 plvl_targets=undo_padding_tensor(plvl, plvl_lens),
                 boundary_seqs=undo_padding_tensor(boundary, feat_lens))


def host_bnd(stats, ids, v, feat_lens, fa, gt):
    preds = []
    for i, row in enumerate(undo_padding_tensor(v, feat_lens)):
        k = torch.sum(fa[i, :]).int()
        pred = torch.zeros_like(row)
        pred[torch.topk(row, k=k)[1]] = 1
        preds.append(pred)
    stats.append(ids, predictions=preds, targets=undo_padding_tensor(gt, feat_lens))


def synthetic_batch(a):
    from brain.dataio import PaddedBatch
    from utils.data_io import SyntheticSet
    items = SyntheticSet(a.B, a.F, a.T * 3 // 4, a.T, seed=1, md_labels=True, phn_labels=True,
                         n_phonemes=a.C - 2).items
    return items, PaddedBatch(items).to("cuda:0")


# --------------------------------------------------------------------------- 1. the scoring tails
def tails(a):
    from mlvae_hip import ops
    from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
    from utils.metric_stats.phn_acc_metric_stats import PhnAccMetricStats
    _, batch = synthetic_batch(a)
    ids = batch["id"]
    feat_lens = batch["feat"][1]
    B, T = batch["feat"][0].shape[:2]
    g = torch.Generator().manual_seed(0)
    out = torch.randn(B, T, a.C, generator=g).cuda()
    v = torch.rand(B, T, generator=g).cuda()
    plvl, plvl_lens = batch["gt_cnncl_seq"]
    flvl, fa, gt = (batch[k][0] for k in ("flvl_gt_cnncl_seq", "fa_boundary_seq", "gt_boundary_seq"))
    stats = {}

    def fresh(name, cls):
        stats[name] = cls()
        return stats[name]

    def phn_device():
        fresh("pd", PhnAccMetricStats).append_counts(
            ids, ops.phn_acc_counts(out, feat_lens, flvl, plvl, plvl_lens, gt))

    def phn_host():
        host_phn(fresh("ph", PhnAccMetricStats), ids, out, feat_lens, flvl, plvl, plvl_lens, gt)

    def bnd_device():
        pred = ops.boundary_topk(v, feat_lens, fa)
        fresh("bd", BoundaryMetricStats).append_counts(ids, ops.boundary_counts(pred, gt, feat_lens))

    def bnd_host():
        host_bnd(fresh("bh", BoundaryMetricStats), ids, v, feat_lens, fa, gt)

    for pair, dev, host in (("phn_acc", phn_device, phn_host), ("boundary", bnd_device, bnd_host)):
        ms = alternate({"device_counts": dev, "host_lists": host}, a.runs, a.iters, warmup=10)
        d, h = ("pd", "ph") if pair == "phn_acc" else ("bd", "bh")
        same = stats[d].summarize() == stats[h].summarize()
        report(f"{pair} scoring tail of one batch, B={B} T={T} C={a.C}", ms,
               {"iters_per_run": a.iters, "summaries_equal": same, "summary": stats[d].summarize()})
    ops.raise_score_err()


# --------------------------------------------------------------------------- 2. the training steps
def training_steps(a):
    from brain import Stage
    from brain.dataio import PaddedBatch
    from hyperpyyaml import load_hyperpyyaml
    from utils.data_utils import apply_lens_to_loss
    items, _ = synthetic_batch(a)

    for recipe, key in (("test_phn_classifier", "phn_acc_stats"), ("test_b_ind_classifier", "boundary_stats")):
        SBModel = importlib.import_module(f"models.{recipe}.model").SBModel

        class HostTail(SBModel):
            """The reference's form of compute_objectives: host lists on every batch."""

            def compute_objectives(self, predictions, batch, stage):
                feat_lens = batch["feat"][1]
                st = self.stats_loggers[key]
                if recipe == "test_phn_classifier":
                    loss = apply_lens_to_loss(predictions["losses"]["phn_recog_bce_loss"], feat_lens)
                    host_phn(st, batch["id"], predictions["out"].detach(), feat_lens,
                             batch["flvl_gt_cnncl_seq"][0], *batch["gt_cnncl_seq"], batch["gt_boundary_seq"][0])
                    return loss
                loss = 0
                for k, value in predictions["losses"].items():
                    loss = loss + getattr(self.hparams, k.replace("_loss", "_weight"), 1) * \
                        apply_lens_to_loss(value, feat_lens)
                host_bnd(st, batch["id"], predictions["boundary_v"].detach(), feat_lens,
                         batch["fa_boundary_seq"][0], batch["gt_boundary_seq"][0])
                return loss

        ov = (f"dataset: synthetic\nmodel_class: {recipe}\nmodel_name: score_step\n"
              f"batch_size: {a.B}\nn_phonemes: {a.C - 2}\nmodel: !include:../models/{recipe}/model.yaml\n")
        models = {}
        for name, cls in (("device_counts", SBModel), ("host_lists", HostTail)):
            with open(os.path.join(PKG, "config", "run.yaml")) as f:  # a model of its own per form
                hp = load_hyperpyyaml(f, [{"model": {"input_size": a.F}}, ov])
            m = cls(modules=hp["model"]["modules"], hparams=hp["model"], run_opts={"device": "cuda:0"})
            m.init_optimizers()
            m.modules.train()
            m.on_stage_start(Stage.TRAIN, 1)
            models[name] = m
        losses = {}

        def step_of(name):
            m = models[name]

            def step():
                losses[name] = m.fit_batch(PaddedBatch(items))
            return step

        ms = alternate({name: step_of(name) for name in models}, a.runs, a.steps, warmup=3)
        hpm = models["device_counts"].hparams
        report(f"{recipe} training step, B={a.B} T={a.T} F={a.F}, LSTM {hpm.rnn_num_layers}x{hpm.rnn_hidden_size}, "
               "fp32 module mode", ms,
               {"steps_per_run": a.steps, "last_loss": {k: float(v) for k, v in losses.items()},
                "train_scores": {name: m.stats_loggers[key].summarize() for name, m in models.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--C", type=int, default=41)
    ap.add_argument("--F", type=int, default=120)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100, help="scoring tails per run")
    ap.add_argument("--steps", type=int, default=10, help="training steps per run")
    ap.add_argument("--only", choices=["tails", "steps"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/score_step.py measures on the device: no HIP device found")
    if a.only != "steps":
        tails(a)
    if a.only != "tails":
        training_steps(a)


if __name__ == "__main__":
    main()
