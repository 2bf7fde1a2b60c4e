"""Timings of the LSTM_FC recipe's fused head on the device, at the recipe's shape
(B = 8, T = 500, E = fc_size = 64; DESIGN.md, the LSTM_FC baseline).

    python tools/flvl_head_step.py [--runs 5] [--iters 200] [--steps 10]

1. The head, forward + backward: ops.flvl_md_head (one kernel forward, one kernel and the sum of
   its partials backward) and the masked mean, the counts left on the device -- against the same
   tail in torch ops on the device: ops.linear for the 64 -> 2 layer, the reference's
   binary_cross_entropy_with_logits expression, the masked mean, argmax and undo_padding of the
   predictions and the labels to host lists (what the reference does on every batch).
2. A full training step (forward, objectives, backward, Adam) of models/LSTM_FC at the yaml's
   4 x 1024 LSTM, with the fused head and with the torch-op tail.  The torch-op form exists in
   this tool only.

Both pairs run on the same build in alternating runs; the medians over the runs and the spread
(min .. max) are printed, one JSON line per measurement.  Times are host clocks around work that
ends in a device synchronise."""
import argparse
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
import torch.nn.functional as F_  # noqa: E402


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


def torch_tail(h, weight, bias, labels, lens, pos_weight):
    """The reference's tail in torch ops on the device (ref:src/models/LSTM_FC/model.py:30-61):
    (logits, mean loss, predicted lists, true lists)."""
    from mlvae_hip import ops
    from utils.data_utils import undo_padding
    out = ops.linear(h, weight, bias, False)
    targets = torch.stack([1 - labels, labels], dim=-1).type(out.dtype)
    loss_e = F_.binary_cross_entropy_with_logits(out, targets, reduction="none", pos_weight=pos_weight)
    loss = ops.masked_mean(loss_e, lens)
    pred = torch.argmax(out, dim=-1)
    return out, loss, undo_padding(pred, lens), undo_padding(labels, lens)


# --------------------------------------------------------------------------- 1. the head
def head(a):
    from mlvae_hip import ops
    B, T, E = a.B, a.T, a.E
    g = torch.Generator().manual_seed(0)
    h = torch.randn(B, T, E, generator=g).cuda().requires_grad_(True)
    w = (0.3 * torch.randn(2, E, generator=g)).cuda().requires_grad_(True)
    b = torch.randn(2, generator=g).cuda().requires_grad_(True)
    labels = (torch.rand(B, T, generator=g) < 0.2).long().cuda()
    lens = (0.5 + 0.5 * torch.rand(B, generator=g)).cuda()
    lens[0] = 1.0
    pw = torch.tensor([1.0, a.misp_weight]).cuda()

    def finish(loss):
        h.grad = w.grad = b.grad = None
        loss.backward()
        return loss.detach(), (h.grad, w.grad, b.grad)

    def hip():
        _, loss_e, _, counts = ops.flvl_md_head(h, w, b, labels, lens, (1.0, a.misp_weight))
        return finish(ops.masked_mean(loss_e, lens)) + (counts,)

    def torch_ops():
        _, loss, pred, gt = torch_tail(h, w, b, labels, lens, pw)
        return finish(loss) + ((pred, gt),)

    (hl, hg, _), (tl, tg, _) = hip(), torch_ops()
    err = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip((hl, *hg), (tl, *tg)))
    ms = alternate({"hip_fused": hip, "torch_ops": torch_ops}, a.runs, a.iters, warmup=20)
    report(f"LSTM_FC head fwd+bwd, B={B} T={T} E={E}", ms,
           {"max_rel_diff_hip_vs_torch": err, "iters_per_run": a.iters})


# --------------------------------------------------------------------------- 2. the training step
def training_step(a):
    from brain import Stage
    from brain.dataio import PaddedBatch
    from hyperpyyaml import load_hyperpyyaml
    from models.LSTM_FC.model import SBModel
    from utils.data_io import SyntheticSet

    ov = ("dataset: synthetic\nmodel_class: LSTM_FC\nmodel_name: flvl_head_step\n"
          f"batch_size: {a.B}\nmodel: !include:../models/LSTM_FC/model.yaml\n")

    class TorchTail(SBModel):
        """The reference's form: the FCBlock to the end, then torch ops and host lists."""

        def compute_forward(self, batch, stage):
            batch = batch.to(self.device)
            feats, _ = batch["feat"]
            out = self.modules["lstm"](feats.contiguous())[0]
            return {"h": self._hidden(out)}

        def _hidden(self, out):
            from mlvae_hip import ops
            for lin, act in self.modules["fc"].linear_plan()[:-1]:
                out = ops.linear(out, lin.weight, lin.bias, act)
            return out

        def compute_objectives(self, predictions, batch, stage):
            last = self.modules["fc"].linear_plan()[-1][0]
            labels, lens = batch["flvl_gt_md_lbl_seq"][0], batch["feat"][1]
            pw = torch.tensor([1, self.hparams.misp_weight]).type(torch.float32).to(self.device)
            _, loss, pred, gt = torch_tail(predictions["h"], last.weight, last.bias, labels, lens, pw)
            self.stats_loggers["flvl_md_stats"].append(batch["id"], pred_md_lbl_seqs=pred, gt_md_lbl_seqs=gt)
            return loss

    items = SyntheticSet(a.B, a.F, a.T, a.T, seed=1, md_labels=True).items
    models = {}
    for name, cls in (("hip_fused", SBModel), ("torch_ops", TorchTail)):
        with open(os.path.join(PKG, "config", "run.yaml")) as f:  # a model of its own per form
            hp = load_hyperpyyaml(f, [{"model": {"input_size": a.F, "lr": 1e-4}}, ov])
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
    scores = {name: m.stats_loggers["flvl_md_stats"].summarize() for name, m in models.items()}
    hpm = models["hip_fused"].hparams
    report(f"LSTM_FC training step, B={a.B} T={a.T} F={a.F}, LSTM {hpm.lstm_num_layers}x{hpm.lstm_hidden_size}, "
           "fp32 module mode", ms,
           {"steps_per_run": a.steps, "last_loss": {k: float(v) for k, v in losses.items()},
            "train_flvl_md": scores})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--E", type=int, default=64)
    ap.add_argument("--F", type=int, default=120)
    ap.add_argument("--misp_weight", type=float, default=10.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="head calls per run")
    ap.add_argument("--steps", type=int, default=10, help="training steps per run")
    ap.add_argument("--only", choices=["head", "step"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/flvl_head_step.py measures on the device: no HIP device found")
    if a.only != "step":
        head(a)
    if a.only != "head":
        training_step(a)


if __name__ == "__main__":
    main()
