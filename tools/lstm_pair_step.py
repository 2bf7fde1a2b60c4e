"""Timings of the joint recipes' two upstream LSTM stacks on the device, at the recipes' shape
(B = 8, T = 500, F = 120, H = 512, L = 2; DESIGN.md, "The joint recipes and the paired upstream
recurrence").

    python tools/lstm_pair_step.py [--runs 5] [--iters 10] [--steps 10] [--only stacks|step]

1. The recogniser's and the detector's nn.LSTM(F, 512, 2, batch_first=True), forward + backward
   with the input projections and every weight gradient, in fp32 and in bf16: as two ops.lstm
   calls (one chain of recurrence launches per stack) against one ops.lstm_pair (one paired launch
   per layer and direction of the pass).
2. The MD_VAE_joint training step (forward, objectives, backward, Adam) with ``pair_upstream`` off
   and on.

The forms run on the same build in alternating runs; the medians over the runs and the spread
(min .. max) are printed, one JSON line per measurement.  Times are host clocks around work that
ends in a device synchronise.  With MLVAE_LIB_PATH naming a library that lacks the paired entry
points (an older build: the baseline), only the two-ops.lstm form of 1. is measured."""
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


def has_pair():
    from mlvae_hip._lib import lib
    return hasattr(lib(), "mlvae_lstm_pair_fwd") and hasattr(lib(), "mlvae_lstm_pair_bwd")


# --------------------------------------------------------------------------- 1. the two stacks
def stacks(a, prec):
    from mlvae_hip import ops
    B, T, F, H, L = a.B, a.T, a.F, a.H, a.L
    torch.manual_seed(0)
    rnn_a = torch.nn.LSTM(F, H, L, batch_first=True).cuda()
    rnn_b = torch.nn.LSTM(F, H, L, batch_first=True).cuda()
    x = torch.randn(B, T, F).cuda()  # feats: no gradient, as in the recipes
    cot_a, cot_b = torch.randn(B, T, H).cuda(), torch.randn(B, T, H).cuda()
    params = list(rnn_a.parameters()) + list(rnn_b.parameters())

    def finish(out_a, out_b):
        for p in params:
            p.grad = None
        torch.autograd.backward([out_a, out_b], [cot_a, cot_b])
        return out_a, out_b, [p.grad for p in params]

    def two_lstm():
        return finish(ops.lstm(x, rnn_a, True), ops.lstm(x, rnn_b, True))

    def pair():
        return finish(*ops.lstm_pair(x, rnn_a, rnn_b, True))

    forms = {"two_ops_lstm": two_lstm}
    extra = {"iters_per_run": a.iters}
    with ops.precision(prec):
        if has_pair():
            forms["one_ops_lstm_pair"] = pair
            (ya, yb, ga), (pa, pb, gp) = two_lstm(), pair()
            extra["pair_equals_two_bit_for_bit"] = bool(
                torch.equal(ya, pa) and torch.equal(yb, pb) and all(torch.equal(u, v) for u, v in zip(ga, gp)))
        ms = alternate(forms, a.runs, a.iters, warmup=3)
    report(f"two upstream stacks fwd+bwd, B={B} T={T} F={F} H={H} L={L}, {prec}", ms, extra)


# --------------------------------------------------------------------------- 2. the training step
def training_step(a):
    from brain import Stage
    from brain.dataio import PaddedBatch
    from hyperpyyaml import load_hyperpyyaml
    from models.MD_VAE_joint.model import SBModel
    from utils.data_io import SyntheticSet

    ov = ("dataset: synthetic\nmodel_class: MD_VAE_joint\nmodel_name: lstm_pair_step\n"
          f"batch_size: {a.B}\nmodel: !include:../models/MD_VAE_joint/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{"model": {"input_size": a.F}}, ov])
    items = SyntheticSet(a.B, a.F, a.T, a.T, seed=1, md_labels=True, n_phonemes=hp["n_phonemes"]).items
    batch = PaddedBatch(items)
    models = {}
    for name, on in (("pair_upstream_off", False), ("pair_upstream_on", True)):
        m = SBModel(modules=hp["model"]["modules"], hparams=dict(hp["model"], pair_upstream=on),
                    run_opts={"device": "cuda:0"})
        m.init_optimizers()
        m.modules.train()
        m.on_stage_start(Stage.TRAIN, 1)
        models[name] = m
    losses = {}

    def step_of(name):
        m = models[name]

        def step():
            losses[name] = m.fit_batch(batch)
        return step

    import warnings
    warnings.filterwarnings("ignore", message="loss stats logger")
    ms = alternate({name: step_of(name) for name in models}, a.runs, a.steps, warmup=3)
    for m in models.values():
        m.on_stage_end(Stage.TRAIN, 0.0, 1)
    report(f"MD_VAE_joint training step, B={a.B} T={a.T} F={a.F}, fp32 module mode", ms,
           {"steps_per_run": a.steps, "last_loss": {k: float(v) for k, v in losses.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--F", type=int, default=120)
    ap.add_argument("--H", type=int, default=512)
    ap.add_argument("--L", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="fwd+bwd calls of the two stacks per run")
    ap.add_argument("--steps", type=int, default=10, help="training steps per run")
    ap.add_argument("--only", choices=["stacks", "step"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lstm_pair_step.py measures on the device: no HIP device found")
    if a.only != "step":
        for prec in ("fp32", "bf16"):
            stacks(a, prec)
    if a.only != "stacks" and has_pair():
        training_step(a)


if __name__ == "__main__":
    main()
