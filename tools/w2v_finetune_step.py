"""Times of the trainable wav2vec2 encoder ("The wav2vec2 encoder", "Backward").

    python tools/w2v_finetune_step.py [--layers 24] [--batch 8] [--samples 80000] [--out FILE]

Large-lv60 sizes, bf16, feature extractor frozen, random weights, one GPU, one process.  Device
events, two warm-up passes, eight timed passes of each path alternating:

  1. forward + backward of Wav2Vec2(freeze=False, freeze_feature_extractor=True) (loss = sum(out * cot))
     against tests/w2v_ref.py forward + autograd under torch bf16 autocast on the same GPU (its conv
     stack under no_grad, as the module's);
  2. the frozen module's forward;
  3. the weight refresh after an optimizer step (every trainable tensor's version bumped);
  4. the per-family split of one forward + backward: events around every top-level op call.
One JSON line per figure (median and min - max in ms).  A record, not a gate.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "ml-vae_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import w2v_ref as R  # noqa: E402
from mlvae_hip import ops  # noqa: E402
from modules.wav2vec2 import Wav2Vec2  # noqa: E402

FAMILIES = {
    "w2v_linear": "linear GEMMs forward", "w2v_linear_dx": "linear GEMMs dX", "w2v_linear_dw": "linear GEMMs dW",
    "w2v_conv_gemm": "conv stack (frozen)", "w2v_conv0": "conv stack (frozen)",
    "w2v_attention_train": "attention forward", "w2v_attention": "attention forward",
    "w2v_attention_bwd": "attention backward", "w2v_rows": "row kernel forward", "w2v_rows_bwd": "row kernel backward",
    "w2v_regroup": "positional conv", "w2v_pos_conv": "positional conv", "w2v_pos_conv_dx": "positional conv",
    "w2v_pos_conv_dw": "positional conv", "w2v_tensor_stats": "whole-tensor norms", "w2v_scale_shift": "whole-tensor norms",
    "w2v_norm_bwd": "whole-tensor norms", "w2v_colsum": "bias column sums", "w2v_cast": "bf16 casts",
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stat(name, xs, out, **extra):
    rec = dict(name=name, median_ms=round(statistics.median(xs), 3), min_ms=round(min(xs), 3), max_ms=round(max(xs), 3),
               n=len(xs), **extra)
    print(json.dumps(rec), flush=True)
    if out:
        out.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=80000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    cfg = dict(R.LARGE_LV60, num_hidden_layers=args.layers)
    torch.manual_seed(0)
    train = Wav2Vec2(config=cfg, precision="bf16", freeze=False, freeze_feature_extractor=True).cuda()
    frozen = Wav2Vec2(config=cfg, precision="bf16").cuda()
    frozen.load_state_dict(train.state_dict())
    wav = R.ragged_wav(1, B=args.batch, N=args.samples, lens=tuple([args.samples] * args.batch)).cuda()
    T = R.n_frames(cfg, args.samples)
    cot = torch.randn(args.batch, T, cfg["hidden_size"], device="cuda")
    state = {k: v.detach().clone().requires_grad_(Wav2Vec2.trainable_key(k)) for k, v in train.state_dict().items()}
    meta = dict(B=args.batch, N=args.samples, T=T, layers=args.layers)

    def hip_step():
        for p in train.parameters():
            p.grad = None
        (train(wav) * cot).sum().backward()

    def ref_step():
        for v in state.values():
            v.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            o = R.forward(state, cfg, wav)
        (o.float() * cot).sum().backward()

    def frozen_fwd():
        frozen(wav)

    def refresh():
        for p in train.parameters():
            torch.autograd.graph.increment_version(p)
        train._prepare(wav.device, train._prep)

    paths = [("hip forward+backward", hip_step), ("w2v_ref autocast forward+backward", ref_step),
             ("hip frozen forward", frozen_fwd), ("weight refresh, every tensor", refresh)]
    times = {n: [] for n, _ in paths}
    for i in range(10):  # two warm-ups, eight timed, alternating
        for n, fn in paths:
            t = timed(fn)
            if i >= 2:
                times[n].append(t)
    for n, _ in paths:
        stat(n, times[n], out, **meta)

    # the per-family split: events around every top-level op call of one forward + backward
    events, depth = [], [0]

    def wrap(name, fn):
        def inner(*a, **k):
            if depth[0]:
                return fn(*a, **k)
            depth[0] += 1
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            try:
                return fn(*a, **k)
            finally:
                e1.record()
                depth[0] -= 1
                events.append((FAMILIES[name], e0, e1))
        return inner
    saved = {n: getattr(ops, n) for n in FAMILIES}
    for n, fn in saved.items():  # the module's calls go through ops., the autograd pieces' through ops.w2v
        for where in (ops, ops.w2v):
            setattr(where, n, wrap(n, fn))
    try:
        fam = {}
        for _ in range(3):
            events.clear()
            hip_step()
            torch.cuda.synchronize()
            tot = {}
            for f, e0, e1 in events:
                tot[f] = tot.get(f, 0.0) + e0.elapsed_time(e1)
            for f, v in tot.items():
                fam.setdefault(f, []).append(v)
            calls = {}
            for f, _, _ in events:
                calls[f] = calls.get(f, 0) + 1
        for f in sorted(fam, key=lambda f: -statistics.median(fam[f])):
            stat("family: " + f, fam[f], out, calls=calls[f], **meta)
    finally:
        for n, fn in saved.items():
            for where in (ops, ops.w2v):
                setattr(where, n, fn)


if __name__ == "__main__":
    main()
