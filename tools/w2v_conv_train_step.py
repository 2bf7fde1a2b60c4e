"""Times of training the wav2vec2 conv stack ("The wav2vec2 encoder", "Backward",
"The conv stack").

    python tools/w2v_conv_train_step.py [--layers 24] [--batch 8] [--samples 64000] [--out FILE]

Large-lv60 sizes, bf16, random weights, one GPU, one process.  Device events, two warm-up passes, eight
timed passes of the paths of a group alternating:

  1. one w2v_LSTM_FC training step (encoder, FCBlock 1024 -> 1, masked BCE, both Adam groups' steps) with
     freeze_feature_extractor=True and with train_feature_extractor=True;
  2. the conv stack alone: its forward (Wav2Vec2._conv_stack under no_grad) and its backward
     (ops.W2VConvFn's, timed around backward() only), with their ratio;
  3. ops.w2v_conv0_bwd alone at every workgroup cap of --caps, with the rate at which it reads the
     output's gradient (B T0 C fp32, its one HBM stream) and that rate's share of the 8.0 TB/s HBM peak.
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
from mlvae_hip import _lib, ops  # noqa: E402
from mlvae_hip import optim as hip_optim  # noqa: E402
from modules.fc_block import FCBlock  # noqa: E402
from modules.wav2vec2 import Wav2Vec2  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's HBM3E specification


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stat(name, xs, out, **extra):
    rec = dict(name=name, median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4),
               n=len(xs), **extra)
    print(json.dumps(rec), flush=True)
    if out:
        out.write(json.dumps(rec) + "\n")
    return rec


def alternate(paths, out, reps=1, **meta):
    """reps: calls per timed window (a short kernel is timed over several back-to-back calls)."""
    times = {n: [] for n, _ in paths}
    for i in range(10):  # two warm-ups, eight timed, alternating
        for n, fn in paths:
            t = fn() if getattr(fn, "times_itself", False) else timed(lambda: [fn() for _ in range(reps)]) / reps
            if i >= 2:
                times[n].append(t)
    return {n: stat(n, times[n], out, **meta) for n, _ in paths}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--caps", default="64,128,256,512,1024")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    cfg = dict(R.LARGE_LV60, num_hidden_layers=args.layers)
    B, N = args.batch, args.samples
    T = R.n_frames(cfg, N)
    meta = dict(B=B, N=N, T=T, layers=args.layers)
    wav = R.ragged_wav(1, B=B, N=N, lens=tuple([N] * B)).cuda()
    torch.manual_seed(0)

    # 1. the w2v_LSTM_FC training step, conv stack frozen / trained
    labels = (torch.rand(B, T, device="cuda") < 0.3).float()

    def make_step(**kw):
        enc = Wav2Vec2(config=cfg, precision="bf16", freeze=False, **kw).cuda()
        clf = FCBlock([cfg["hidden_size"], 1]).cuda()
        opts = [hip_optim.Adam(clf.parameters(), lr=3e-4), hip_optim.Adam(enc.parameters(), lr=1e-4)]

        def step():
            logits = clf(enc(wav).contiguous()).squeeze(-1)
            torch.nn.functional.binary_cross_entropy_with_logits(logits, labels).backward()
            for o in opts:
                o.step()
                o.zero_grad()
        return enc, step
    enc_head, step_head = make_step(freeze_feature_extractor=True)
    enc_whole, step_whole = make_step(train_feature_extractor=True)
    r = alternate([("w2v_LSTM_FC step, freeze_feature_extractor", step_head),
                   ("w2v_LSTM_FC step, train_feature_extractor", step_whole)], out, **meta)
    a, b = (r[k]["median_ms"] for k in r)
    stat("w2v_LSTM_FC step: trained / frozen conv stack", [b / a], out, **meta)
    del enc_head, step_head

    # 2. the conv stack alone
    enc = enc_whole
    enc(wav)  # the kernel-side weights are current
    geo = (cfg["conv_kernel"], cfg["conv_stride"], cfg["layer_norm_eps"], True, True, None)
    masters = [enc._w[f"feature_extractor.conv_layers.{i}.{n}"] for i in range(len(cfg["conv_dim"]))
               for n in ("conv.weight", "conv.bias", "layer_norm.weight", "layer_norm.bias")]
    cot = torch.randn(B, T, cfg["conv_dim"][-1], device="cuda")

    def fwd():
        with torch.no_grad():
            enc._conv_stack(wav, None)

    def bwd():
        xf = ops.W2VConvFn.apply(wav, enc._prep, geo, *masters)
        torch.cuda.synchronize()
        return timed(lambda: xf.backward(cot))
    bwd.times_itself = True
    r = alternate([("conv stack forward", fwd), ("conv stack backward", bwd)], out, **meta)
    a, b = (r[k]["median_ms"] for k in r)
    stat("conv stack backward / forward", [b / a], out, **meta)

    # 3. layer 0's backward alone, per workgroup cap
    W, b0, g0, be0 = enc._prep["conv"][0][:4]
    stats = ops.w2v_tensor_stats(wav)
    K, s0 = cfg["conv_kernel"][0], cfg["conv_stride"][0]
    T0 = (N - K) // s0 + 1
    dout = torch.randn(B, T0, W.shape[0], device="cuda")
    nbytes = dout.numel() * 4
    caps = [int(c) for c in args.caps.split(",")]
    default = _lib.lib().mlvae_w2v_conv0_bwd_set_max_blocks(0)
    try:
        def with_cap(c):
            def run():
                _lib.lib().mlvae_w2v_conv0_bwd_set_max_blocks(c)
                ops.w2v_conv0_bwd(wav, stats, W, b0, g0, be0, s0, dout)
            return run
        ref = None
        for c in caps:  # the caps only regroup the sums: the same result to fp32 rounding
            with_cap(c)()
            got = ops.w2v_conv0_bwd(wav, stats, W, b0, g0, be0, s0, dout)[0]
            ref = got if ref is None else ref
            assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item(), c
        r = alternate([(f"conv0_bwd, cap {c} workgroups", with_cap(c)) for c in caps], out, reps=20, T0=T0,
                      dout_bytes=nbytes, default_cap=default, **meta)
        for k, rec in r.items():
            rate = nbytes / (rec["median_ms"] * 1e-3)
            stat(k + ": dout read rate, TB/s", [rate / 1e12], out, share_of_hbm_peak=round(rate / HBM_PEAK, 4), **meta)
    finally:
        _lib.lib().mlvae_w2v_conv0_bwd_set_max_blocks(default)


if __name__ == "__main__":
    main()
