"""Timings of the Kaldi-compatible front end on the device (the Kaldi front end).

    python tools/kaldi_fbank_step.py [--B 16 96] [--frames 200] [--runs 7] [--iters 50]

The kernels of csrc/kaldi_fbank.hip -- ops.kaldi_fbank (tile + finish), ops.cmvn_accumulate and
ops.cmvn_apply over 4 speakers -- next to ops.fbank (the SpeechBrain front end, csrc/fbank.hip) on
the same waveforms, 4 s utterances at full length.  The forms take turns, round after round, on one
build in one process; HIP events around `iters` calls; the medians over the rounds and the spread
(min .. max) are printed, one JSON line per batch size, with the kernels' arithmetic and traffic
per frame.  cmvn_accumulate / cmvn_apply include their error word's host read (one sync per call,
as the corpus builder pays it).  The front end runs once per corpus, not on the training step: a
record, not a gate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ml-vae_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from fbank_step import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[16, 96])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/kaldi_fbank_step.py measures on the device: no HIP device found")
    from mlvae_hip import ops
    sr, hop_ms, win_ms, M, S = 16000, 20, 25, 40, 4
    hop, L, P = sr * hop_ms // 1000, sr * win_ms // 1000, 512
    K, D = P // 2, 3 * M
    for B in a.B:
        N = a.frames * hop
        g = torch.Generator().manual_seed(B)
        n = torch.arange(N, dtype=torch.float64)
        f1 = 300 + 800 * torch.rand(B, 1, generator=g, dtype=torch.float64)
        f2 = 1400 + 2600 * torch.rand(B, 1, generator=g, dtype=torch.float64)
        wav = (0.5 * torch.sin(2 * torch.pi * f1 * n / sr) + 0.3 * torch.sin(2 * torch.pi * f2 * n / sr) +
               0.01 * torch.randn(B, N, generator=g, dtype=torch.float64)).float().cuda()
        kw = dict(sample_rate=sr, hop_length=hop_ms, win_length=win_ms, n_mels=M)
        feats, frames = ops.kaldi_fbank(wav, None, **kw)
        T = feats.shape[1]
        spk = (torch.arange(B) % S).int().cuda()
        stats = torch.zeros(S, 2 * D + 1, device="cuda", dtype=torch.float64)
        ops.cmvn_accumulate(stats, feats, frames, spk)
        # the apply is timed in place over and over: statistics of mean 0 and variance 1 keep the
        # values where they are
        unit = torch.zeros_like(stats)
        unit[:, D:] = 1.0
        work = feats.clone()
        forms = {"kaldi_fbank": lambda: ops.kaldi_fbank(wav, None, **kw)[0],
                 "cmvn_accumulate": lambda: ops.cmvn_accumulate(stats, feats, frames, spk),
                 "cmvn_apply": lambda: ops.cmvn_apply(work, frames, spk, unit),
                 "speechbrain_fbank": lambda: ops.fbank(wav, None, n_fft=400, **kw)[0]}
        ms = alternate(forms, a.runs, a.iters, warmup=5)
        rec = {"measurement": f"kaldi fbank + deltas + per-speaker CMVN, B={B} N={N} ({T} frames), {sr} Hz "
                              f"L={L} P={P} hop={hop} mels={M} speakers={S}",
               "iters_per_round": a.iters,
               # per frame: the DFT as a product over the window, |X|^2, the mel projection
               "flop_per_frame": 2 * L * 2 * K + 3 * K + 2 * K * M,
               # per frame: hop new samples in, the log-mel frame out and back in, three output rows
               "hbm_bytes_per_frame": 4 * hop + 4 * M + 4 * M + 4 * D,
               # per frame: CMVN reads the row once to accumulate, reads and writes it to apply
               "cmvn_bytes_per_frame": 4 * D + 8 * D}
        for name, v in ms.items():
            rec[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                         "max_ms": round(max(v), 4), "rounds": len(v)}
        rec["frames_per_s_kaldi_fbank"] = round(B * T / (rec["kaldi_fbank"]["median_ms"] * 1e-3))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
