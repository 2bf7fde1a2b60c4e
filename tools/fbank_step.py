"""Timings of the feature front end on the device (the feature front end).

    python tools/fbank_step.py [--B 16] [--frames 200] [--runs 7] [--iters 50]

The two kernels of csrc/fbank.hip (ops.fbank) against the composed device form of the same
features on the same tensors: torch.stft (center=True, pad_mode="constant") + |X|^2 + the mel
matmul + log + the per-utterance floor + the two delta passes as replicate-padded conv1d's.  Every
utterance is full length (the composed form has no per-utterance lengths).  The forms take turns,
round after round, on one build in one process; HIP events around `iters` calls; the medians over
the rounds and the spread (min .. max) are printed, one JSON line per shape, with the largest
difference between the two forms' outputs and the kernels' arithmetic per frame.  The front end
runs once per corpus, not on the training step: a record, not a gate."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ml-vae_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402


def timed(fn, iters):
    """ms per call between two HIP events around `iters` calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(forms, runs, iters, warmup):
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    out = {name: [] for name in forms}
    for _ in range(runs):
        for name, fn in forms.items():
            out[name].append(timed(fn, iters))
    return out


def composed(wav, hop, win, n_fft, window, fb):
    """The same features from torch's device ops (full-length utterances)."""
    st = torch.stft(wav, n_fft, hop, win, window, center=True, pad_mode="constant", return_complex=True)
    p = (st.real ** 2 + st.imag ** 2).transpose(1, 2)  # [B, T, bins]
    db = 10.0 * torch.log10(torch.clamp(p @ fb, min=1e-10))
    db = torch.maximum(db, db.amax(dim=(1, 2), keepdim=True) - 80.0)
    k = torch.arange(-2, 3, device=wav.device, dtype=wav.dtype).view(1, 1, 5) / 10.0

    def delta(x):  # [B, T, M]
        B, T, M = x.shape
        y = torch.nn.functional.pad(x.transpose(1, 2).reshape(B * M, 1, T), (2, 2), mode="replicate")
        return torch.nn.functional.conv1d(y, k).reshape(B, M, T).transpose(1, 2)

    d = delta(db)
    return torch.cat([db, d, delta(d)], dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[16, 96])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/fbank_step.py measures on the device: no HIP device found")
    import fbank_ref as R
    from mlvae_hip import ops
    sr, hop_ms, win_ms, n_fft, M = 16000, 20, 25, 400, 40
    hop, win = R.geometry(sr, hop_ms, win_ms)
    lo = (n_fft - win) // 2
    window = torch.from_numpy(R.window(win, n_fft)[lo:lo + win]).float().cuda()
    fb = torch.from_numpy(R.mel_filters(sr, n_fft, M)).float().cuda()
    K = n_fft // 2 + 1
    for B in a.B:
        N = a.frames * hop
        g = torch.Generator().manual_seed(B)
        n = torch.arange(N, dtype=torch.float64)
        f1 = 300 + 800 * torch.rand(B, 1, generator=g, dtype=torch.float64)
        f2 = 1400 + 2600 * torch.rand(B, 1, generator=g, dtype=torch.float64)
        wav = (0.5 * torch.sin(2 * torch.pi * f1 * n / sr) + 0.3 * torch.sin(2 * torch.pi * f2 * n / sr) +
               0.01 * torch.randn(B, N, generator=g, dtype=torch.float64)).float().cuda()
        kw = dict(sample_rate=sr, hop_length=hop_ms, win_length=win_ms, n_fft=n_fft, n_mels=M)
        forms = {"hip_kernels": lambda: ops.fbank(wav, None, **kw)[0],
                 "composed_torch": lambda: composed(wav, hop, win, n_fft, window, fb)}
        diff = float((forms["hip_kernels"]() - forms["composed_torch"]()).abs().max())
        ms = alternate(forms, a.runs, a.iters, warmup=5)
        T = 1 + N // hop
        rec = {"measurement": f"fbank + deltas, B={B} N={N} ({T} frames), {sr} Hz n_fft={n_fft} hop={hop} mels={M}",
               "iters_per_round": a.iters, "max_abs_diff_db": diff,
               # per frame: the DFT as a product over the window, |X|^2, the mel projection
               "flop_per_frame": 2 * win * 2 * K + 3 * K + 2 * K * M,
               # per frame: hop new samples in, the dB frame out and back in, three output rows
               "hbm_bytes_per_frame": 4 * hop + 4 * M + 4 * M + 12 * M}
        for name, v in ms.items():
            rec[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                         "max_ms": round(max(v), 4), "rounds": len(v)}
        rec["frames_per_s_hip"] = round(B * T / (rec["hip_kernels"]["median_ms"] * 1e-3))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
