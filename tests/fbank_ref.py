"""numpy restatement of the feature front end (include/mlvae.h, mlvae_fbank): the pin of the HIP
kernels in float64, and -- run with dtype=float32 on the same tables -- the yardstick of what
fp32 arithmetic costs.  Tables (window, twiddles, mel filters) are always built in float64 and
rounded once to `dtype`, as the library's host fill does; every product, sum, log and division
after that runs in `dtype`.  Also the spoken corpus's nearest-centroid scorer."""
import numpy as np


def geometry(sample_rate, hop_ms, win_ms):
    return int(round(sample_rate / 1000.0 * hop_ms)), int(round(sample_rate / 1000.0 * win_ms))


def window(win, n_fft):
    """Periodic Hamming of `win` points, zero-padded and centred to n_fft (float64)."""
    w = np.zeros(n_fft)
    lo = (n_fft - win) // 2
    w[lo:lo + win] = 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(win) / win)
    return w


def twiddles(win, n_fft):
    """(cos, sin) [n_fft, n_fft/2 + 1] times the window, float64; the angle reduced in integers."""
    n = np.arange(n_fft)[:, None]
    k = np.arange(n_fft // 2 + 1)[None, :]
    ang = 2 * np.pi * ((n * k) % n_fft) / n_fft
    w = window(win, n_fft)[:, None]
    return w * np.cos(ang), w * np.sin(ang)


def mel_filters(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None):
    """[n_fft/2 + 1, n_mels] triangular filters on the HTK mel scale (float64)."""
    f_max = sample_rate / 2 if f_max is None else f_max
    to_mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)
    mel = np.linspace(to_mel(f_min), to_mel(f_max), n_mels + 2)
    hz = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    f_c, band = hz[1:-1], (hz[1:] - hz[:-1])[:-1]
    freqs = np.linspace(0, sample_rate // 2, n_fft // 2 + 1)
    s = (freqs[:, None] - f_c[None, :]) / band[None, :]
    return np.maximum(0.0, np.minimum(s + 1.0, 1.0 - s))


def frames_of(x, hop, n_fft):
    """[T, n_fft] frames of one utterance: T = 1 + N // hop, frame t = samples
    [t hop - n_fft/2, t hop + n_fft/2), zero outside [0, N)."""
    N = x.shape[0]
    T = 1 + N // hop
    pad = np.zeros(N + 2 * n_fft + T * hop, dtype=x.dtype)
    pad[n_fft // 2:n_fft // 2 + N] = x
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return pad[idx]


def power_spectrum(x, hop, win, n_fft, dtype=np.float64):
    c, s = twiddles(win, n_fft)
    fr = frames_of(np.asarray(x).astype(dtype), hop, n_fft)
    re, im = fr @ c.astype(dtype), fr @ s.astype(dtype)
    return re * re + im * im


def deltas(x, dtype=np.float64):
    """d_t = sum_{k=-2..2} k x_{clamp(t+k)} / 10 along axis 0, the edges replicated."""
    T = x.shape[0]
    acc = np.zeros_like(x)
    for k in range(-2, 3):
        acc = acc + dtype(k) * x[np.clip(np.arange(T) + k, 0, T - 1)]
    return acc / dtype(10)


def fbank_utt(x, *, sample_rate=16000, hop_ms=10, win_ms=25, n_fft=400, n_mels=40, f_min=0.0,
              f_max=None, dtype=np.float64):
    """[T, 3 n_mels] (static | delta | delta-delta) of one unpadded utterance."""
    dtype = np.dtype(dtype).type
    hop, win = geometry(sample_rate, hop_ms, win_ms)
    p = power_spectrum(x, hop, win, n_fft, dtype)
    mel = p @ mel_filters(sample_rate, n_fft, n_mels, f_min, f_max).astype(dtype)
    db = dtype(10) * np.log10(np.maximum(mel, dtype(1e-10)))
    db = np.maximum(db, db.max() - dtype(80))
    d = deltas(db, dtype)
    out = np.concatenate([db, d, deltas(d, dtype)], axis=1)
    assert out.dtype == dtype
    return out


def fbank_batch(wav, n_samples, **kw):
    """(feats [B, Tmax, 3 n_mels] zero past each utterance's frames, frames [B]) of a padded
    batch; samples at or past n_samples[b] are not looked at."""
    hop, _ = geometry(kw.get("sample_rate", 16000), kw.get("hop_ms", 10), kw.get("win_ms", 25))
    wav = np.asarray(wav)
    outs = [fbank_utt(wav[b, :int(n)], **kw) for b, n in enumerate(n_samples)]
    Tmax = 1 + wav.shape[1] // hop
    feats = np.zeros((len(outs), Tmax, outs[0].shape[1]), dtype=outs[0].dtype)
    for b, o in enumerate(outs):
        feats[b, :o.shape[0]] = o
    return feats, np.array([o.shape[0] for o in outs], dtype=np.int32)


class RefFbank:
    """The helper behind the compute_features interface (wav [B, N], relative lens) -> torch
    [B, T, 3 n_mels] float32, for building a spoken corpus without the device."""

    def __init__(self, **kw):
        self.kw = kw

    def __call__(self, wav, wav_lens=None):
        import torch
        w = wav.detach().cpu().numpy().astype(np.float64)
        N = w.shape[1]
        lens = np.ones(w.shape[0]) if wav_lens is None else wav_lens.detach().cpu().numpy().astype(np.float64)
        feats, _ = fbank_batch(w, np.round(lens * N).astype(np.int64), **self.kw)
        return torch.from_numpy(feats.astype(np.float32))


def frame_phonemes(e):
    """The pronounced id of every frame of a spoken utterance."""
    seg = np.cumsum(e["gt_boundary_seq"].numpy()).astype(np.int64) - 1
    return e["gt_phn_seq"].numpy()[seg]


def nearest_centroid_accuracy(train_items, test_items, n_static=40):
    """Standardise with the train split's mean and std, one centroid of the static coefficients
    per pronounced id over the train frames, classify every frame of the held-out split."""
    xtr = np.concatenate([e["feat"].numpy()[:, :n_static] for e in train_items]).astype(np.float64)
    ytr = np.concatenate([frame_phonemes(e) for e in train_items])
    xte = np.concatenate([e["feat"].numpy()[:, :n_static] for e in test_items]).astype(np.float64)
    yte = np.concatenate([frame_phonemes(e) for e in test_items])
    mu, sd = xtr.mean(0), xtr.std(0) + 1e-12
    xtr, xte = (xtr - mu) / sd, (xte - mu) / sd
    ids = np.unique(ytr)
    cent = np.stack([xtr[ytr == p].mean(0) for p in ids])
    d = ((xte[:, None, :] - cent[None, :, :]) ** 2).sum(-1)
    return float((ids[d.argmin(1)] == yte).mean())
