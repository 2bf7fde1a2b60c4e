"""numpy restatement of the Kaldi-compatible front end (include/mlvae.h, mlvae_kaldi_fbank and
mlvae_cmvn_*): the pin of the HIP kernels in float64, and -- run with dtype=float32 on the same
tables -- the yardstick of what fp32 arithmetic costs.  What is restated is the documented
behaviour of

    compute-fbank-feats --window-type=hamming --htk-compat=true --dither=0.0 --energy-floor=1.0
                        --snip-edges=false
    add-deltas                      (order 2, window 2)
    compute-cmvn-stats / apply-cmvn --norm-vars=true, per speaker

(ref:src/utils/data_io_utils.py:150-206); no Kaldi binary is among the pinned references, so
parity with Kaldi itself is unpinned.  Tables (window, twiddles, mel filters) are built in float64
and rounded once to `dtype`, as the library's host fill does; every product, sum, log and division
after that runs in `dtype`.  The CMVN statistics are float64 sums whatever `dtype` is."""
import numpy as np

PREEMPH = 0.97
LOW_HZ = 20.0
DD_TAPS = (4, 4, 1, -4, -10, -4, 1, 4, 4)  # [-2..2] convolved with itself, over 100
VAR_FLOOR = 1e-20


def geometry(sample_rate, hop_ms, win_ms):
    """(shift, L, P): frame shift and length in samples, P the power of two at or above L."""
    shift, L = int(round(sample_rate * hop_ms / 1000.0)), int(round(sample_rate * win_ms / 1000.0))
    P = 1
    while P < L:
        P *= 2
    return shift, L, P


def num_frames(N, shift):
    """snip-edges=false: frames are centred on shift f + shift/2, so N samples give
    (N + shift/2) / shift of them."""
    return (int(N) + shift // 2) // shift


def reflect(s, N):
    """The sample index s mirrored at the utterance's ends until it lies in [0, N)."""
    while s < 0 or s >= N:
        s = -s - 1 if s < 0 else 2 * N - 1 - s
    return s


def frame_indices(N, shift, L):
    """[T, L] sample indices: frame f covers shift f + shift/2 - L/2 + i, reflected into [0, N)."""
    T = num_frames(N, shift)
    idx = np.zeros((T, L), dtype=np.int64)
    for f in range(T):
        s0 = shift * f + shift // 2 - L // 2
        for i in range(L):
            idx[f, i] = reflect(s0 + i, N)
    return idx


def hamming(L):
    """Symmetric Hamming window (float64)."""
    return 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(L) / (L - 1)) if L > 1 else np.ones(1)


def preprocess(frames, dtype=np.float64):
    """Per frame: subtract the mean, then pre-emphasis w[i] -= 0.97 w[i-1] for i = L-1 .. 1 and
    w[0] -= 0.97 w[0].  The window is part of the twiddle table."""
    dtype = np.dtype(dtype).type
    w = frames.astype(dtype)
    w = w - w.mean(axis=1, keepdims=True, dtype=dtype)
    prev = np.concatenate([w[:, :1], w[:, :-1]], axis=1)
    out = w - dtype(PREEMPH) * prev
    assert out.dtype == dtype
    return out


def twiddles(L, P):
    """(cos, sin) [L, P/2] times the Hamming window, float64; the angle reduced in integers."""
    n = np.arange(L)[:, None]
    k = np.arange(P // 2)[None, :]
    ang = 2 * np.pi * ((n * k) % P) / P
    w = hamming(L)[:, None]
    return w * np.cos(ang), w * np.sin(ang)


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_edges(sample_rate, n_mels, low=LOW_HZ, high=None):
    """The n_mels + 2 triangle edges on the mel scale."""
    high = sample_rate / 2 if high is None else high
    lo, hi = float(mel(low)), float(mel(high))
    return lo + (hi - lo) / (n_mels + 1) * np.arange(n_mels + 2)


def mel_filters(sample_rate, P, n_mels, low=LOW_HZ, high=None):
    """[P/2, n_mels] triangles: FFT bin i sits at mel(i sample_rate / P); its weight in filter j is
    (m - left)/(centre - left) for left < m <= centre, (right - m)/(right - centre) for
    centre < m < right, else 0 (float64)."""
    e = mel_edges(sample_rate, n_mels, low, high)
    m = mel(np.arange(P // 2) * (sample_rate / P))[:, None]
    left, centre, right = e[None, :-2], e[None, 1:-1], e[None, 2:]
    up = (m - left) / (centre - left)
    down = (right - m) / (right - centre)
    return np.where((m > left) & (m <= centre), up, np.where((m > centre) & (m < right), down, 0.0))


def frames_of(x, shift, L):
    """[T, L] reflected frames of one unpadded utterance."""
    x = np.asarray(x)
    idx = frame_indices(x.shape[0], shift, L)
    return x[idx] if idx.size else np.zeros((0, L), dtype=x.dtype)


def power_of_frames(w, L, P, dtype=np.float64):
    """|X_k|^2, k = 0 .. P/2 - 1, of preprocessed (unwindowed) frames [T, L]."""
    c, s = twiddles(L, P)
    re, im = w @ c.astype(dtype), w @ s.astype(dtype)
    return re * re + im * im


def power_spectrum(x, shift, L, P, dtype=np.float64):
    dtype = np.dtype(dtype).type
    return power_of_frames(preprocess(frames_of(np.asarray(x).astype(dtype), shift, L), dtype), L, P, dtype)


def statics(x, *, sample_rate=16000, hop_ms=20, win_ms=25, n_mels=40, dtype=np.float64):
    """[T, n_mels] ln(max(mel energy, FLT_EPSILON)) of one unpadded utterance."""
    dtype = np.dtype(dtype).type
    shift, L, P = geometry(sample_rate, hop_ms, win_ms)
    p = power_spectrum(x, shift, L, P, dtype)
    e = p @ mel_filters(sample_rate, P, n_mels).astype(dtype)
    out = np.log(np.maximum(e, dtype(np.finfo(np.float32).eps)))
    assert out.dtype == dtype
    return out


def _taps(x, taps, denom, dtype):
    T, half = x.shape[0], len(taps) // 2
    acc = np.zeros_like(x)
    for j, c in zip(range(-half, half + 1), taps):
        acc = acc + dtype(c) * x[np.clip(np.arange(T) + j, 0, T - 1)]
    return acc / dtype(denom)


def delta(x, dtype=np.float64):
    """delta_t = sum_{j=-2..2} j x[clamp(t + j, 0, T-1)] / 10 along axis 0."""
    return _taps(x, (-2, -1, 0, 1, 2), 10, np.dtype(dtype).type)


def delta_delta(x, dtype=np.float64):
    """The convolved 9-tap kernel on the statics at clamped indices (not the 5-tap applied twice:
    the two differ wherever the inner pass's clamp is reached)."""
    return _taps(x, DD_TAPS, 100, np.dtype(dtype).type)


def kaldi_fbank_utt(x, *, deltas=True, dtype=np.float64, **kw):
    """[T, 3 n_mels] (static | delta | delta-delta) of one unpadded utterance ([T, n_mels] with
    deltas=False)."""
    s = statics(x, dtype=dtype, **kw)
    if not deltas:
        return s
    out = np.concatenate([s, delta(s, dtype), delta_delta(s, dtype)], axis=1)
    assert out.dtype == np.dtype(dtype)
    return out


def kaldi_fbank_batch(wav, n_samples, **kw):
    """(feats [B, Tmax, D] zero past each utterance's frames, frames [B]) of a padded batch;
    samples at or past n_samples[b] are not looked at.  Tmax = num_frames(row length)."""
    shift, _, _ = geometry(kw.get("sample_rate", 16000), kw.get("hop_ms", 20), kw.get("win_ms", 25))
    wav = np.asarray(wav)
    outs = [kaldi_fbank_utt(wav[b, :int(n)], **kw) for b, n in enumerate(n_samples)]
    Tmax = num_frames(wav.shape[1], shift)
    feats = np.zeros((len(outs), Tmax, outs[0].shape[1]), dtype=outs[0].dtype)
    for b, o in enumerate(outs):
        feats[b, :o.shape[0]] = o
    return feats, np.array([o.shape[0] for o in outs], dtype=np.int32)


def cmvn_accumulate(stats, feats, frames, spk):
    """Adds one batch's per-speaker sums into stats [S, 2 D + 1] float64 = (sum x | sum x^2 | n):
    per speaker the batch's utterances in row order, their frames in time order, one running
    float64 sum that is then added to the buffer (the kernel's order)."""
    S, D = stats.shape[0], feats.shape[2]
    assert stats.dtype == np.float64 and stats.shape[1] == 2 * D + 1
    for s in range(S):
        sx, sq, n = np.zeros(D), np.zeros(D), 0
        for b in range(feats.shape[0]):
            if int(spk[b]) != s:
                continue
            x = feats[b, :int(frames[b])].astype(np.float64)
            for t in range(x.shape[0]):
                sx = sx + x[t]
                sq = sq + x[t] * x[t]
            n += x.shape[0]
        stats[s, :D] += sx
        stats[s, D:2 * D] += sq
        stats[s, 2 * D] += n
    return stats


def cmvn_moments(stats):
    """(mean, var) [S, D] float64: mean = sum x / n, var = max(sum x^2 / n - mean^2, 1e-20)."""
    D = (stats.shape[1] - 1) // 2
    n = stats[:, 2 * D:]
    mean = stats[:, :D] / n
    return mean, np.maximum(stats[:, D:2 * D] / n - mean * mean, VAR_FLOOR)


def cmvn_apply(feats, frames, spk, stats, dtype=np.float64):
    """y = (x - mean) / sqrt(var) on the valid rows (moments in float64, rounded once to dtype);
    rows past frames[b] stay as they are."""
    dtype = np.dtype(dtype).type
    mean, var = cmvn_moments(stats)
    out = feats.astype(dtype)
    for b in range(feats.shape[0]):
        T, s = int(frames[b]), int(spk[b])
        out[b, :T] = (out[b, :T] - mean[s].astype(dtype)) / np.sqrt(var[s]).astype(dtype)
    assert out.dtype == dtype
    return out


class RefKaldiFbank:
    """The helper behind the KaldiFbank interface: (wav [B, N], relative lens) -> torch
    [B, T, 3 n_mels] float32, for building a corpus without the device."""

    def __init__(self, **kw):
        self.kw = kw

    def __call__(self, wav, wav_lens=None):
        import torch
        w = wav.detach().cpu().numpy().astype(np.float64)
        N = w.shape[1]
        lens = np.ones(w.shape[0]) if wav_lens is None else wav_lens.detach().cpu().numpy().astype(np.float64)
        feats, _ = kaldi_fbank_batch(w, np.round(lens * N).astype(np.int64), **self.kw)
        return torch.from_numpy(feats.astype(np.float32))


class RefSpeakerCMVN:
    """brain.features.SpeakerCMVN on the host (same three methods)."""

    def __init__(self, n_speakers, dim):
        self.n_speakers, self.dim = n_speakers, dim
        self.stats = np.zeros((n_speakers, 2 * dim + 1))

    def reset(self):
        self.stats[:] = 0.0

    def accumulate(self, feats, frames, spk):
        cmvn_accumulate(self.stats, feats.detach().cpu().numpy(), np.asarray(frames), np.asarray(spk))

    def apply(self, feats, frames, spk):
        import torch
        out = cmvn_apply(feats.detach().cpu().numpy().astype(np.float64), np.asarray(frames), np.asarray(spk),
                         self.stats)
        return torch.from_numpy(out.astype(np.float32))
