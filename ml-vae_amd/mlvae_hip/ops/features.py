"""The feature front ends: Fbank, Kaldi-compatible Fbank and per-speaker CMVN (csrc/fbank.hip,
csrc/kaldi_fbank.hip)."""
import torch

from .._lib import check, lib
from ._core import _need, _p, raise_err, _stream, _workspace, _ws_bytes


# ---- the feature front end (csrc/fbank.hip)
_fbank_tables = {}


def _fbank_table(dev, sample_rate, win, n_fft, n_mels, f_min, f_max):
    """The windowed twiddles and mel filters of one geometry on one device: filled once on the host
    (mlvae_fbank_table, float64 rounded to fp32) and kept."""
    key = (dev, sample_rate, win, n_fft, n_mels, float(f_min), float(f_max))
    t = _fbank_tables.get(key)
    if t is None:
        nbytes = lib().mlvae_fbank_table_size(win, n_fft, n_mels)
        if nbytes == 0:
            check(1, "fbank")
        host = torch.empty(nbytes // 4, dtype=torch.float32)
        check(lib().mlvae_fbank_table(sample_rate, win, n_fft, n_mels, float(f_min), float(f_max),
                                      host.data_ptr(), nbytes), "fbank_table")
        t = _fbank_tables[key] = host.to(dev)
    return t


def fbank(wav, wav_lens=None, *, sample_rate=16000, hop_length=10, win_length=25, n_fft=400, n_mels=40,
          f_min=0.0, f_max=None):
    """(feats [B, Tmax, 3 n_mels] fp32, frames [B] int32) of the padded waveforms wav [B, N]:
    log-mel filterbank, deltas and delta-deltas as SpeechBrain's Fbank(deltas=True) computes them
    per utterance (include/mlvae.h, mlvae_fbank), Tmax = 1 + N // hop, rows past an utterance's
    frames[b] = 1 + N_b // hop exact zeros.  wav_lens: None (every row N samples), an integer
    tensor of sample counts N_b, or a floating tensor of relative lengths (N_b = round(N len_b));
    samples at or past N_b are never read.  hop_length / win_length in milliseconds.  No autograd:
    the front end has no parameters; an input that requires grad raises."""
    if wav.dim() != 2:
        raise ValueError(f"fbank: wav must be [B, N], got {tuple(wav.shape)}")
    if wav.requires_grad:
        raise RuntimeError("fbank: the front end has no backward; detach the waveform")
    wav = _need(wav, "fbank wav")
    B, N = wav.shape
    dev = wav.device
    sample_rate, n_fft, n_mels = int(sample_rate), int(n_fft), int(n_mels)
    # samples from SpeechBrain's milliseconds
    hop, win = (int(round(sample_rate / 1000.0 * ms)) for ms in (hop_length, win_length))
    f_max = sample_rate / 2 if f_max is None else f_max
    if wav_lens is None:
        ns = torch.full((B,), N, device=dev, dtype=torch.int32)
    else:
        wav_lens = torch.as_tensor(wav_lens)
        if tuple(wav_lens.shape) != (B,):
            raise ValueError(f"fbank: wav_lens must be [{B}], got {tuple(wav_lens.shape)}")
        if wav_lens.is_floating_point():
            ns = torch.round(wav_lens.to(dev, torch.float64) * N).to(torch.int32)
        else:
            ns = wav_lens.to(dev, torch.int32)
        ns = ns.contiguous()
    # geometry errors come from the library (status 1 with its message)
    table = _fbank_table(dev, sample_rate, win, n_fft, n_mels, f_min, f_max)
    Tmax = 1 + N // max(hop, 1)
    feats = torch.empty(B, Tmax, 3 * n_mels, device=dev, dtype=torch.float32)
    frames = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        ws = _workspace(lib().mlvae_fbank_workspace_size(B, N, hop, n_mels), "fbank")
        check(lib().mlvae_fbank(B, N, _p(wav) if N else None, N, ns.data_ptr(), hop, win, n_fft, n_mels,
                                _p(table), _p(feats), 3 * n_mels, frames.data_ptr(), _p(ws),
                                _ws_bytes(ws), _stream()), "fbank")
    return feats, frames


# ---- the Kaldi-compatible front end and per-speaker CMVN (csrc/kaldi_fbank.hip)
_kaldi_tables = {}


def _kaldi_table(dev, sample_rate, L, P, n_mels):
    """The Hamming-windowed twiddles and mel filters of one geometry on one device: filled once on
    the host (mlvae_kaldi_fbank_table, float64 rounded to fp32) and kept."""
    key = (dev, sample_rate, L, P, n_mels)
    t = _kaldi_tables.get(key)
    if t is None:
        nbytes = lib().mlvae_kaldi_fbank_table_size(L, P, n_mels)
        if nbytes == 0:
            check(1, "kaldi_fbank")
        host = torch.empty(nbytes // 4, dtype=torch.float32)
        check(lib().mlvae_kaldi_fbank_table(sample_rate, L, P, n_mels, host.data_ptr(), nbytes),
              "kaldi_fbank_table")
        t = _kaldi_tables[key] = host.to(dev)
    return t


def kaldi_fbank(wav, wav_lens=None, *, sample_rate=16000, hop_length=20, win_length=25, n_mels=40,
                deltas=True):
    """(feats [B, Tmax, 3 n_mels] fp32, frames [B] int32) of the padded waveforms wav [B, N]: Kaldi's
    compute-fbank-feats (Hamming, snip-edges=false, no dither) + add-deltas as restated in
    include/mlvae.h (mlvae_kaldi_fbank), before CMVN.  Tmax = (N + hop/2) // hop, rows past an
    utterance's frames[b] = (N_b + hop/2) // hop exact zeros; deltas=False gives the n_mels statics.
    wav_lens as ops.fbank: None (every row N samples), an integer tensor of sample counts N_b, or a
    floating tensor of relative lengths (N_b = round(N len_b)); samples at or past N_b are never
    read.  hop_length / win_length in milliseconds.  No autograd: an input that requires grad
    raises."""
    if wav.dim() != 2:
        raise ValueError(f"kaldi_fbank: wav must be [B, N], got {tuple(wav.shape)}")
    if wav.requires_grad:
        raise RuntimeError("kaldi_fbank: the front end has no backward; detach the waveform")
    wav = _need(wav, "kaldi_fbank wav")
    B, N = wav.shape
    dev = wav.device
    sample_rate, n_mels = int(sample_rate), int(n_mels)
    hop, L = (int(round(sample_rate / 1000.0 * ms)) for ms in (hop_length, win_length))
    P = 1 << max(L - 1, 0).bit_length()  # the power of two at or above L
    if wav_lens is None:
        ns = torch.full((B,), N, device=dev, dtype=torch.int32)
    else:
        wav_lens = torch.as_tensor(wav_lens)
        if tuple(wav_lens.shape) != (B,):
            raise ValueError(f"kaldi_fbank: wav_lens must be [{B}], got {tuple(wav_lens.shape)}")
        if wav_lens.is_floating_point():
            ns = torch.round(wav_lens.to(dev, torch.float64) * N).to(torch.int32)
        else:
            ns = wav_lens.to(dev, torch.int32)
        ns = ns.contiguous()
    # geometry errors come from the library (status 1 with its message)
    table = _kaldi_table(dev, sample_rate, L, P, n_mels)
    Tmax = (N + hop // 2) // max(hop, 1)
    D = (3 if deltas else 1) * n_mels
    feats = torch.empty(B, Tmax, D, device=dev, dtype=torch.float32)
    frames = torch.empty(B, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        ws = _workspace(lib().mlvae_kaldi_fbank_workspace_size(B, N, hop, n_mels), "kaldi_fbank")
        check(lib().mlvae_kaldi_fbank(B, N, _p(wav) if N else None, N, ns.data_ptr(), hop, L, P, n_mels,
                                      int(bool(deltas)), _p(table), _p(feats) if Tmax else None, D,
                                      frames.data_ptr(), _p(ws), _ws_bytes(ws), _stream()), "kaldi_fbank")
    return feats, frames


def _cmvn_args(feats, frames, spk, stats, who):
    if feats.dim() != 3:
        raise ValueError(f"{who}: feats must be [B, T, D], got {tuple(feats.shape)}")
    if not (feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous()):
        raise TypeError(f"{who}: feats must be a contiguous float32 HIP tensor "
                        "(the HIP path has no CPU fallback)")
    B, T, D = feats.shape
    if not (stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous() and
            stats.dim() == 2 and stats.shape[1] == 2 * D + 1):
        raise TypeError(f"{who}: stats must be a contiguous float64 HIP tensor [S, {2 * D + 1}]")
    dev = feats.device
    frames = torch.as_tensor(frames).to(dev, torch.int32).contiguous()
    spk = torch.as_tensor(spk).to(dev, torch.int32).contiguous()
    if tuple(frames.shape) != (B,) or tuple(spk.shape) != (B,):
        raise ValueError(f"{who}: frames and spk must be [{B}]")
    return B, T, D, stats.shape[0], frames, spk


def _raise_cmvn(err, who):
    raise_err(err, "cmvn", who)  # one host sync: corpus preparation, not the training step


def cmvn_accumulate(stats, feats, frames, spk):
    """Adds the batch's per-speaker (sum x | sum x^2 | n) over the rows t < frames[b] of feats
    [B, T, D] into stats [S, 2 D + 1] float64, in place (include/mlvae.h, mlvae_cmvn_accumulate):
    a fixed accumulation order, so a rerun is bit-identical.  A speaker id outside [0, S) raises
    ValueError (that utterance is not accumulated)."""
    B, T, D, S, frames, spk = _cmvn_args(feats, frames, spk, stats, "cmvn_accumulate")
    err = torch.zeros(1, device=feats.device, dtype=torch.int32)
    with torch.cuda.device(feats.device):
        check(lib().mlvae_cmvn_accumulate(B, T, D, S, _p(feats) if feats.numel() else None, D,
                                          frames.data_ptr(), spk.data_ptr(), stats.data_ptr(),
                                          err.data_ptr(), _stream()), "cmvn_accumulate")
    if B:
        _raise_cmvn(err, "cmvn_accumulate")
    return stats


def cmvn_apply(feats, frames, spk, stats):
    """y = (x - mean) / sqrt(var) of the speaker's statistics on the rows t < frames[b] of feats
    [B, T, D], in place (mean = sum x / n, var = max(sum x^2 / n - mean^2, 1e-20)); rows past
    frames[b] are not touched.  Returns feats."""
    B, T, D, S, frames, spk = _cmvn_args(feats, frames, spk, stats, "cmvn_apply")
    err = torch.zeros(1, device=feats.device, dtype=torch.int32)
    with torch.cuda.device(feats.device):
        check(lib().mlvae_cmvn_apply(B, T, D, S, _p(feats) if feats.numel() else None, D,
                                     frames.data_ptr(), spk.data_ptr(), stats.data_ptr(),
                                     err.data_ptr(), _stream()), "cmvn_apply")
    if B and T:
        _raise_cmvn(err, "cmvn_apply")
    return feats
