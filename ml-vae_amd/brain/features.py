"""InputNormalization(norm_type='global') as used by the recipe
(ref:src/models/test_vanilla_vae/model.yaml:14-15, called at model.py:24-25).

SpeechBrain 0.5 semantics restated (parity unpinned): per-utterance mean/std over the first
round(len*T) frames, averaged over the batch; in train mode the global statistics are set on
the first batch and then running-averaged with weight 1/(count+1) while
epoch < update_until_epoch; x <- (x - mean) / std.  Device-side torch ops with no host
synchronisation (outside the fused train step, which takes already normalised features).

Fbank: the reference's compute_features (ref:src/config/run.yaml:39-44), waveform -> log-mel
filterbank + deltas + delta-deltas on the HIP kernels of csrc/fbank.hip.

KaldiFbank and SpeakerCMVN: the reference's `kaldi_feat` (ref:src/utils/data_io_utils.py:150-206),
Kaldi's filterbank + add-deltas and the per-speaker CMVN on the kernels of csrc/kaldi_fbank.hip."""
import torch


class InputNormalization(torch.nn.Module):
    def __init__(self, mean_norm=True, std_norm=True, norm_type="global", avg_factor=None,
                 requires_grad=False, update_until_epoch=3):
        super().__init__()
        if norm_type != "global":
            raise NotImplementedError("only norm_type='global' is used by the VAE recipe")
        self.mean_norm, self.std_norm = mean_norm, std_norm
        self.norm_type = norm_type
        self.avg_factor = avg_factor
        self.update_until_epoch = update_until_epoch
        self.eps = 1e-10
        self.count = 0
        self.register_buffer("glob_mean", torch.zeros(0))
        self.register_buffer("glob_std", torch.zeros(0))

    def _load_from_state_dict(self, state_dict, prefix, *args):
        # the statistics take their shape from the first batch: a checkpoint of a normaliser that
        # has seen data loads into a fresh one (CRDNN_CTC applies and checkpoints its normaliser).
        # The batch count is not part of the state: loaded statistics count as one batch, so the
        # next training batch averages into them instead of replacing them.
        for name in ("glob_mean", "glob_std"):
            v = state_dict.get(prefix + name)
            cur = getattr(self, name)
            if v is not None and v.shape != cur.shape:
                setattr(self, name, torch.zeros(v.shape, dtype=cur.dtype, device=cur.device))
                if v.numel():
                    self.count = max(self.count, 1)
        super()._load_from_state_dict(state_dict, prefix, *args)

    @torch.no_grad()
    def forward(self, x, lengths, spk_ids=None, epoch=0):
        # per-utterance statistics over the first round(len*T) frames, as one masked device
        # reduction (no per-utterance host sync); std is the unbiased torch.std
        B, T = x.shape[0], x.shape[1]
        n = torch.round(lengths.to(x.device, torch.float32) * T)
        mask = (torch.arange(T, device=x.device, dtype=torch.float32).unsqueeze(0) < n.unsqueeze(1))
        mask = mask.to(x.dtype).reshape(B, T, *([1] * (x.dim() - 2)))
        nb = n.to(x.dtype).reshape(B, *([1] * (x.dim() - 2)))
        # zero-length utterances (the fillers of a short data-parallel evaluation slice) carry no
        # statistics: they are left out of the batch averages
        valid = (n > 0).to(x.dtype).reshape(B, *([1] * (x.dim() - 2)))
        nb = nb.clamp(min=1)
        means = (x * mask).sum(1) / nb
        var = (((x - means.unsqueeze(1)) * mask) ** 2).sum(1) / (nb - 1)
        stds = torch.clamp(var.sqrt(), min=self.eps)
        stds = torch.where(valid > 0, stds, torch.zeros_like(stds))  # 0/0 of an empty utterance
        nvalid = valid.sum(0).clamp(min=1)
        cur_mean = (means * valid).sum(0) / nvalid
        cur_std = (stds * valid).sum(0) / nvalid
        from brain.distributed import all_reduce_sum_, world_size
        if self.training and world_size() > 1:  # data parallel: the statistics of the global batch
            acc = torch.cat([(means * valid).sum(0).reshape(-1), (stds * valid).sum(0).reshape(-1),
                             valid.sum().reshape(1)])
            all_reduce_sum_(acc)
            k = cur_mean.numel()
            cur_mean = (acc[:k] / acc[-1]).reshape(cur_mean.shape)
            cur_std = (acc[k:2 * k] / acc[-1]).reshape(cur_std.shape)
        if self.training:
            if self.count == 0:
                self.glob_mean, self.glob_std = cur_mean, cur_std
            elif epoch < self.update_until_epoch:
                w = self.avg_factor if self.avg_factor is not None else 1.0 / (self.count + 1)
                self.glob_mean = (1 - w) * self.glob_mean + w * cur_mean
                self.glob_std = (1 - w) * self.glob_std + w * cur_std
            self.count += 1
        if self.glob_mean.numel() == 0:
            self.glob_mean, self.glob_std = cur_mean, cur_std
        out = x
        if self.mean_norm:
            out = out - self.glob_mean
        if self.std_norm:
            out = out / self.glob_std
        return out


class Fbank(torch.nn.Module):
    """speechbrain.lobes.features.Fbank as the reference configures it (compute_features,
    ref:src/config/run.yaml:39-44; applied per utterance at ref:src/utils/data_io.py:187-214):
    waveform [B, N] -> log-mel filterbank [B, T, n_mels], with deltas and delta-deltas
    [B, T, 3 n_mels] (static | delta | delta-delta), T = 1 + N // hop.  SpeechBrain 0.5's
    constructor names and semantics restated (parity unpinned, include/mlvae.h mlvae_fbank); the
    work is two HIP kernels (mlvae_hip.ops.fbank), per utterance: with wav_lens (relative,
    N_b = round(N len_b)) an utterance's frames, its 80 dB floor and its delta edges are those of
    the unpadded waveform, and the rows past 1 + N_b // hop are zeros.  hop_length / win_length in
    milliseconds.  Constructing it touches neither the device nor a random generator."""

    def __init__(self, deltas=False, context=False, requires_grad=False, sample_rate=16000, f_min=0,
                 f_max=None, n_fft=400, n_mels=40, filter_shape="triangular", left_frames=5,
                 right_frames=5, win_length=25, hop_length=10):
        super().__init__()
        if context:
            raise NotImplementedError("Fbank(context=True): context windows are not built (no recipe "
                                      "of the reference uses them)")
        if requires_grad:
            raise NotImplementedError("Fbank(requires_grad=True): the filterbank is a fixed table of "
                                      "the kernels; learnable filters need a backward that is not built")
        if filter_shape != "triangular":
            raise NotImplementedError(f"Fbank(filter_shape={filter_shape!r}): the kernels' filter table "
                                      "holds triangular filters only")
        self.deltas, self.context = bool(deltas), False
        self.sample_rate, self.n_fft, self.n_mels = int(sample_rate), int(n_fft), int(n_mels)
        self.f_min = float(f_min)
        self.f_max = float(sample_rate / 2 if f_max is None else f_max)
        self.filter_shape = filter_shape
        self.left_frames, self.right_frames = left_frames, right_frames
        self.win_length, self.hop_length = win_length, hop_length

    @torch.no_grad()
    def forward(self, wav, wav_lens=None):
        from mlvae_hip import ops
        if wav_lens is not None:
            wav_lens = torch.as_tensor(wav_lens, dtype=torch.float32)
        feats, _ = ops.fbank(wav, wav_lens, sample_rate=self.sample_rate, hop_length=self.hop_length,
                             win_length=self.win_length, n_fft=self.n_fft, n_mels=self.n_mels,
                             f_min=self.f_min, f_max=self.f_max)
        return feats if self.deltas else feats[..., :self.n_mels]


class KaldiFbank(torch.nn.Module):
    """What the reference's Kaldi binaries compute before CMVN (kaldi_feature_params of
    ref:src/config/run.yaml, run by ref:src/utils/data_io_utils.py:150-206): compute-fbank-feats
    --window-type=hamming --htk-compat=true --dither=0.0 --energy-floor=1.0 --snip-edges=false and
    add-deltas, waveform [B, N] -> [B, T, 3 n_mels] (static | delta | delta-delta; [B, T, n_mels]
    with deltas=False), T = (N + hop/2) // hop.  The constructor keys are the reference's:
    hop_length in milliseconds, n_fft the frame length in samples (the frame length is
    n_fft / sample_rate, ref:src/utils/data_io_utils.py:161).  Kaldi's documented behaviour restated
    (parity with Kaldi unpinned, include/mlvae.h mlvae_kaldi_fbank); the work is two HIP kernels
    (mlvae_hip.ops.kaldi_fbank), per utterance as in Fbank: with wav_lens (relative,
    N_b = round(N len_b)) the mirrored edges and the delta edges are those of the unpadded waveform
    and the rows past (N_b + hop/2) // hop are zeros.  The per-speaker normalisation is SpeakerCMVN.
    Constructing it touches neither the device nor a random generator."""

    def __init__(self, sample_rate=16000, hop_length=20, n_fft=400, n_mels=40, deltas=True):
        super().__init__()
        self.sample_rate, self.n_fft, self.n_mels = int(sample_rate), int(n_fft), int(n_mels)
        self.hop_length = hop_length
        self.win_length = 1000.0 * self.n_fft / self.sample_rate  # milliseconds
        self.deltas = bool(deltas)

    def frames(self, n_samples):
        """Frames of an utterance of n_samples samples."""
        hop = int(round(self.sample_rate / 1000.0 * self.hop_length))
        return (int(n_samples) + hop // 2) // hop

    @torch.no_grad()
    def forward(self, wav, wav_lens=None):
        from mlvae_hip import ops
        if wav_lens is not None:
            wav_lens = torch.as_tensor(wav_lens, dtype=torch.float32)
        feats, _ = ops.kaldi_fbank(wav, wav_lens, sample_rate=self.sample_rate, hop_length=self.hop_length,
                                   win_length=self.win_length, n_mels=self.n_mels, deltas=self.deltas)
        return feats


class SpeakerCMVN:
    """Kaldi's per-speaker compute-cmvn-stats + apply-cmvn --norm-vars=true over one split: holds
    the float64 statistics [n_speakers, 2 dim + 1] = (sum x | sum x^2 | n) on the device.
    accumulate(feats [B, T, dim], frames [B], spk [B]) adds a batch's valid rows (fixed order: a
    rerun is bit-identical); apply(...) normalises the valid rows in place with each utterance's
    speaker's mean and variance (floored at 1e-20) and returns feats; reset() zeroes the
    statistics.  The buffer is created on the first batch's device."""

    def __init__(self, n_speakers, dim):
        self.n_speakers, self.dim = int(n_speakers), int(dim)
        if self.n_speakers < 1 or self.dim < 1:
            raise ValueError("SpeakerCMVN: n_speakers and dim must be >= 1")
        self.stats = None

    def _buffer(self, dev):
        if self.stats is None or self.stats.device != dev:
            self.stats = torch.zeros(self.n_speakers, 2 * self.dim + 1, device=dev, dtype=torch.float64)
        return self.stats

    def reset(self):
        if self.stats is not None:
            self.stats.zero_()

    @torch.no_grad()
    def accumulate(self, feats, frames, spk):
        from mlvae_hip import ops
        ops.cmvn_accumulate(self._buffer(feats.device), feats, frames, spk)

    @torch.no_grad()
    def apply(self, feats, frames, spk):
        from mlvae_hip import ops
        return ops.cmvn_apply(feats, frames, spk, self._buffer(feats.device))
