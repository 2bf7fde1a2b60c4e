"""The Kaldi-compatible front end's float64 pin (tests/kaldi_fbank_ref.py) by properties that need
no Kaldi, the host table of the library, the config's entries, the corpus option and the
MD_VAE_sfl hook -- all without a device."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import PKG
import fbank_ref as F
import kaldi_fbank_ref as R
from utils.data_io import SyntheticSet

SHIFT, L, P = 320, 400, 512
GEO = dict(sample_rate=16000, hop_ms=20, win_ms=25, n_mels=40)


def _noise(N, seed=0):
    return np.random.default_rng(seed).standard_normal(N)


# --------------------------------------------------------------------------- frames
def test_geometry_and_frame_counts():
    assert R.geometry(16000, 20, 25) == (SHIFT, L, P)
    assert R.geometry(8000, 10, 25) == (80, 200, 256)
    want = {0: 0, 159: 0, 160: 1, 479: 1, 480: 2}
    for k in (1, 2, 7, 33):
        want.update({320 * k - 1: k, 320 * k: k, 320 * k + 1: k})
    for N, T in want.items():
        assert R.num_frames(N, SHIFT) == T, N
        assert R.frames_of(_noise(N), SHIFT, L).shape == (T, L)
        assert R.kaldi_fbank_utt(_noise(N), **GEO).shape == (T, 120)


@pytest.mark.parametrize("N", [100, 160, 479, 5 * 320 + 7])
def test_first_and_last_frame_are_the_mirrored_waveform(N):
    """Against an explicitly mirrored array: x | reversed x | x | ... in both directions (N = 100
    is shorter than the window: its one frame is reflected more than once)."""
    x = np.arange(N, dtype=np.float64) + 0.25
    reps = L // N + 2
    period = np.concatenate([x, x[::-1]])
    mirrored = np.tile(period, 2 * reps)  # index j holds the sample at j - 2 N reps
    origin = 2 * N * reps
    # N = 100 has no frame at a 320-sample shift (100 < 160): its frame is the 10 ms shift's
    shift = 160 if N == 100 else SHIFT
    fr = R.frames_of(x, shift, L)
    T = R.num_frames(N, shift)
    assert T >= 1 and fr.shape == (T, L)
    for f in (0, T - 1):
        s0 = shift * f + shift // 2 - L // 2
        assert s0 < 0 or s0 + L > N  # an edge is reached
        assert np.array_equal(fr[f], mirrored[origin + s0:origin + s0 + L]), f
    if N == 100:  # the map itself, over a window's reach on both sides
        for s in range(-L, L):
            assert x[R.reflect(s, N)] == mirrored[origin + s]
        assert R.reflect(-101, N) == 99 and R.reflect(-201, N) == 0 and R.reflect(250, N) == 50
        assert R.num_frames(N, SHIFT) == 0


def test_padding_is_not_read():
    x = _noise(1000, 1)
    wav = np.full((2, 1500), np.nan)
    wav[0, :1000] = x
    wav[1] = _noise(1500, 2)
    feats, frames = R.kaldi_fbank_batch(wav, [1000, 1500], **GEO)
    assert list(frames) == [3, 5] and feats.shape == (2, 5, 120)
    assert np.isfinite(feats).all() and not feats[0, 3:].any()
    assert np.array_equal(feats[0, :3], R.kaldi_fbank_utt(x, **GEO))


# --------------------------------------------------------------------------- preprocessing, DFT
def test_dc_invariance():
    x = 0.1 * _noise(3000, 3)
    a = R.kaldi_fbank_utt(x, **GEO)
    b = R.kaldi_fbank_utt(x + 0.37, **GEO)
    err = np.abs(a - b).max()
    print(f"max |features(x + c) - features(x)| {err:.2e}")
    assert err <= 1e-9


def test_preemphasis_order():
    w = np.array([[1.0, 2.0, 4.0, 8.0]])
    w0 = w - w.mean()
    got = R.preprocess(w)
    want = w0.copy()
    for i in range(3, 0, -1):
        want[0, i] -= 0.97 * want[0, i - 1]
    want[0, 0] -= 0.97 * want[0, 0]
    assert np.allclose(got, want, rtol=0, atol=1e-15)


def test_power_spectrum_equals_rfft():
    x = _noise(2000, 4)
    w = R.preprocess(R.frames_of(x, SHIFT, L))
    got = R.power_of_frames(w, L, P)
    spec = np.fft.rfft(w * R.hamming(L)[None, :], P, axis=1)[:, :P // 2]
    want = spec.real ** 2 + spec.imag ** 2
    assert got.shape == want.shape == (6, 256)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"max |power - rfft| relative to the largest bin {err:.2e}")
    assert err <= 1e-12
    h = R.hamming(L)
    assert np.allclose(h, h[::-1]) and abs(h[0] - 0.08) < 1e-12  # symmetric, L - 1 in the cosine


# --------------------------------------------------------------------------- mel filters
@pytest.mark.parametrize("sr,P_,M", [(16000, 512, 40), (8000, 256, 23), (16000, 512, 64)])
def test_mel_filters(sr, P_, M):
    fb = R.mel_filters(sr, P_, M)
    assert fb.shape == (P_ // 2, M) and (fb >= 0).all() and (fb <= 1).all()
    hz = np.arange(P_ // 2) * sr / P_
    assert not fb[hz <= 20.0].any() and not fb[0].any()
    assert ((fb > 0).sum(1) <= 2).all()
    assert (fb.sum(1) <= 1 + 1e-12).all()
    e = R.mel_edges(sr, M)
    m = R.mel(hz)
    between = (m >= e[1]) & (m <= e[-2])  # from the first centre to the last: two slopes that add to 1
    assert between.sum() > P_ // 4 and np.allclose(fb[between].sum(1), 1.0, atol=1e-12)
    assert (fb.sum(0) > 0).all()  # every filter holds a bin
    assert abs(float(R.mel(1000.0)) - 1127.0 * np.log(1 + 1000 / 700)) < 1e-12


def test_a_tone_peaks_in_its_filter():
    n = np.arange(16000)
    s = R.statics(np.sin(2 * np.pi * 1000.0 * n / 16000), **GEO)
    centres = R.mel_edges(16000, 40)[1:-1]
    want = int(np.abs(centres - float(R.mel(1000.0))).argmin())
    assert (s[2:-2].argmax(1) == want).all()


def test_statics_floor_is_flt_epsilon():
    s = R.statics(np.zeros(1000), **GEO)
    assert s.shape == (3, 40) and np.all(s == np.log(np.float64(np.finfo(np.float32).eps)))


# --------------------------------------------------------------------------- deltas
def test_deltas_of_a_ramp():
    t = np.arange(20, dtype=np.float64)[:, None]
    x = 3.0 + 0.5 * t * np.array([[1.0, -2.0]])
    d, dd = R.delta(x), R.delta_delta(x)
    assert np.allclose(d[2:-2], 0.5 * np.array([[1.0, -2.0]]), atol=1e-12)
    assert np.allclose(dd[4:-4], 0.0, atol=1e-12)
    assert sum(R.DD_TAPS) == 0
    five = np.array([-2, -1, 0, 1, 2])
    assert list(np.convolve(five, five)) == list(R.DD_TAPS)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
def test_delta_delta_is_the_nine_taps_on_the_statics(T):
    """From T = 2 the 9-tap kernel at clamped indices differs from the 5-tap pass applied twice
    (whose inner pass clamps first).  At T = 1 every index clamps to the one frame and both sets
    of taps sum to zero, so both are zero there: nothing to tell apart."""
    x = np.random.default_rng(T).standard_normal((T, 3))
    nine = R.delta_delta(x)
    twice = R.delta(R.delta(x))
    idx = np.clip(np.arange(T)[:, None] + np.arange(-4, 5)[None, :], 0, T - 1)
    want = (x[idx] * (np.array(R.DD_TAPS) / 100.0)[None, :, None]).sum(1)
    assert np.allclose(nine, want, atol=1e-14)
    if T == 1:
        assert np.abs(nine).max() < 1e-15 and np.abs(twice).max() < 1e-15
    else:
        assert np.abs(nine - twice).max() > 1e-3
    full = R.kaldi_fbank_utt(_noise(320 * T, T), **GEO)
    assert full.shape == (T, 120)
    assert np.array_equal(full[:, 80:], R.delta_delta(full[:, :40]))
    assert np.array_equal(full[:, 40:80], R.delta(full[:, :40]))


def test_float32_mode_runs_in_float32():
    x = _noise(2000, 6).astype(np.float32)
    a = R.kaldi_fbank_utt(x, dtype=np.float32, **GEO)
    b = R.kaldi_fbank_utt(x.astype(np.float64), dtype=np.float64, **GEO)
    assert a.dtype == np.float32 and b.dtype == np.float64
    assert 0 < np.abs(a - b).max() < 1e-3


# --------------------------------------------------------------------------- CMVN
def test_cmvn_moments_per_speaker():
    g = np.random.default_rng(7)
    feats = (3.0 + 2.0 * g.standard_normal((5, 9, 4))) * np.array([1.0, 10.0, 0.1, 1.0])
    feats[..., 3] = 2.5  # a constant column: the variance floor
    frames = np.array([9, 4, 7, 0, 9])
    spk = np.array([0, 1, 0, 1, 2])
    for b, T in enumerate(frames):
        feats[b, T:] = 0.0
    stats = np.zeros((3, 9))
    R.cmvn_accumulate(stats, feats[:3], frames[:3], spk[:3])
    R.cmvn_accumulate(stats, feats[3:], frames[3:], spk[3:])
    assert list(stats[:, 8]) == [16.0, 4.0, 9.0]
    out = R.cmvn_apply(feats, frames, spk, stats)
    assert np.isfinite(out).all()
    for s in range(3):
        rows = np.concatenate([out[b, :frames[b]] for b in range(5) if spk[b] == s])
        assert np.allclose(rows[:, :3].mean(0), 0.0, atol=1e-12)
        assert np.allclose(rows[:, :3].var(0), 1.0, atol=1e-9)
        assert not rows[:, 3].any()  # (x - mean) = 0 over the floored deviation
    _, var = R.cmvn_moments(stats)
    assert np.all(var[:, 3] == R.VAR_FLOOR)
    for b, T in enumerate(frames):
        assert not out[b, T:].any()


# --------------------------------------------------------------------------- the library's table
@pytest.mark.parametrize("sr,L_,M", [(16000, 400, 40), (8000, 200, 23), (16000, 400, 64), (16000, 399, 40)])
def test_library_table_is_the_helpers(sr, L_, M):
    """mlvae_kaldi_fbank_table is host code: the windowed twiddles and filters it fills are the
    helper's float64 ones rounded to fp32, in the kernel's layout (rows = frame samples, 32 re |
    32 im columns per bin tile, then the [bins, 64] filters)."""
    from mlvae_hip import _lib
    l = _lib.lib()
    P_ = 1 << (L_ - 1).bit_length()
    K, wr = P_ // 2, (L_ + 1) // 2 * 2
    nbt = (K + 31) // 32
    nbytes = l.mlvae_kaldi_fbank_table_size(L_, P_, M)
    assert nbytes == 4 * (wr * nbt * 64 + K * 64)
    tab = np.full(nbytes // 4, np.nan, dtype=np.float32)
    assert l.mlvae_kaldi_fbank_table(sr, L_, P_, M, tab.ctypes.data, nbytes) == 0
    c, s = R.twiddles(L_, P_)
    dft = tab[:wr * nbt * 64].reshape(wr, nbt, 2, 32)
    re = dft[:, :, 0, :].reshape(wr, nbt * 32)
    im = dft[:, :, 1, :].reshape(wr, nbt * 32)
    # two libms' float64 cosines may round to neighbouring fp32 values (|entries| <= 1)
    assert np.abs(re[:L_, :K] - c.astype(np.float32)).max() <= 1.2e-7
    assert np.abs(im[:L_, :K] - s.astype(np.float32)).max() <= 1.2e-7
    assert not re[L_:].any() and not im[L_:].any()
    fb = tab[wr * nbt * 64:].reshape(K, 64)
    assert np.abs(fb[:, :M] - R.mel_filters(sr, P_, M).astype(np.float32)).max() <= 1e-6
    assert not fb[:, M:].any()
    for bad, word in (((L_, 384, M), "power of two"), ((L_, 1024, M), "512"), ((P_ + 1, P_, M), "window"),
                      ((L_, P_, 65), "n_mels")):
        assert l.mlvae_kaldi_fbank_table_size(*bad) == 0 and word in _lib.last_error(), bad
    assert l.mlvae_kaldi_fbank_table(sr, L_, P_, M, tab.ctypes.data, nbytes - 4) == 1


# --------------------------------------------------------------------------- module and config
def test_module_constructor_surface():
    from brain.features import KaldiFbank, SpeakerCMVN
    torch.manual_seed(11)
    before = torch.get_rng_state()
    k = KaldiFbank()
    c = SpeakerCMVN(4, 120)
    assert torch.equal(torch.get_rng_state(), before)
    assert (k.sample_rate, k.hop_length, k.n_fft, k.n_mels, k.deltas) == (16000, 20, 400, 40, True)
    assert k.win_length == 25.0 and k.frames(320 * 7) == 7 and k.frames(159) == 0
    assert not list(k.parameters()) and not list(k.buffers())
    assert c.stats is None  # the device buffer comes with the first batch
    c.reset()
    k8 = KaldiFbank(sample_rate=8000, hop_length=10, n_fft=200, n_mels=23, deltas=False)
    assert k8.win_length == 25.0 and not k8.deltas
    with pytest.raises(ValueError, match="n_speakers"):
        SpeakerCMVN(0, 120)
    with pytest.raises(TypeError, match="HIP tensor"):
        k(torch.zeros(1, 640))
    with pytest.raises(TypeError, match="HIP tensor"):
        from mlvae_hip import ops
        ops.cmvn_accumulate(torch.zeros(2, 7, dtype=torch.float64), torch.zeros(1, 2, 3), [2], [0])


def test_config_gives_the_reference_kaldi_front_end():
    from brain.features import KaldiFbank
    from hyperpyyaml import load_hyperpyyaml
    ov = ("dataset: synthetic\nmodel_class: MD_VAE_sfl\nmodel_name: m\n"
          "model: !include:../models/MD_VAE_sfl/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{"model": {"n_epochs": 1}}, ov])
    assert hp["kaldi_feature_params"] == {"sample_rate": 16000, "hop_length": 20, "n_fft": 400, "n_mels": 40}
    k = hp["compute_kaldi_features"]
    assert isinstance(k, KaldiFbank)
    assert (k.sample_rate, k.hop_length, k.n_fft, k.n_mels, k.deltas) == (16000, 20, 400, 40, True)
    assert hp["synthetic"]["kaldi_feats"] is False and hp["synthetic"]["n_speakers"] == 4
    assert "use_kaldi_feat" not in hp["model"]
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{"model": {"use_kaldi_feat": True}, "synthetic": {"kaldi_feats": True}}, ov])
    assert hp["model"]["use_kaldi_feat"] is True and hp["synthetic"]["kaldi_feats"] is True


# --------------------------------------------------------------------------- the corpus
def _corpus(**kw):
    ref = F.RefFbank(sample_rate=16000, hop_ms=20, win_ms=25, n_fft=400, n_mels=40)
    base = dict(md_labels=True, n_phonemes=39, phn_labels=True, ali_labels=True, waveforms=True,
                compute_features=ref)
    base.update(kw)
    return SyntheticSet(6, 120, 30, 60, 77, **base)


def test_corpus_adds_kaldi_feat_and_spk_only():
    spoken = _corpus()
    kaldi = _corpus(kaldi_feats=True, n_speakers=4, compute_kaldi_features=R.RefKaldiFbank(**GEO),
                    speaker_cmvn=R.RefSpeakerCMVN(4, 120))
    by_id = {e["id"]: e for e in kaldi.items}
    assert [e["id"] for e in kaldi.items] == [e["id"] for e in spoken.items]
    for e in spoken.items:
        k = by_id[e["id"]]
        assert set(k) == set(e) | {"kaldi_feat", "spk"}
        for key, v in e.items():
            assert torch.equal(k[key], v) if torch.is_tensor(v) else k[key] == v, key
        T = e["feat"].shape[0]
        assert k["kaldi_feat"].shape == (T, 120) and k["kaldi_feat"].dtype == torch.float32
        assert k["spk"] == int(e["id"][3:]) % 4
        assert torch.isfinite(k["kaldi_feat"]).all()
    # per speaker: mean 0, variance 1 over the split, to float32 storage
    for s in range(4):
        rows = torch.cat([e["kaldi_feat"] for e in kaldi.items if e["spk"] == s]).double()
        assert rows.mean(0).abs().max() < 1e-5 and (rows.var(0, unbiased=False) - 1).abs().max() < 1e-4
    # the raw features are the helper's, normalised by the helper's per-speaker statistics
    e = by_id["utt00005"]
    mates = [by_id["utt00001"], e]
    raw = [R.kaldi_fbank_utt(m["wav"].numpy().astype(np.float64), **GEO) for m in mates]
    allr = np.concatenate(raw)
    want = (raw[1] - allr.mean(0)) / allr.std(0)
    assert np.abs(e["kaldi_feat"].numpy() - want).max() < 1e-5
    batch = next(iter(kaldi.batches(batch_size=3)))
    assert batch["kaldi_feat"][0].shape[2] == 120 and len(batch["spk"]) == 3
    assert torch.equal(batch["kaldi_feat"][1], batch["feat"][1])


def test_corpus_option_errors():
    with pytest.raises(ValueError, match="waveforms"):
        SyntheticSet(2, 120, 30, 40, 1, md_labels=True, kaldi_feats=True,
                     compute_kaldi_features=R.RefKaldiFbank(**GEO))
    with pytest.raises(ValueError, match="compute_kaldi_features"):
        _corpus(kaldi_feats=True)
    with pytest.raises(ValueError, match="n_speakers"):
        _corpus(kaldi_feats=True, n_speakers=0, compute_kaldi_features=R.RefKaldiFbank(**GEO))
    with pytest.raises(ValueError, match="hop_length"):  # 10 ms frames: twice the labels' frames
        _corpus(kaldi_feats=True, compute_kaldi_features=R.RefKaldiFbank(**dict(GEO, hop_ms=10)),
                speaker_cmvn=R.RefSpeakerCMVN(4, 120))


# --------------------------------------------------------------------------- the MD_VAE_sfl hook
class _Spy:
    calls = 0

    def __call__(self, feats, lens, epoch=None):
        self.calls += 1
        return feats + 1.0


def _hook_model(**hp):
    from models.MD_VAE_sfl.model import SBModel
    spy = _Spy()
    m = SBModel(modules={}, hparams=dict(normalizer=spy, epoch_counter=types.SimpleNamespace(current=1),
                                         metric_keys=[], **hp), run_opts={"device": "cpu"})
    return m, spy


def test_md_vae_sfl_reads_kaldi_feat_and_skips_the_normaliser():
    feat = (torch.zeros(2, 5, 3), torch.ones(2))
    kaldi = (torch.full((2, 5, 3), 7.0), torch.tensor([1.0, 0.8]))
    batch = {"feat": feat, "kaldi_feat": kaldi}
    m, spy = _hook_model(use_kaldi_feat=True)
    x, lens = m._input_feats(batch)
    assert x is kaldi[0] and lens is kaldi[1] and spy.calls == 0
    assert m._feat_field() == "kaldi_feat" and m._dp_lens_field(batch, None) == "kaldi_feat"
    with pytest.raises(ValueError, match=r"synthetic: \{kaldi_feats: true\}"):
        m._input_feats({"feat": feat})
    assert spy.calls == 0
    # without the override, and with anything that is not True (the reference tests `is True`)
    for hp in ({}, {"use_kaldi_feat": False}, {"use_kaldi_feat": "yes"}):
        m, spy = _hook_model(**hp)
        x, lens = m._input_feats(batch)
        assert spy.calls == 1 and torch.equal(x, feat[0] + 1.0) and lens is feat[1]
        assert m._feat_field() == "feat" and m._dp_lens_field(batch, None) == "feat"
    from models.MD_VAE.model import SBModel as MD_VAE
    plain = MD_VAE(modules={}, hparams=dict(normalizer=_Spy(), use_kaldi_feat=True, metric_keys=[],
                                            epoch_counter=types.SimpleNamespace(current=1)),
                   run_opts={"device": "cpu"})
    assert plain._feat_field() == "feat"  # the option is MD_VAE_sfl's, as in the reference
