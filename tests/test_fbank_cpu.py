"""The feature front end's float64 pin against torch.stft, the spoken synthetic corpus's
invariants, the config's compute_features entry and the corpus's separability -- all without a
device (the corpus is built through the numpy helper tests/fbank_ref.py)."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG
import fbank_ref as R
from utils.data_io import SyntheticSet

GEOMETRIES = [(16000, 400, 20), (8000, 256, 10), (16000, 512, 10)]  # (sample rate, n_fft, hop ms)


@pytest.mark.parametrize("sr,n_fft,hop_ms", GEOMETRIES)
def test_power_spectrum_equals_torch_stft(sr, n_fft, hop_ms):
    hop, win = R.geometry(sr, hop_ms, 25)
    g = torch.Generator().manual_seed(5)
    for N in (1, hop - 1, hop, hop + 1, 2345):
        x = torch.randn(N, generator=g, dtype=torch.float64)
        w = torch.from_numpy(R.window(win, n_fft)[(n_fft - win) // 2:(n_fft - win) // 2 + win])
        st = torch.stft(x, n_fft, hop, win, w, center=True, pad_mode="constant", normalized=False,
                        onesided=True, return_complex=True)
        want = (st.real ** 2 + st.imag ** 2).T.numpy()  # [T, bins]
        got = R.power_spectrum(x.numpy(), hop, win, n_fft)
        assert got.shape == want.shape == (1 + N // hop, n_fft // 2 + 1)
        err = np.abs(got - want).max()
        print(f"sr {sr} n_fft {n_fft} hop {hop} N {N}: max |power - stft| {err:.2e}")
        assert err <= 1e-9


def _sets(n_phonemes=39, n=6, **kw):
    ref = R.RefFbank(sample_rate=16000, hop_ms=20, win_ms=25, n_fft=400, n_mels=40)
    base = dict(md_labels=True, n_phonemes=n_phonemes, phn_labels=True, ali_labels=True)
    plain = SyntheticSet(n, 120, 30, 60, 77, **base)
    spoken = SyntheticSet(n, 120, 30, 60, 77, waveforms=True, compute_features=ref, **base, **kw)
    return plain, spoken, ref


def test_spoken_corpus_invariants():
    plain, spoken, ref = _sets()
    again = SyntheticSet(6, 120, 30, 60, 77, md_labels=True, n_phonemes=39, phn_labels=True,
                         ali_labels=True, waveforms=True, compute_features=ref)
    by_id = {e["id"]: e for e in spoken.items}
    assert sorted(by_id) == sorted(e["id"] for e in plain.items)
    changed = 0
    for e in plain.items:
        s = by_id[e["id"]]
        assert set(s) == set(e) | {"wav", "gt_phn_seq"}
        for k, v in e.items():
            if k == "feat":
                assert s[k].shape == v.shape and s[k].dtype == v.dtype
            elif torch.is_tensor(v):
                assert torch.equal(s[k], v), k
            else:
                assert s[k] == v, k
        T = e["feat"].shape[0]
        assert s["wav"].shape == (T * 320,) and s["wav"].dtype == torch.float32
        assert s["gt_phn_seq"].dtype == torch.int64
        assert int(s["gt_phn_seq"].min()) >= 0 and int(s["gt_phn_seq"].max()) < 39
        assert torch.equal(s["gt_phn_seq"] != s["gt_cnncl_seq"], s["plvl_gt_md_lbl_seq"] == 1)
        changed += int((s["plvl_gt_md_lbl_seq"] == 1).sum())
        assert torch.isfinite(s["feat"]).all()
    assert changed > 0
    for a, b in zip(spoken.items, again.items):
        assert a["id"] == b["id"]
        for k, v in a.items():
            assert torch.equal(v, b[k]) if torch.is_tensor(v) else v == b[k], k


def test_spoken_corpus_errors():
    ref = R.RefFbank(sample_rate=16000, hop_ms=20, win_ms=25, n_fft=400, n_mels=40)
    with pytest.raises(ValueError, match="md_labels"):
        SyntheticSet(2, 120, 30, 40, 1, waveforms=True, compute_features=ref)
    with pytest.raises(ValueError, match="n_phonemes"):
        SyntheticSet(2, 120, 30, 40, 1, md_labels=True, n_phonemes=43, waveforms=True, compute_features=ref)
    with pytest.raises(ValueError, match="compute_features"):
        SyntheticSet(2, 120, 30, 40, 1, md_labels=True, waveforms=True)
    with pytest.raises(ValueError, match="input_size"):
        SyntheticSet(2, 80, 30, 40, 1, md_labels=True, waveforms=True, compute_features=ref)


def test_config_gives_the_reference_front_end():
    from brain.features import Fbank
    from hyperpyyaml import load_hyperpyyaml
    ov = ("dataset: synthetic\nmodel_class: test_vanilla_vae\nmodel_name: vae\n"
          "model: !include:../models/test_vanilla_vae/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{"model": {"n_epochs": 1}}, ov])
    fb = hp["compute_features"]
    assert isinstance(fb, Fbank)
    assert (fb.deltas, fb.context, fb.sample_rate, fb.hop_length, fb.n_fft, fb.n_mels, fb.win_length) == \
        (True, False, 16000, 20, 400, 40, 25)
    assert (fb.f_min, fb.f_max, fb.filter_shape) == (0.0, 8000.0, "triangular")
    assert hp["synthetic"]["waveforms"] is False
    assert not list(fb.parameters()) and not list(fb.buffers())


def test_fbank_module_refusals_and_no_random_draw():
    from brain.features import Fbank
    torch.manual_seed(11)
    before = torch.get_rng_state()
    Fbank(deltas=True, hop_length=20)
    assert torch.equal(torch.get_rng_state(), before)
    for kw, word in ((dict(context=True), "context"), (dict(requires_grad=True), "backward"),
                     (dict(filter_shape="gaussian"), "triangular")):
        with pytest.raises(NotImplementedError, match=word):
            Fbank(**kw)


@pytest.mark.parametrize("sr,win,n_fft,n_mels", [(16000, 400, 400, 40), (8000, 200, 256, 23),
                                                 (16000, 399, 512, 64)])
def test_library_table_is_the_helpers(sr, win, n_fft, n_mels):
    """mlvae_fbank_table is host code: the windowed twiddles and filters it fills are the helper's
    float64 ones rounded to fp32, in the kernel's layout (rows = window samples, 32 re | 32 im
    columns per bin tile, then the [bins, 64] filters)."""
    from mlvae_hip import _lib
    l = _lib.lib()
    nbytes = l.mlvae_fbank_table_size(win, n_fft, n_mels)
    K, wr = n_fft // 2 + 1, (win + 1) // 2 * 2
    nbt = (K + 31) // 32
    assert nbytes == 4 * (wr * nbt * 64 + K * 64)
    tab = np.full(nbytes // 4, np.nan, dtype=np.float32)
    assert l.mlvae_fbank_table(sr, win, n_fft, n_mels, 0.0, sr / 2, tab.ctypes.data, nbytes) == 0
    c, s = R.twiddles(win, n_fft)
    lo = (n_fft - win) // 2
    dft = tab[:wr * nbt * 64].reshape(wr, nbt, 2, 32)
    re = dft[:, :, 0, :].reshape(wr, nbt * 32)
    im = dft[:, :, 1, :].reshape(wr, nbt * 32)
    # two libms' float64 cosines may round to neighbouring fp32 values (|entries| <= 1.08)
    assert np.abs(re[:win, :K] - c[lo:lo + win].astype(np.float32)).max() <= 1.2e-7
    assert np.abs(im[:win, :K] - s[lo:lo + win].astype(np.float32)).max() <= 1.2e-7
    assert not re[win:].any() and not im[win:].any() and not re[:, K:].any() and not im[:, K:].any()
    fb = tab[wr * nbt * 64:].reshape(K, 64)
    want = R.mel_filters(sr, n_fft, n_mels)
    assert np.abs(fb[:, :n_mels] - want.astype(np.float32)).max() <= 1e-6
    assert not fb[:, n_mels:].any()
    assert l.mlvae_fbank_table_size(win, n_fft + 1, n_mels) == 0 and "n_fft" in _lib.last_error()


def test_reference_features_separate_the_phonemes():
    """39 phonemes, 16 + 8 utterances of 100-200 frames: the float64 features alone classify the
    pronounced id of a frame by its nearest centroid (chance 0.026)."""
    ref = R.RefFbank(sample_rate=16000, hop_ms=20, win_ms=25, n_fft=400, n_mels=40)
    kw = dict(md_labels=True, n_phonemes=39, waveforms=True, compute_features=ref)
    train = SyntheticSet(16, 120, 100, 200, 123456, **kw)
    held = SyntheticSet(8, 120, 100, 200, 123457, **kw)
    acc = R.nearest_centroid_accuracy(train.items, held.items)
    print(f"nearest-centroid frame accuracy {acc:.3f}")
    assert acc >= 0.8
