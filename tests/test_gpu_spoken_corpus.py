"""The spoken synthetic corpus through the device front end (brain.features.Fbank):

* its nearest-centroid frame accuracy equals the float64 helper's on the same waveforms to 0.01
  (the helper's own floor of 0.8 is held by tests/test_fbank_cpu.py);
* the features carry the labels: test_phn_classifier trained through the recipe path
  (prepare_experiment + fit, as train.py runs it) at a small size, the same seed twice -- on the
  spoken corpus and on today's random-feature corpus (the control: its labels are independent of
  its features).  The spoken run's VALID phn_acc.flvl_acc must be at least twice the control's."""
import numpy as np
import pytest
import torch

from conftest import PKG
import fbank_ref as R
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu

EPOCHS = 12  # x 4 steps of 8 utterances


def test_nearest_centroid_parity_with_the_helper():
    need_gpu()
    from brain.features import Fbank
    from utils.data_io import SyntheticSet
    dev = Fbank(deltas=True, sample_rate=16000, hop_length=20, n_fft=400, n_mels=40)
    ref = R.RefFbank(sample_rate=16000, hop_ms=20, win_ms=25, n_fft=400, n_mels=40)
    acc = {}
    for name, cf in (("device", dev), ("helper", ref)):
        kw = dict(md_labels=True, n_phonemes=39, waveforms=True, compute_features=cf)
        train = SyntheticSet(16, 120, 100, 200, 123456, **kw)
        held = SyntheticSet(8, 120, 100, 200, 123457, **kw)
        acc[name] = R.nearest_centroid_accuracy(train.items, held.items)
        if name == "device":
            items = train.items
        else:
            worst = max(float((a["feat"] - b["feat"]).abs().max()) for a, b in zip(items, train.items))
            assert all(torch.equal(a["wav"], b["wav"]) for a, b in zip(items, train.items))
    print(f"nearest-centroid accuracy: device {acc['device']:.4f}, helper {acc['helper']:.4f}; "
          f"max |feat - helper| {worst:.2e} dB")
    assert abs(acc["device"] - acc["helper"]) <= 0.01


def _valid_flvl_acc(waveforms, out_dir):
    from prepare_experiment import prepare_experiment
    overrides = ("{n_phonemes: 7, synthetic: {md_labels: true, phn_labels: true, waveforms: %s, n_train: 32, "
                 "n_valid: 16, n_test: 2, min_frames: 40, max_frames: 60}, model: {n_epochs: %d, "
                 "rnn_hidden_size: 16, lr: 0.01}}" % ("true" if waveforms else "false", EPOCHS))
    args = ["config/run.yaml", "--model_class", "test_phn_classifier", "--model_name", "spoken_ci",
            "--model", "!include:../models/test_phn_classifier/model.yaml", "--output_dir", str(out_dir),
            "--extra_overrides", overrides]
    prepared = prepare_experiment(args, prepare_exp_dir=True)
    hp, model = prepared["hparams"], prepared["model"]
    train_set, valid_set, _ = prepared["datasets"]
    assert ("wav" in train_set.items[0]) == waveforms
    model.fit(hp["model"]["epoch_counter"], train_set, valid_set,
              train_loader_kwargs=hp["train_dataloader_opts"], valid_loader_kwargs=hp["valid_dataloader_opts"])
    # the last stage fit ran is the last epoch's VALID
    return float(model.stats_loggers["phn_acc_stats"].summarize("flvl_acc")) / 100.0


def test_features_carry_the_labels(tmp_path, monkeypatch):
    need_gpu()
    monkeypatch.chdir(PKG)  # the recipe's relative paths, as `python train.py` from the package
    spoken = _valid_flvl_acc(True, tmp_path / "spoken")
    control = _valid_flvl_acc(False, tmp_path / "control")
    print(f"VALID phn_acc.flvl_acc after {EPOCHS} epochs: spoken {spoken:.3f}, control {control:.3f} "
          f"(chance {1 / 7:.3f})")
    assert spoken >= 2 * control
