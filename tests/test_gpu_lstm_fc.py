"""The LSTM_FC recipe (models/LSTM_FC) on the HIP path.

* compute_forward + compute_objectives against the reference's own numbers
  (tests/golden/lstm_fc_tiny.npz, make_golden_lstm_fc.py), fp32: ``out`` and the loss at 1e-5
  relative-max for TRAIN and TEST, every parameter gradient at 1e-4 (test_gpu_md_vae.py's bounds
  for the same quantities), the predicted and the true labels cut to length equal to the recorded
  sequences, and the summarised flvl_md scores equal to MDMetricStats fed those sequences.
* train.py / test.py end to end with --model_class LSTM_FC on the synthetic corpus with MD labels.
Reference ops: ref:src/models/LSTM_FC/model.py:16-69."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import PKG
from gpu_utils import need_gpu, rel_err
from test_gpu_md_vae import _script

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstm_fc_tiny.npz")
KEYS = ["flvl_md.ACC", "flvl_md.PRE", "flvl_md.REC", "flvl_md.F1"]


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLD)
    return {k: d[k] for k in d.files}


def _model(gold, tmp_path):
    from models.LSTM_FC.model import SBModel
    from modules.fc_block import FCBlock
    from modules.lstm import LSTM
    meta = json.loads(str(gold["meta_json"]))
    modules = {"lstm": LSTM(batch_first=True, input_size=meta["F"], hidden_size=meta["H"],
                            num_layers=meta["L"], dropout=0.0),
               "fc": FCBlock(meta["fc_sizes"], dropout=0)}
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1), misp_weight=meta["misp_weight"],
                   batch_size=meta["B"], metric_keys=KEYS, output_dir=str(tmp_path))
    m = SBModel(modules=modules, hparams=hparams, run_opts={"device": "cuda:0"})
    assert [n for n, _ in m.modules.named_parameters()] == meta["param_names"]
    m.modules.load_state_dict({n: torch.from_numpy(gold["param/" + n]) for n in meta["param_names"]})
    return m, meta


def _batch(gold, meta, aug):
    from brain.dataio import PaddedBatch
    t = lambda k: torch.from_numpy(gold[k])
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    fl = t("feat_lens")
    b.update({"id": [f"utt{i}" for i in range(meta["B"])], "feat": (t("feat"), fl),
              "flvl_gt_md_lbl_seq": (t("flvl_gt_md_lbl_seq"), fl)})
    if aug:  # the reference's field names in TRAIN; the plain ones then hold something else
        b.update({"aug_feat": b["feat"], "aug_flvl_gt_md_lbl_seq": b["flvl_gt_md_lbl_seq"],
                  "feat": (torch.zeros_like(t("feat")), fl),
                  "flvl_gt_md_lbl_seq": (1 - t("flvl_gt_md_lbl_seq"), fl)})
    return b


def _seqs(padded):
    return [[v for v in row if v >= 0] for row in padded.tolist()]


def _run(m, batch, stage, name, gold, meta):
    from utils.metric_stats.md_metric_stats import MDMetricStats
    m.on_stage_start(stage, 1)
    pred = m.compute_forward(batch, stage)
    loss = m.compute_objectives(pred, batch, stage)
    e_out = rel_err(pred["out"], torch.from_numpy(gold[name + "/out"]))
    e_loss = rel_err(loss, torch.from_numpy(gold[name + "/loss"]))
    print(f"{name}: out rel {e_out:.2e}, loss {float(loss.detach()):.7f} ref {float(gold[name + '/loss']):.7f} "
          f"rel {e_loss:.2e}")
    assert pred["out"].shape == (meta["B"], meta["T"], 2)
    assert e_out < 1e-5 and e_loss < 1e-5
    # the predicted labels, cut to length (-1 past it), and the labels: the recorded sequences
    want_pred, want_gt = gold[name + "/pred_md_lbl_seqs"], gold[name + "/gt_md_lbl_seqs"]
    got = pred["flvl_pred_md_lbl_seq"].cpu().numpy()
    assert np.array_equal(got, want_pred)
    assert _seqs(got) == _seqs(want_pred)
    lens = meta["lengths"]
    assert [row[:n] for row, n in zip(gold["flvl_gt_md_lbl_seq"].tolist(), lens)] == _seqs(want_gt)
    # the stage's scores from the device counts against MDMetricStats fed the recorded sequences
    ref = MDMetricStats()
    ref.append(batch["id"], pred_md_lbl_seqs=_seqs(want_pred), gt_md_lbl_seqs=_seqs(want_gt))
    st = m.stats_loggers["flvl_md_stats"]
    assert st.scores_list == []  # nothing brought to the host per batch
    assert st.summarize() == ref.summarize()
    for a, b in zip(st.scores_list, ref.scores_list):
        assert all(torch.equal(a[k], b[k]) for k in ("ACC", "PRE", "REC", "F1"))
    print(f"{name}: flvl_md {st.summarize()}")
    return pred, loss


def test_train_matches_reference(gold, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = _model(gold, tmp_path)
    m.modules.train()
    pred, loss = _run(m, _batch(gold, meta, aug=True), Stage.TRAIN, "TRAIN", gold, meta)
    assert not pred["out"].requires_grad and pred["loss_e"].requires_grad
    loss.backward()
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        assert p.grad is not None, n
        e = rel_err(p.grad, torch.from_numpy(gold[f"TRAIN/grad/{n}"]))
        print(f"TRAIN grad {n} rel {e:.2e}")
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (n, e)
    print(f"TRAIN: worst gradient {worst[0]} rel {worst[1]:.2e}")
    # without the aug_ fields TRAIN reads the plain ones: the same numbers
    m.modules.zero_grad()
    _run(m, _batch(gold, meta, aug=False), Stage.TRAIN, "TRAIN", gold, meta)


def test_test_matches_reference(gold, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = _model(gold, tmp_path)
    m.modules.eval()
    with torch.no_grad():
        # evaluation reads the plain fields even when the batch has the aug_ ones
        b = _batch(gold, meta, aug=False)
        b.update({"aug_feat": (torch.zeros_like(b["feat"][0]), b["feat"][1]),
                  "aug_flvl_gt_md_lbl_seq": (1 - b["flvl_gt_md_lbl_seq"][0], b["feat"][1])})
        _run(m, b, Stage.TEST, "TEST", gold, meta)
    m.on_stage_end(Stage.TEST, 0.0, None)
    metrics = open(tmp_path / "test_output" / "test_metrics.txt").read()
    for k in KEYS:
        assert k in metrics, (k, metrics)


def test_bad_label_raises_at_the_stage_end(gold, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = _model(gold, tmp_path)
    m.modules.eval()
    b = _batch(gold, meta, aug=False)
    lbl = b["flvl_gt_md_lbl_seq"][0].clone()
    lbl[2, meta["lengths"][2] - 1] = 3  # the last valid frame of the shortest utterance
    b["flvl_gt_md_lbl_seq"] = (lbl, b["feat"][1])
    m.on_stage_start(Stage.VALID, 1)
    with torch.no_grad():
        m.compute_objectives(m.compute_forward(b, Stage.VALID), b, Stage.VALID)  # no raise per batch
    with pytest.raises(ValueError, match="outside"):
        m.on_stage_end(Stage.VALID, 0.0, 1)


def test_train_and_test_scripts(tmp_path):
    need_gpu()
    overrides = ("{synthetic: {md_labels: true, n_train: 16, n_valid: 8, n_test: 8, min_frames: 40, "
                 "max_frames: 60}, model: {n_epochs: 1, lstm_hidden_size: 16, lstm_num_layers: 2, "
                 "lr: 0.001}}")
    common = ["config/run.yaml", "--model_class", "LSTM_FC", "--model_name", "lstm_fc_ci",
              "--model", "!include:../models/LSTM_FC/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    lines = [l for l in log.splitlines() if "flvl_md.F1" in l]
    assert len(lines) == 2, log[-2000:]  # TRAIN and VALID both score, as the reference
    assert lines[0].startswith("stage: train, epoch: 1") and lines[1].startswith("stage: valid, epoch: 1")
    for key in KEYS:
        assert f"train {key}" in lines[0] and f"valid {key}" in lines[1], (key, lines)
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1
    from modules.fc_block import FCBlock
    from modules.lstm import LSTM
    fc, lstm = FCBlock([16, 64, 64, 2]), LSTM(batch_first=True, input_size=120, hidden_size=16, num_layers=2)
    fc.load_state_dict(torch.load(os.path.join(ckpts[0], "fc.ckpt"), weights_only=True))  # strict
    lstm.load_state_dict(torch.load(os.path.join(ckpts[0], "lstm.ckpt"), weights_only=True))
    assert all(bool(torch.isfinite(p).all()) for mod in (fc, lstm) for p in mod.parameters())
    assert os.path.exists(os.path.join(ckpts[0], "normalizer.ckpt"))
    r = _script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    for key in KEYS:
        assert key in metrics, (key, metrics)
