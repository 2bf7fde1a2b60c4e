"""The joint MD-VAE recipes' host-side parts (no GPU):

* the evaluation gates of MD_VAE_joint (TEST, and VALID of every tenth epoch; ``epoch=None`` raises)
  and MD_VAE_joint_ll (every VALID and TEST), with the stats loggers each stage gets;
* both model.yaml files through load_hyperpyyaml with the top-level config, their key names
  against the reference yamls' (tests/golden/md_vae_joint*_yaml_keys.json) plus ``pair_upstream``
  only;
* ops.lstm_pair_ok's truth table on CPU-constructed nn.LSTMs."""
import json
import os

import pytest
import torch

from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = {
    "MD_VAE_joint": ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "vae_kld_loss",
                     "recon_loss", "plvl_md", "boundary.f1", "boundary.r_value"],
    "MD_VAE_joint_ll": ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "pi_nll_loss",
                        "vae_kld_loss", "recon_loss", "plvl_md", "boundary.f1", "boundary.r_value"],
}


def _model(name, tmp_path):
    import importlib
    cls = importlib.import_module(f"models.{name}.model").SBModel
    hp = {"metric_keys": KEYS[name], "output_dir": str(tmp_path),
          "epoch_counter": type("E", (), {"current": 1})()}
    return cls(modules={}, hparams=hp, run_opts={"device": "cpu"})


def _loggers(name, evaluated):
    if not evaluated:
        return set()
    return {k + "_stats" for k in KEYS[name] if k.endswith("_loss")} | {"plvl_md_stats", "boundary_stats"}


def test_joint_evaluation_gate(tmp_path):
    from brain import Stage
    from models.MD_VAE.model import SBModel as MD_VAE
    m = _model("MD_VAE_joint", tmp_path)
    assert isinstance(m, MD_VAE) and m.dp_exact and not hasattr(m, "target")
    for epoch in range(1, 21):
        assert m.to_run_evaluation(Stage.TRAIN, epoch) is False
        assert m.to_run_evaluation(Stage.TEST, epoch) is True
        assert m.to_run_evaluation(Stage.VALID, epoch) == (epoch in (10, 20))
        for stage in (Stage.TRAIN, Stage.VALID):
            m.hparams.epoch_counter.current = epoch
            m.on_stage_start(stage, epoch)
            assert set(m.stats_loggers) == _loggers("MD_VAE_joint", stage == Stage.VALID and epoch % 10 == 0)
    assert m.to_run_evaluation(Stage.TRAIN, None) is False
    assert m.to_run_evaluation(Stage.TEST, None) is True
    with pytest.raises(ValueError, match="epoch"):
        m.to_run_evaluation(Stage.VALID, None)
    m.on_stage_start(Stage.TEST, None)
    assert set(m.stats_loggers) == _loggers("MD_VAE_joint", True)


def test_joint_ll_evaluation_gate(tmp_path):
    from brain import Stage
    from models.MD_VAE_joint.model import SBModel as Joint
    m = _model("MD_VAE_joint_ll", tmp_path)
    assert isinstance(m, Joint) and m.dp_exact
    assert not m.upstream_grad and not m.saves_md_result and Joint.upstream_grad and Joint.saves_md_result
    for epoch in list(range(1, 21)) + [None]:
        assert m.to_run_evaluation(Stage.TRAIN) is False
        assert m.to_run_evaluation(Stage.VALID) is True
        assert m.to_run_evaluation(Stage.TEST) is True
        for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
            m.on_stage_start(stage, epoch)
            assert set(m.stats_loggers) == _loggers("MD_VAE_joint_ll", stage != Stage.TRAIN)


@pytest.mark.parametrize("name,fixture", [("MD_VAE_joint", "md_vae_joint_yaml_keys.json"),
                                          ("MD_VAE_joint_ll", "md_vae_joint_ll_yaml_keys.json")])
def test_model_yaml_resolves_with_the_reference_keys(name, fixture):
    import functools
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import optim as hip_optim
    from modules.boundary_detector import BoundaryDetector
    from modules.lstm import LSTM
    from modules.phoneme_recognizer import PhonemeRecognizer
    ov = (f"dataset: synthetic\nmodel_class: {name}\nmodel_name: {name.lower()}\n"
          f"model: !include:../models/{name}/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    m = hp["model"]
    with open(os.path.join(GOLD, fixture)) as f:
        ref = json.load(f)
    assert list(m["modules"].keys()) == ref["modules"]
    assert list(m["checkpointer"].recoverables.keys()) == ref["recoverables"]
    assert set(ref["top_level"]) <= set(m.keys())
    # the file's own top-level keys: the reference's, in its order, plus pair_upstream only
    import re
    with open(os.path.join(PKG, "models", name, "model.yaml")) as f:
        own = re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", f.read(), flags=re.M)
    assert [k for k in own if k != "pair_upstream"] == ref["top_level"]
    assert own.count("pair_upstream") == 1
    assert isinstance(m["pair_upstream"], bool)
    assert m["max_key"] == "plvl_md.F1"
    assert m["metric_keys"] == KEYS[name]
    assert m["boundary_kld_weight"] == 0.00001 and m["vae_kld_weight"] == 0.00001
    if name == "MD_VAE_joint":
        assert m["phn_recog_bce_weight"] == 10 and m["boundary_bce_weight"] == 10
        assert "pi_nll_weight" not in m
    else:
        assert m["pi_nll_weight"] == 0.001
        assert "phn_recog_bce_weight" not in m and "boundary_bce_weight" not in m
    assert isinstance(m["rnn"], LSTM) and m["rnn"].hidden_size == 512 and m["rnn"].dropout == 0.15
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    recog, det = m["phoneme_recognizer"], m["boundary_detector"]
    assert isinstance(recog, PhonemeRecognizer) and isinstance(det, BoundaryDetector)
    # the shipped upstream stacks are a pair: one shape, no dropout
    from mlvae_hip import ops
    assert ops.lstm_pair_ok(recog.rnn, det.rnn, True)
    assert recog.rnn.hidden_size == 512 and recog.rnn.num_layers == 2


def test_lstm_pair_ok_truth_table():
    from mlvae_hip import ops
    L = lambda i=8, h=16, n=2, **kw: torch.nn.LSTM(i, h, n, **{"batch_first": True, **kw})
    a = L()
    for train in (True, False):
        assert ops.lstm_pair_ok(a, L(), train) is True
        assert ops.lstm_pair_ok(a, a, train) is True
        assert ops.lstm_pair_ok(a, L(h=32), train) is False
        assert ops.lstm_pair_ok(a, L(n=1), train) is False
        assert ops.lstm_pair_ok(a, L(i=12), train) is False
        assert ops.lstm_pair_ok(a, L(bidirectional=True), train) is False
        assert ops.lstm_pair_ok(L(bidirectional=True), L(bidirectional=True), train) is False
        assert ops.lstm_pair_ok(a, L(batch_first=False), train) is False
        assert ops.lstm_pair_ok(L(batch_first=False), a, train) is False
        assert ops.lstm_pair_ok(a, L(proj_size=4), train) is False
        assert ops.lstm_pair_ok(a, torch.nn.GRU(8, 16, 2, batch_first=True), train) is False
        assert ops.lstm_pair_ok(L(h=18), L(h=18), train) is False  # H % 4
    # dropout inside a paired stack: refused in training only
    assert ops.lstm_pair_ok(a, L(dropout=0.15), True) is False
    assert ops.lstm_pair_ok(L(dropout=0.15), a, True) is False
    assert ops.lstm_pair_ok(a, L(dropout=0.15), False) is True
    assert ops.lstm_pair_ok(L(dropout=0.15), L(dropout=0.15), False) is True
    with pytest.raises(ValueError, match="lstm_pair"):
        ops.lstm_pair(torch.zeros(2, 3, 8), a, L(h=32), True)
