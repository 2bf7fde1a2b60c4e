"""The host-side parts of fine-tuning wav2vec2 and of the w2v_LSTM_FC recipe (no GPU):

* the gradient oracle: float64 autograd of tests/w2v_ref.py (tests/w2v_grad_ref.py) against a live
  `transformers` Wav2Vec2Model for the TINY config -- dropout 0, no masking, eval() -- on every
  trainable tensor and at the `proj` stage;
* modules.wav2vec2.Wav2Vec2's constructor matrix (freeze=False alone raises; with the feature
  extractor frozen it builds; the parameter set is everything from the projection upward), the
  state_dict round trip frozen <-> trainable, and the one logged warning for regularisation that a
  config asks for and the module does not build;
* models/w2v_LSTM_FC/model.yaml through load_hyperpyyaml against the reference yaml's key names
  (tests/golden/w2v_lstm_fc_yaml_keys.json), every added and dropped key named;
* tests/golden/w2v_lstm_fc_tiny.npz (make_golden_w2v_lstm_fc.py) is self-consistent: the masked
  BCE recomputed in numpy fp64 from the recorded logits gives the recorded loss, and the recorded
  sequences are round(sigmoid(logits)) and the labels cut to length;
* the recipe's hooks: the stats on every stage, both length refusals, the single-process refusal.
"""
import json
import logging
import os

import numpy as np
import pytest
import torch

import w2v_grad_ref as GR
import w2v_ref as R
from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ["flvl_md.ACC", "flvl_md.PRE", "flvl_md.REC", "flvl_md.F1"]


# --------------------------------------------------------------------------- the gradient oracle
def test_oracle_gradients_match_the_live_model():
    transformers = pytest.importorskip("transformers")
    z = np.load(os.path.join(GOLD, "w2v_tiny.npz"))
    cfg = json.loads(str(z["config"]))
    state = R.fill_state(cfg, int(z["seed"]))
    wav = torch.from_numpy(z["wav"])
    cot = torch.randn(3, R.n_frames(cfg, wav.shape[1]), cfg["hidden_size"], generator=torch.Generator().manual_seed(3))
    _, grads, dproj = GR.encoder_grads(state, cfg, wav, cot, "fp64", normalize_wav=False, output_norm=False)

    hf_cfg = transformers.Wav2Vec2Config(**cfg, hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0,
                                         feat_proj_dropout=0.0, layerdrop=0.0, apply_spec_augment=False)
    model = transformers.Wav2Vec2Model(hf_cfg).eval().double()
    model.load_state_dict({k: v.double() for k, v in state.items()})
    kept = {}

    def keep_proj(mod, inp, out):  # (projected, normalised input): the `proj` stage is the first
        out[0].retain_grad()
        kept["proj"] = out[0]
    hook = model.feature_projection.register_forward_hook(keep_proj)
    out = model(wav.double()).last_hidden_state
    hook.remove()
    (out * cot.double()).sum().backward()
    live = dict(model.named_parameters())
    assert {k for k in live if GR.trainable(k)} == set(grads)
    worst = 0.0
    for k, g in grads.items():
        e = (live[k].grad - g).abs().max().item() / max(g.abs().max().item(), 1e-300)
        worst = max(worst, e)
        # float64 on both sides: summation order only (k_proj.bias's gradient is identically zero:
        # its two roundings are compared to the scale of its weight's gradient)
        scale = grads[k.replace(".bias", ".weight")].abs().max().item() if "k_proj.bias" in k else g.abs().max().item()
        assert (live[k].grad - g).abs().max().item() <= 1e-10 * scale, (k, e)
    e = (kept["proj"].grad - dproj).abs().max().item()
    print(f"worst relative difference {worst:.2e}; at proj {e:.2e}")
    assert e <= 1e-10 * dproj.abs().max().item()


# --------------------------------------------------------------------------- the module
def test_constructor_matrix_and_parameter_set():
    from modules.wav2vec2 import Wav2Vec2
    with pytest.raises(NotImplementedError, match=r"feature extractor has no\s+backward.*freeze_feature_extractor"):
        Wav2Vec2(config=R.TINY, freeze=False)
    with pytest.raises(NotImplementedError, match=r"no\s+backward"):
        Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=False)
    assert list(Wav2Vec2(config=R.TINY, freeze_feature_extractor=True).parameters()) == []  # frozen as before
    m = Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=True)
    names = [k for k, _ in m.named_parameters()]
    # everything but the conv stack; masked_spec_embed is unused without masking and stays a tensor
    want = [k for k in R.state_shapes(R.TINY) if not k.startswith("feature_extractor.") and k != "masked_spec_embed"]
    assert names == want == [k for k in R.state_shapes(R.TINY) if GR.trainable(k)]
    assert all(p.requires_grad and p.dtype == torch.float32 and p.is_leaf for p in m.parameters())
    sd = m.state_dict()
    assert list(sd) == list(R.state_shapes(R.TINY))  # HuggingFace's names and order
    assert all(not v.requires_grad for v in sd.values())
    assert all(sd[k].data_ptr() == p.data_ptr() for k, p in m.named_parameters())  # the masters themselves
    # a ModuleDict (the Brain's) sees the same parameters: an optimizer group over `wav2vec2` gets them
    assert [k for k, _ in torch.nn.ModuleDict({"wav2vec2": m}).named_parameters()] == ["wav2vec2." + k for k in want]
    m.eval()
    m.train()
    assert [k for k, _ in m.named_parameters()] == want


def test_state_dict_round_trips_between_frozen_and_trainable():
    from modules.wav2vec2 import Wav2Vec2
    state = R.fill_state(R.TINY, 4)
    frozen, train = Wav2Vec2(config=R.TINY), Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=True)
    frozen.load_state_dict(state)
    versions = [p._version for p in train.parameters()]
    train.load_state_dict(frozen.state_dict())  # strict
    assert all(p._version > v for p, v in zip(train.parameters(), versions))  # a load refreshes the kernel copies
    assert all(isinstance(p, torch.nn.Parameter) for p in train.parameters())
    back = Wav2Vec2(config=R.TINY)
    back.load_state_dict(train.state_dict())
    for k, v in state.items():
        assert torch.equal(train.state_dict()[k], v) and torch.equal(back.state_dict()[k], v), k
    with pytest.raises(RuntimeError, match="Missing key"):
        train.load_state_dict({k: v for k, v in state.items() if k != "encoder.layer_norm.weight"})


def test_local_directory_load_into_the_trainable_module(tmp_path):
    from modules.wav2vec2 import Wav2Vec2
    state = R.fill_state(R.TINY_D32, 6)
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(R.TINY_D32, model_type="wav2vec2"), f)
    torch.save(state, tmp_path / "pytorch_model.bin")
    m = Wav2Vec2(source=str(tmp_path), freeze=False, freeze_feature_extractor=True)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in state.items())
    torch.save({k: v for k, v in state.items() if k != "encoder.layer_norm.bias"}, tmp_path / "pytorch_model.bin")
    with pytest.raises(ValueError, match="lacks 1 of the encoder's tensors"):
        Wav2Vec2(source=str(tmp_path), freeze=False, freeze_feature_extractor=True)


def test_regularisation_in_a_config_is_ignored_with_one_warning(caplog):
    from modules.wav2vec2 import Wav2Vec2
    cfg = dict(R.TINY, hidden_dropout=0.1, layerdrop=0.05, mask_time_prob=0.05, attention_dropout=0.0)
    with caplog.at_level(logging.WARNING, logger="modules.wav2vec2"):
        Wav2Vec2(config=cfg, freeze=False, freeze_feature_extractor=True)
    assert len(caplog.records) == 1
    msg = caplog.records[0].getMessage()
    assert "not built" in msg and all(k in msg for k in ("hidden_dropout", "layerdrop", "mask_time_prob"))
    assert "attention_dropout" not in msg
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="modules.wav2vec2"):
        Wav2Vec2(config=cfg)                                                   # frozen: nothing is trained
        Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=True)   # nothing asked for
    assert caplog.records == []


# --------------------------------------------------------------------------- yaml
def test_model_yaml_resolves_with_the_reference_keys():
    import functools
    from hyperpyyaml import load_hyperpyyaml
    from modules.fc_block import FCBlock
    from modules.wav2vec2 import Wav2Vec2
    small = {"model": {"wav2vec2_size": 128, "wav2vec2_config": {  # the README's small encoder
        "conv_dim": [32] * 7, "num_hidden_layers": 2, "num_attention_heads": 2, "intermediate_size": 256,
        "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4}}}
    ov = ("dataset: synthetic\nmodel_class: w2v_LSTM_FC\nmodel_name: w2v_lstm_fc\n"
          "model: !include:../models/w2v_LSTM_FC/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [small, ov])
    m = hp["model"]
    with open(os.path.join(GOLD, "w2v_lstm_fc_yaml_keys.json")) as f:
        ref = json.load(f)
    assert ref["modules"] == ["wav2vec2", "classifier"] == list(m["modules"].keys())
    assert ref["optimizers"] == ["adam_opt", "wav2vec_opt"] == list(m["optimizers"].keys())
    # dropped: the two NewBob schedulers the reference's model.py never calls, and their recoverables
    dropped = {"lr_annealing_adam", "lr_annealing_wav2vec"}
    assert set(ref["top_level"]) - set(m.keys()) == dropped
    assert [k for k in ref["recoverables"] if k not in dropped] == list(m["checkpointer"].recoverables.keys()) == [
        "classifier", "wav2vec2", "counter"]
    # added: the encoder's size / architecture / precision overrides of the other w2v recipes
    import re
    text = open(os.path.join(PKG, "models", "w2v_LSTM_FC", "model.yaml")).read()
    own = set(re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", text, flags=re.M))  # (the run's keys join them in m)
    assert own - set(ref["top_level"]) == {"wav2vec2_size", "wav2vec2_config", "wav2vec2_precision"} and own <= set(m)
    assert (m["n_epochs"], m["lr"], m["lr_wav2vec"], m["max_key"]) == (50, 0.0003, 0.0001, "flvl_md.F1")
    assert m["metric_keys"] == KEYS
    enc = m["wav2vec2"]
    assert isinstance(enc, Wav2Vec2) and m["modules"]["wav2vec2"] is enc and m["checkpointer"].recoverables["wav2vec2"] is enc
    assert not enc.freeze and enc.freeze_feature_extractor and enc.output_norm and enc.precision == "bf16"
    assert enc.config["hidden_size"] == 128 and len(list(enc.parameters())) == 41
    clf = m["classifier"]
    assert isinstance(clf, FCBlock) and [(l.in_features, l.out_features) for l, _ in clf.linear_plan()] == [(128, 1)]
    assert [act for _, act in clf.linear_plan()] == [False]
    for name, lr, mods in (("adam_opt", 0.0003, ["classifier"]), ("wav2vec_opt", 0.0001, ["wav2vec2"])):
        g = m["optimizers"][name]
        assert isinstance(g["opt_class"], functools.partial) and g["opt_class"].func is torch.optim.Adam
        assert g["opt_class"].keywords == {"lr": lr} and g["modules"] == mods
    assert m["checkpointer"].recoverables["counter"] is m["epoch_counter"] and m["epoch_counter"].limit == 50


def test_the_large_default_is_large_lv60():
    """The yaml without overrides names the reference's encoder (read, not built: 317 M weights)."""
    text = open(os.path.join(PKG, "models", "w2v_LSTM_FC", "model.yaml")).read()
    for line in ("wav2vec2_size: 1024", "num_hidden_layers: 24", "num_attention_heads: 16", "intermediate_size: 4096",
                 "freeze: False", "freeze_feature_extractor: True", "source: null", "output_norm: True"):
        assert line in text, line


# --------------------------------------------------------------------------- the fixture
def test_fixture_is_self_consistent():
    g = np.load(os.path.join(GOLD, "w2v_lstm_fc_tiny.npz"))
    meta = json.loads(str(g["meta_json"]))
    B, T = meta["B"], meta["T"]
    lbl, rel = g["flvl_gt_md_lbl_seq"], g["feat_lens"].astype(np.float32)
    assert g["short/feats"].shape == (B, T - 1, meta["C"]) and g["equal/feats"].shape == (B, T, meta["C"])
    for case, stage in (("short", "TRAIN"), ("short", "TEST"), ("equal", "TEST")):
        k = f"{case}/{stage}"
        logits = g[k + "/logits"].astype(np.float64)
        n = min(logits.shape[1], T)
        assert logits.shape == (B, g[case + "/feats"].shape[1])
        # the reference's head is one Linear: the recorded logits follow from the recorded features
        w, b = g["param/blocks.0.weight"].astype(np.float64), g["param/blocks.0.bias"].astype(np.float64)
        assert np.allclose(g[case + "/feats"].astype(np.float64) @ w[0] + b[0], logits, rtol=0, atol=1e-5)
        y = lbl[:, :n].astype(np.float64)
        x = logits[:, :n]
        mask = (np.arange(n, dtype=np.float32)[None, :] < (rel * np.float32(n))[:, None]).astype(np.float64)
        bce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
        loss = (bce * mask).sum() / mask.sum()
        assert abs(loss - float(g[k + "/loss"])) <= 1e-6 * abs(loss), (k, loss, float(g[k + "/loss"]))
        lens = [int(torch.round(torch.tensor(r) * n)) for r in rel]
        assert lens == meta["lengths"][case]
        pred = torch.round(torch.sigmoid(torch.from_numpy(g[k + "/logits"][:, :n]))).long().numpy()
        for i, L in enumerate(lens):
            assert g[k + "/pred_md_lbl_seqs"][i].tolist() == pred[i, :L].tolist() + [-1] * (T - L)
            assert g[k + "/gt_md_lbl_seqs"][i].tolist() == lbl[i, :L].tolist() + [-1] * (T - L)
    assert np.array_equal(g["short/TRAIN/logits"], g["short/TEST/logits"])  # no train-mode randomness in the head


# --------------------------------------------------------------------------- the recipe's hooks
class _Fixed(torch.nn.Module):
    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out


def _model(tmp_path, logits):
    from models.w2v_LSTM_FC.model import SBModel
    mods = {"wav2vec2": _Fixed(torch.zeros(2, logits.shape[1], 4)), "classifier": _Fixed(logits.unsqueeze(-1))}
    return SBModel(modules=mods, hparams={"metric_keys": KEYS, "output_dir": str(tmp_path)}, run_opts={"device": "cpu"})


def _batch(T):
    from brain.dataio import PaddedBatch
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    rel = torch.tensor([1.0, 0.5])
    lbl = torch.zeros(2, T, dtype=torch.int64)
    lbl[:, ::2] = 1
    b.update({"id": ["a", "b"], "wav": (torch.zeros(2, 320 * T), rel), "feat": (torch.zeros(2, T, 1), rel),
              "flvl_gt_md_lbl_seq": (lbl, rel)})
    return b


def test_recipe_hooks_lengths_and_rounding(tmp_path):
    from brain import Stage
    from models.md_model import MDModel
    from models.w2v_LSTM_FC.model import SBModel
    from utils.metric_stats.md_metric_stats import MDMetricStats
    assert issubclass(SBModel, MDModel) and SBModel.dp_exact is False
    T = 8
    logits = torch.tensor([[3.0, -2.0, 0.0, 1.0, -1.0, 2.0, -3.0], [1.0, 1.0, -1.0, 0.0, 5.0, 5.0, 5.0]])
    m = _model(tmp_path, logits)  # one frame short of the labels: cut to 7
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        m.on_stage_start(stage, 1)
        assert set(m.stats_loggers) == {"flvl_md_stats"} and isinstance(m.stats_loggers["flvl_md_stats"], MDMetricStats)
    b = _batch(T)
    pred = m.compute_forward(b, Stage.TEST)
    assert torch.equal(pred["logits"], logits)
    loss = m.compute_objectives(pred, b, Stage.TEST)
    # the loss's mask: t < len * 7 in fp32 (7 and 4 frames: 0.5 * 7 = 3.5 -> frames 0..3); the scored
    # sequences: round(len * 7) = 7 and 4 frames (half to even); a logit of exactly 0 predicts 0
    x, y = logits.double(), b["flvl_gt_md_lbl_seq"][0][:, :7].double()
    mask = torch.tensor([[1.0] * 7, [1.0] * 4 + [0.0] * 3], dtype=torch.float64)
    bce = x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    assert abs(loss.item() - ((bce * mask).sum() / mask.sum()).item()) < 1e-6
    seqs = m.stats_loggers["flvl_md_stats"].saved_seqs
    assert seqs["pred_md_lbl_seqs"] == [[1, 0, 0, 1, 0, 1, 0], [1, 1, 0, 0]]
    assert seqs["gt_md_lbl_seqs"] == [[1, 0, 1, 0, 1, 0, 1], [1, 0, 1, 0]]
    # logits longer than the labels: compute_forward refuses one frame, compute_objectives two
    with pytest.raises(ValueError, match="Inconsistent sequence lengths: 7 != 6"):
        m.compute_forward(_batch(6), Stage.TEST)
    m.compute_objectives(pred, _batch(6), Stage.TEST)  # one frame longer passes here, as in the reference
    with pytest.raises(ValueError, match="Inconsistent sequence lengths: 7 != 5"):
        m.compute_objectives(pred, _batch(5), Stage.TEST)
    no_wav = _batch(T)
    del no_wav["wav"]
    with pytest.raises(ValueError, match="waveforms: true"):
        m.compute_forward(no_wav, Stage.TEST)


def test_recipe_is_single_process(tmp_path):
    from brain import Stage
    m = _model(tmp_path, torch.zeros(2, 7))
    m.world_size = 2
    with pytest.raises(RuntimeError, match="single-process.*--distributed_launch"):
        m.on_stage_start(Stage.TRAIN, 1)
