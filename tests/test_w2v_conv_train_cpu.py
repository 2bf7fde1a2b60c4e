"""The host-side parts of training wav2vec2 whole and of the w2v_CRDNN_CTC recipes (no GPU):

* modules.wav2vec2.Wav2Vec2's constructor matrix with ``train_feature_extractor``: the two
  contradictions raise ValueError, the old NotImplementedErrors are still raised without it, the
  parameter set is every tensor but masked_spec_embed under HuggingFace's names and in its order
  (fp32 leaves, state_dict shares their storage), a ModuleDict optimizer group sees them;
* the input gradient's residue decomposition (ops.w2v_conv_dx), restated in plain torch
  (tests/w2v_conv_grad_ref.conv_dx_by_residue), against conv1d's autograd in float64 for every
  (k, stride) the device tests use -- the index arithmetic, pinned without a GPU -- and the device
  op's own geometry and weight regrouping (host code) against the restatement's;
* models/w2v_CRDNN_CTC/model.yaml and models/w2v_CRDNN_CTC_cnncl/model.yaml through load_hyperpyyaml
  with the README's overrides against the reference yamls' key names
  (tests/golden/w2v_crdnn_ctc_yaml_keys.json, w2v_crdnn_ctc_cnncl_yaml_keys.json), every added and
  dropped key named;
* the recipes' hooks: what they subclass, the missing-wav refusal, the single-process refusal.
"""
import functools
import json
import os
import re

import pytest
import torch

import w2v_conv_grad_ref as CR
import w2v_ref as R
from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KS = [(3, 2), (2, 2), (3, 1), (4, 3), (3, 3)]


# --------------------------------------------------------------------------- the module
def test_constructor_matrix_with_the_new_keyword():
    from modules.wav2vec2 import Wav2Vec2
    with pytest.raises(ValueError, match="train_feature_extractor=True contradicts"):
        Wav2Vec2(config=R.TINY, train_feature_extractor=True)  # freeze defaults to True
    with pytest.raises(ValueError, match="train_feature_extractor=True contradicts"):
        Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=True, train_feature_extractor=True)
    with pytest.raises(NotImplementedError, match=r"no\s+backward.*freeze_feature_extractor.*train_feature_extractor"):
        Wav2Vec2(config=R.TINY, freeze=False)
    with pytest.raises(NotImplementedError, match=r"no\s+backward"):
        Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=False, train_feature_extractor=False)
    m = Wav2Vec2(config=R.TINY, freeze=False, train_feature_extractor=True)
    assert m.train_feature_extractor and not m.freeze and not m.freeze_feature_extractor
    assert not Wav2Vec2(config=R.TINY).train_feature_extractor
    names = [k for k, _ in m.named_parameters()]
    want = [k for k in R.state_shapes(R.TINY) if k != "masked_spec_embed"]
    assert names == want == [k for k in R.state_shapes(R.TINY) if CR.trainable(k)]
    assert sum(k.startswith("feature_extractor.conv_layers.") for k in names) == 7 * 4
    for i in range(7):
        for n in ("conv.weight", "conv.bias", "layer_norm.weight", "layer_norm.bias"):
            assert f"feature_extractor.conv_layers.{i}.{n}" in names
    assert all(p.requires_grad and p.dtype == torch.float32 and p.is_leaf for p in m.parameters())
    shapes = R.state_shapes(R.TINY)
    assert all(tuple(p.shape) == tuple(shapes[k]) for k, p in m.named_parameters())
    sd = m.state_dict()
    assert list(sd) == list(shapes)  # HuggingFace's names and order, masked_spec_embed included
    assert all(not v.requires_grad for v in sd.values())
    assert all(sd[k].data_ptr() == p.data_ptr() for k, p in m.named_parameters())  # the masters themselves
    assert not isinstance(m.state_dict(keep_vars=True)["masked_spec_embed"], torch.nn.Parameter)
    assert [k for k, _ in torch.nn.ModuleDict({"wav2vec2": m}).named_parameters()] == ["wav2vec2." + k for k in want]
    opt = torch.optim.Adam(torch.nn.ModuleDict({"wav2vec2": m}).parameters(), lr=1e-4)
    assert len(opt.param_groups[0]["params"]) == len(want)
    m.eval()
    m.train()
    assert [k for k, _ in m.named_parameters()] == want
    # a state dict round-trips between the three kinds of module, and a load refreshes the kernel copies
    state = R.fill_state(R.TINY, 4)
    versions = [p._version for p in m.parameters()]
    m.load_state_dict(state)
    assert all(p._version > v for p, v in zip(m.parameters(), versions))
    frozen, head = Wav2Vec2(config=R.TINY), Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=True)
    frozen.load_state_dict(m.state_dict())
    head.load_state_dict(m.state_dict())
    for k, v in state.items():
        assert torch.equal(frozen.state_dict()[k], v) and torch.equal(head.state_dict()[k], v), k


# --------------------------------------------------------------------------- the residue decomposition
@pytest.mark.parametrize("k,stride", KS)
@pytest.mark.parametrize("T_in", [1, 23, 24, 25])
def test_residue_decomposition_equals_conv1d_autograd(k, stride, T_in):
    """T_in = k + extra: Tout = 1 at extra = 1 (or 0 trailing frames when stride = 1), and the three
    longer ones cover every (T_in - k) % stride."""
    T_in = k + T_in
    g = torch.Generator().manual_seed(100 * k + stride)
    B, Cin, Cout = 3, 5, 7
    x = torch.randn(B, T_in, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, k, generator=g, dtype=torch.float64)
    Tout = (T_in - k) // stride + 1
    dy = torch.randn(B, Tout, Cout, generator=g, dtype=torch.float64)
    want, _ = CR.conv_grads(x, w, dy, stride, torch.float64)
    got = CR.conv_dx_by_residue(dy, w, stride, T_in)
    assert got.shape == want.shape == (B, T_in, Cin)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    used = (Tout - 1) * stride + k
    assert torch.equal(got[:, used:], torch.zeros(B, T_in - used, Cin, dtype=torch.float64))  # exactly zero
    # the device op's host side: the same geometry, the same regrouped weights
    from mlvae_hip.ops import w2v as W
    T, m, pf, pa = W._conv_geometry(k, stride, T_in)
    assert T == Tout and m == [-((r - k) // stride) for r in range(stride)] and sum(m) == k
    assert pf == m[0] - 1 and pa == -(-T_in // stride) - Tout >= 0
    regrouped = W.w2v_conv_dx_weights(w, stride, torch.float64)
    assert len(regrouped) == stride
    for r, wr in enumerate(regrouped):
        assert wr.is_contiguous() and wr.shape == (Cin, m[r] * Cout)
        for q in range(m[r]):  # row block j holds tap r + (m_r - 1 - j) stride, in / out swapped
            assert torch.equal(wr[:, (m[r] - 1 - q) * Cout:(m[r] - q) * Cout], w[:, :, r + q * stride].t())
    # every GEMM row of every residue stays inside its utterance's guarded block
    for r in range(stride):
        Ur = -(-(T_in - r) // stride)
        assert pf - (m[r] - 1) >= 0 and pf - (m[r] - 1) + Ur - 1 + m[r] <= pf + Tout + pa


def test_stride_longer_than_the_kernel_is_refused():
    from mlvae_hip.ops import w2v as W
    with pytest.raises(ValueError, match="1 <= stride <= k"):
        W.w2v_conv_dx_weights(torch.zeros(8, 8, 2), 3, torch.float32)
    with pytest.raises(ValueError, match="1 <= stride <= k"):
        W._conv_geometry(2, 3, 10)
    with pytest.raises(ValueError, match="1 <= stride <= k"):
        W._conv_geometry(2, 0, 10)


# --------------------------------------------------------------------------- yaml
SMALL = {"wav2vec2_size": 128, "wav2vec2_config": {  # the README's small encoder
    "conv_dim": [32] * 7, "num_hidden_layers": 2, "num_attention_heads": 2, "intermediate_size": 256,
    "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4}}
ADDED = {"wav2vec2_size", "wav2vec2_config", "wav2vec2_precision", "blank_index"}
# Adam replaces Adadelta + NewBob; SpeechBrain callables the HIP ops replace; jit is not a thing here
DROPPED = {"scheduler", "log_softmax", "compute_cost", "jit_module_keys"}


def _load(name, extra=None):
    from hyperpyyaml import load_hyperpyyaml
    ov = (f"dataset: synthetic\nmodel_class: {name}\nmodel_name: ci\nn_phonemes: 7\n"
          f"model: !include:../models/{name}/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        return load_hyperpyyaml(f, [{"model": dict(SMALL, **(extra or {}))}, ov])["model"]


@pytest.mark.parametrize("name,fixture", [("w2v_CRDNN_CTC", "w2v_crdnn_ctc"), ("w2v_CRDNN_CTC_cnncl", "w2v_crdnn_ctc_cnncl")])
def test_model_yaml_resolves_with_the_reference_keys(name, fixture):
    from modules.crdnn import CRDNN, ConvCRDNN
    from modules.linear import Linear
    from modules.wav2vec2 import Wav2Vec2
    cnncl = name.endswith("cnncl")
    m = _load(name)
    with open(os.path.join(GOLD, fixture + "_yaml_keys.json")) as f:
        ref = json.load(f)
    assert ref["modules"] == ["wav2vec2", "crdnn", "output"] == list(m["modules"].keys())
    assert ref["optimizers"] == ["adam_opt", "wav2vec_opt"] == list(m["optimizers"].keys())
    text = open(os.path.join(PKG, "models", name, "model.yaml")).read()
    own = set(re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", text, flags=re.M))  # (the run's keys join them in m)
    assert set(ref["top_level"]) - own == DROPPED and own - set(ref["top_level"]) == ADDED and own <= set(m)
    assert [k for k in ref["recoverables"] if k not in DROPPED] == list(m["checkpointer"].recoverables.keys()) == [
        "wav2vec2", "crdnn", "output", "epoch_counter"]
    assert m["metric_keys"] == ref["metric_keys"]
    assert (m["n_epochs"], m["lr"], m["lr_wav2vec"], m["dropout"]) == (50, 0.1, 0.0001, 0.15)
    assert m["output_neurons"] == 9 and m["blank_index"] == 8
    # the Conv2d family's Cin = 1 layer has no input gradient, so the CNN blocks and the time pooling are
    # off (the yaml's header); the reference's values stay beside the keys as comments
    assert m["cnn_blocks"] == 0 and "time_pooling: False  # the reference: True" in text
    if cnncl:
        assert (m["cnn_channels"], m["rnn_layers"], m["rnn_neurons"], m["rnn_bidirectional"], m["dnn_blocks"],
                m["dnn_neurons"], m["time_pooling"]) == ([128, 128], 2, 512, True, 2, 128, False)
        assert "min_key" in m and "max_key" in m and m["min_key"] is None and m["max_key"] is None
        assert "cnn_blocks: 0  # the reference: 2" in text
    else:
        assert (m["cnn_channels"], m["rnn_layers"], m["rnn_neurons"], m["rnn_bidirectional"], m["dnn_blocks"],
                m["dnn_neurons"]) == ([16, 16], 1, 32, False, 1, 64)
        assert m["max_key"] == "plvl_md.F1" and "min_key" not in m and "cnn_blocks: 0  # the reference: 1" in text
    enc = m["wav2vec2"]
    assert isinstance(enc, Wav2Vec2) and m["modules"]["wav2vec2"] is enc and m["checkpointer"].recoverables["wav2vec2"] is enc
    assert not enc.freeze and not enc.freeze_feature_extractor and enc.train_feature_extractor
    assert enc.output_norm and enc.normalize_wav and enc.precision == "bf16" and enc.config["hidden_size"] == 128
    assert len(list(enc.parameters())) == 41 + 28
    crdnn = m["crdnn"]
    assert type(crdnn) is CRDNN and not isinstance(crdnn, ConvCRDNN) and crdnn.rnn.input_size == 128
    assert crdnn.rnn.hidden_size == m["rnn_neurons"] and crdnn.rnn.bidirectional == m["rnn_bidirectional"]
    assert crdnn.rnn.num_layers == m["rnn_layers"] and len(crdnn.dnn) == m["dnn_blocks"]
    assert isinstance(m["output"], Linear) and m["output"].w.weight.shape == (9, m["dnn_neurons"])
    for key, lr, mods in (("adam_opt", 0.1, ["crdnn", "output"]), ("wav2vec_opt", 0.0001, ["wav2vec2"])):
        g = m["optimizers"][key]
        assert isinstance(g["opt_class"], functools.partial) and g["opt_class"].func is torch.optim.Adam
        assert g["opt_class"].keywords == {"lr": lr} and g["modules"] == mods
    assert m["checkpointer"].recoverables["epoch_counter"] is m["epoch_counter"] and m["epoch_counter"].limit == 50


@pytest.mark.parametrize("name", ["w2v_CRDNN_CTC", "w2v_CRDNN_CTC_cnncl"])
def test_the_large_default_is_large_lv60_trained_whole(name):
    """The yaml without overrides names the reference's encoder (read, not built: 317 M weights)."""
    text = open(os.path.join(PKG, "models", name, "model.yaml")).read()
    for line in ("wav2vec2_size: 1024", "num_hidden_layers: 24", "num_attention_heads: 16", "intermediate_size: 4096",
                 "freeze: False", "train_feature_extractor: True", "source: null", "output_norm: True",
                 "input_size: !ref <wav2vec2_size>", "crdnn: !new:modules.crdnn.CRDNN"):
        assert line in text, line
    assert "freeze_feature_extractor" not in text


# --------------------------------------------------------------------------- the recipes' hooks
class _Fixed(torch.nn.Module):
    def forward(self, x):
        return x


@pytest.mark.parametrize("name,parent", [("w2v_CRDNN_CTC", "CRDNN_CTC"), ("w2v_CRDNN_CTC_cnncl", "CRDNN_CTC_cnncl")])
def test_recipe_hooks(tmp_path, name, parent):
    import importlib
    from brain import Stage
    from brain.dataio import PaddedBatch
    SBModel = importlib.import_module(f"models.{name}.model").SBModel
    Parent = importlib.import_module(f"models.{parent}.model").SBModel
    assert issubclass(SBModel, Parent) and SBModel.dp_exact is False
    assert SBModel.compute_objectives is Parent.compute_objectives and SBModel.compute_loss is Parent.compute_loss
    mods = {"wav2vec2": _Fixed(), "crdnn": _Fixed(), "output": _Fixed()}
    m = SBModel(modules=mods, hparams={"metric_keys": ["plvl_md"], "output_dir": str(tmp_path), "blank_index": 8},
                run_opts={"device": "cpu"})
    m.on_stage_start(Stage.TEST, 1)
    assert set(m.stats_loggers) == {"phn_per_stats", "cnncl_per_stats", "plvl_md_stats", "boundary_stats"}
    assert (getattr(m, "saved_pouts", None) == {}) == name.endswith("cnncl")
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    rel = torch.tensor([1.0, 0.5])
    seq = (torch.zeros(2, 3, dtype=torch.int64), rel)
    b.update({"id": ["a", "b"], "feat": (torch.zeros(2, 8, 1), rel), "gt_phn_seq": seq, "gt_cnncl_seq": seq,
              "gt_boundary_seq": (torch.zeros(2, 8, dtype=torch.int64), rel)})
    with pytest.raises(ValueError, match=name + ": the batch has no wav.*waveforms: true"):
        m.compute_forward(b, Stage.TEST)
    m.world_size = 2
    with pytest.raises(RuntimeError, match=name + " recipe is single-process.*--distributed_launch"):
        m.on_stage_start(Stage.TRAIN, 1)
