"""The w2v_CRDNN_CTC recipes (models/w2v_CRDNN_CTC, models/w2v_CRDNN_CTC_cnncl) on the HIP path, on the
tiny spoken corpus of test_gpu_crdnn_ctc.py (16 utterances of 40-60 frames, 7 phonemes, batch 4) with
the tiny encoder trained whole (bf16) and a small CRDNN of each yaml's shape (32-unit LSTM; no CNN blocks:
the Conv2d family's Cin = 1 layer has no input gradient, which the last test here pins).

* One training batch: the loss is bit-equal to the parent recipe's objective computed on
  feats := wav2vec2(wav) with the same crdnn / output weights (the parent's compute_forward, without a
  normaliser, then its compute_loss); after backward every feature_extractor.* master has a finite,
  non-zero gradient.
* Thirty fit_batch steps on one batch lower the loss; both optimizer groups step, the conv masters move.
* train.py then test.py through the command line on two debug batches: the metric files;
  w2v_CRDNN_CTC_cnncl writes saved_phn_recog_outs.pt with one entry per test utterance, each of that
  utterance's feature-frame length; a second test.py run merges with the duplicate warning; a
  checkpoint round-trips the conv masters.
Reference ops: ref:src/models/w2v_CRDNN_CTC/model.py:7-24, ref:src/models/w2v_CRDNN_CTC_cnncl/model.py:15-68."""
import functools
import glob
import importlib
import os
import types

import numpy as np
import pytest
import torch

import w2v_ref as R
from conftest import PKG
from gpu_utils import need_gpu
from test_gpu_crdnn_ctc import BLANK, BS, C, NPH, corpus  # noqa: F401  (corpus: the fixture)
from test_gpu_md_vae import _script

pytestmark = pytest.mark.gpu

RECIPES = [("w2v_CRDNN_CTC", "CRDNN_CTC"), ("w2v_CRDNN_CTC_cnncl", "CRDNN_CTC_cnncl")]
KEYS = {"w2v_CRDNN_CTC": ["phn_per.error_rate", "cnncl_per.error_rate", "plvl_md"],
        "w2v_CRDNN_CTC_cnncl": ["phn_per.error_rate", "cnncl_per.error_rate"] + [
            f"plvl_md.{k}" for k in ("ACC", "PRE", "REC", "F1", "correct_per", "misp_per")]}
SMALL = ("wav2vec2_size: 128, wav2vec2_config: {conv_dim: [32, 32, 32, 32, 32, 32, 32], num_hidden_layers: 2, "
         "num_attention_heads: 2, intermediate_size: 256, num_conv_pos_embeddings: 16, "
         "num_conv_pos_embedding_groups: 4}")


def _modules(name):
    from modules.crdnn import CRDNN
    from modules.linear import Linear
    from modules.wav2vec2 import Wav2Vec2
    torch.manual_seed(3)
    enc = Wav2Vec2(config=R.TINY, precision="bf16", freeze=False, train_feature_extractor=True)
    enc.load_state_dict(R.fill_state(R.TINY, 20))
    if name.endswith("cnncl"):  # the yaml's shape in small: two layers, bidirectional, two DNN blocks
        crdnn = CRDNN(128, torch.nn.LeakyReLU, 0.15, 0, (128, 128), (3, 3), False, 2, 32, True, 2, 32)
        out = Linear(32, C)
    else:
        crdnn = CRDNN(128, torch.nn.LeakyReLU, 0.15, 0, (16, 16), (3, 3), False, 1, 32, False, 1, 64)
        out = Linear(64, C)
    return {"wav2vec2": enc, "crdnn": crdnn, "output": out}


def _model(tmp_path, cls, modules, **hp):
    SBModel = importlib.import_module(f"models.{cls}.model").SBModel
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1), blank_index=BLANK, batch_size=BS,
                   metric_keys=["plvl_md"], max_key="plvl_md.F1", output_dir=str(tmp_path), **hp)
    return SBModel(modules=modules, hparams=hparams, run_opts={"device": "cuda:0"})


def _batch(corpus):
    return next(b for b in corpus.batches(batch_size=BS) if not torch.equal(b["gt_phn_seq"][0], b["gt_cnncl_seq"][0]))


@pytest.mark.parametrize("name,parent", RECIPES)
def test_loss_equals_the_parent_objective_on_the_encoder_features(tmp_path, corpus, name, parent):
    from brain import Stage
    from mlvae_hip import ops
    mods = _modules(name)
    m = _model(tmp_path, name, mods)
    m.modules.train()
    batch = _batch(corpus)
    m.on_stage_start(Stage.TRAIN, 1)
    torch.manual_seed(11)  # the LSTM's inter-layer dropout key comes from torch's generator
    pred = m.compute_forward(batch, Stage.TRAIN)
    loss = m.compute_objectives(pred, batch, Stage.TRAIN)
    T, Tw = batch["feat"][0].shape[1], mods["wav2vec2"].n_frames(batch["wav"][0].shape[1])
    assert pred["pout"].shape == (BS, Tw, C) and pred["feat_frames"] == T and Tw == T - 1
    assert torch.equal(pred["pout_lens"], batch["feat"][1].to(pred["pout_lens"].device))
    # the parent recipe on feats := wav2vec2(wav): the same crdnn / output modules, no normaliser
    p = _model(tmp_path, parent, {k: mods[k] for k in ("crdnn", "output")})
    p.modules.train()
    p.on_stage_start(Stage.TRAIN, 1)
    with torch.no_grad():
        feats = mods["wav2vec2"](batch["wav"][0].cuda())
    fed = type(batch).__new__(type(batch))
    dict.__init__(fed)
    fed.update(batch)
    fed["feat"] = (feats, batch["feat"][1])
    torch.manual_seed(11)
    ref_pred = p.compute_forward(fed, Stage.TRAIN)
    ref = p.compute_loss(ref_pred, fed)
    print(f"{name}: loss {loss.item():.7f}, the parent's on wav2vec2(wav) {ref.item():.7f}")
    assert torch.equal(ref_pred["pout"], pred["pout"]) and torch.equal(loss.detach(), ref.detach()) and ref.item() > 0
    loss.backward()
    grads = {k: q.grad for k, q in mods["wav2vec2"].named_parameters()}
    conv = [k for k in grads if k.startswith("feature_extractor.")]
    assert len(conv) == 28 and len(grads) == 41 + 28
    for k in grads:
        assert grads[k] is not None and bool(torch.isfinite(grads[k]).all()) and grads[k].abs().max().item() > 0, k
    assert all(q.grad is not None for mod in ("crdnn", "output") for q in mods[mod].parameters())
    ops.raise_ctc_eval_err()


@pytest.mark.parametrize("name,parent", RECIPES)
def test_thirty_steps_on_one_batch_lower_the_loss(tmp_path, corpus, name, parent):
    from brain import Stage
    from mlvae_hip import optim as hip_optim
    mods = _modules(name)
    opts = {"adam_opt": {"opt_class": functools.partial(torch.optim.Adam, lr=1e-2), "modules": ["crdnn", "output"]},
            "wav2vec_opt": {"opt_class": functools.partial(torch.optim.Adam, lr=1e-4), "modules": ["wav2vec2"]}}
    m = _model(tmp_path, name, mods, optimizers=opts)
    m.init_optimizers()
    assert set(m.optimizers) == {"adam_opt", "wav2vec_opt"}
    assert all(isinstance(o, hip_optim.Adam) for o in m.optimizers.values())
    assert len(m.optimizers["wav2vec_opt"].param_groups[0]["params"]) == 41 + 28
    before = {k: v.clone() for k, v in mods["wav2vec2"].state_dict().items()}
    batch = _batch(corpus)
    m.modules.train()
    m.on_stage_start(Stage.TRAIN, 1)
    losses = [float(m.fit_batch(batch)) for _ in range(30)]
    print(f"{name} fit_batch losses:", " ".join(f"{x:.4f}" for x in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    after = mods["wav2vec2"].state_dict()
    for k in after:
        assert torch.equal(after[k], before[k]) == (k == "masked_spec_embed"), k


@pytest.mark.parametrize("name,parent", RECIPES)
def test_train_and_test_scripts(tmp_path, name, parent):
    need_gpu()
    cnncl = name.endswith("cnncl")
    model = ("n_epochs: 2, rnn_neurons: 32, dnn_neurons: 32, lr: 0.01, " + SMALL +
             (", max_key: plvl_md.F1" if cnncl else ""))  # (the reference's _cnncl yaml names no key to keep by)
    overrides = ("{n_phonemes: 7, batch_size: 4, synthetic: {md_labels: true, waveforms: true, n_train: 8, "
                 "n_valid: 8, n_test: 8, min_frames: 40, max_frames: 60}, model: {" + model + "}}")
    common = ["config/run.yaml", "--model_class", name, "--model_name", "w2v_crdnn_ci",
              "--model", f"!include:../models/{name}/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--debug", "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    assert "train loss: " in log and "plvl_md" in log, log[-2000:]
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1 and all(os.path.exists(os.path.join(ckpts[0], f"{k}.ckpt"))
                                   for k in ("wav2vec2", "crdnn", "output", "epoch_counter"))
    # the checkpoint round-trips the conv masters: a strict load into a fresh trainable module, then back
    from modules.wav2vec2 import Wav2Vec2
    state = torch.load(os.path.join(ckpts[0], "wav2vec2.ckpt"), weights_only=True, map_location="cpu")
    enc = Wav2Vec2(config=R.TINY, freeze=False, train_feature_extractor=True)
    fresh = {k: v.clone() for k, v in enc.state_dict().items()}
    enc.load_state_dict(state)
    conv = [k for k in state if k.startswith("feature_extractor.")]
    assert len(conv) == 28
    for k in conv:
        assert torch.equal(enc.state_dict()[k], state[k]) and bool(torch.isfinite(state[k]).all()), k
        assert isinstance(enc.state_dict(keep_vars=True)[k], torch.nn.Parameter)
    # trained: the saved conv weights are no fresh draw's (biases start at 0, LN weights at 1: they moved)
    assert all(not torch.equal(state[k], fresh[k]) for k in conv if k.endswith((".bias", "layer_norm.weight")))
    r = _script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    print(metrics.splitlines()[-1])
    keys = KEYS[name] if cnncl else KEYS[name][:2] + [f"plvl_md.{k}" for k in ("ACC", "PRE", "REC", "F1")]
    assert all(f"{k}: " in metrics for k in keys), metrics
    seqs = open(tmp_path / "out" / "test_output" / "md_result_seqs.txt").read()
    assert seqs.count("ID: ") == 8
    saved_path = tmp_path / "out" / "saved_phn_recog_outs.pt"
    assert saved_path.exists() == cnncl
    if cnncl:
        from brain.features import Fbank
        from utils.data_io import SyntheticSet
        cf = Fbank(deltas=True, sample_rate=16000, hop_length=20, n_fft=400, n_mels=40)
        test_set = SyntheticSet(8, 120, 40, 60, 123456 + 2, md_labels=True, n_phonemes=NPH, waveforms=True,
                                compute_features=cf)
        frames = {e["id"]: e["feat"].shape[0] for e in test_set.items}
        saved = torch.load(saved_path)
        assert set(saved) == set(frames) and len(saved) == 8
        for k, t in saved.items():
            assert tuple(t.shape) == (frames[k], C) and t.device.type == "cpu" and bool(torch.isfinite(t).all()), k
        r = _script(["test.py"] + common, PKG)  # a second run merges, warning of every id it already holds
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stderr.count("duplicate key utt") == 8, r.stderr[-3000:]
        again = torch.load(saved_path)
        assert set(again) == set(saved) and all(torch.equal(again[k], saved[k]) for k in saved)


def test_the_conv_front_end_cannot_sit_on_a_trained_encoder():
    """Why the yamls ship cnn_blocks: 0: the Conv2d family's Cin = 1 layer has no input gradient."""
    need_gpu()
    from mlvae_hip import ops
    from modules.crdnn import ConvCRDNN
    front = ConvCRDNN(128, torch.nn.LeakyReLU, 0.15, 1, (16, 16), (3, 3), True, 1, 32, False, 1, 64).cuda()
    feats = torch.randn(2, 20, 128, device="cuda", requires_grad=True)
    with ops.precision("bf16"), pytest.raises(ValueError, match="Cin = 1 layer has no input gradient"):
        front(feats)
