"""The single-encoder VAE recipes' host-side parts (no GPU):

* models/test_gmm_vae and models/test_h_vae: model.yaml through load_hyperpyyaml with the top-level
  config; key names, their order and their values against the reference yamls'
  (tests/golden/test_*_vae_yaml_keys.json) plus ``fused_latent``; test_h_vae's recoverables are
  the reference's list followed by rnn and pi_fc;
* the loss stats loggers of every stage; the fused engine declines both recipes;
* the fixtures carry what the GPU tests read;
* ops.hvae_latent / ops.gmm_collapsed argument checks, which raise before any launch."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _resolve(recipe):
    from hyperpyyaml import load_hyperpyyaml
    ov = (f"dataset: synthetic\nmodel_class: {recipe}\nmodel_name: ci\n"
          f"model: !include:../models/{recipe}/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    with open(os.path.join(GOLD, f"{recipe}_yaml_keys.json")) as f:
        return hp, hp["model"], json.load(f)


def _own_keys(recipe):
    with open(os.path.join(PKG, "models", recipe, "model.yaml")) as f:
        return re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", f.read(), flags=re.M)


def _common(recipe, m, ref):
    from brain.features import InputNormalization
    from mlvae_hip import optim as hip_optim
    from modules.decoder import Decoder
    assert list(m["modules"].keys()) == ref["modules"]
    assert set(ref["top_level"]) <= set(m.keys())
    # the file's own top-level keys: the reference's, in its order, plus fused_latent only
    own = _own_keys(recipe)
    assert [k for k in own if k != "fused_latent"] == ref["top_level"]
    assert own.count("fused_latent") == 1 and isinstance(m["fused_latent"], bool)
    assert (m["n_epochs"], m["lr"], m["latent_size"], m["num_components"], m["enc_fc_size"]) == \
        (50, 0.001, 32, 3, 64)
    assert (m["dec_rnn_hidden_size"], m["dec_rnn_num_layers"], m["dec_rnn_dropout"], m["dec_fc_size"]) == \
        (512, 2, 0.15, 64)
    assert m["min_key"] == "loss" and "max_key" not in m
    assert isinstance(m["normalizer"], InputNormalization) and m["epoch_counter"].limit == 50
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    assert m["optimizer"].keywords == {"lr": 0.001}
    dec = m["decoder"]
    assert isinstance(dec, Decoder) and m["modules"]["decoder"] is dec
    assert (dec.rnn.input_size, dec.rnn.hidden_size, dec.rnn.num_layers, dec.rnn.dropout) == (32, 512, 2, 0.15)
    assert dec.rnn.bidirectional
    for k in ref["modules"]:
        assert m["modules"][k] is m[k] is m["checkpointer"].recoverables[k]


def test_gmm_vae_yaml_resolves_with_the_reference_keys():
    from modules.gmm_vae import GMMVAE
    hp, m, ref = _resolve("test_gmm_vae")
    _common("test_gmm_vae", m, ref)
    assert ref["modules"] == ["encoder", "decoder"]
    assert list(m["checkpointer"].recoverables.keys()) == ref["recoverables"] == ["encoder", "decoder", "epoch_counter"]
    assert m["metric_keys"] == ["kld_loss", "recon_loss"] and m["kld_weight"] == 0.001
    enc = m["encoder"]
    assert isinstance(enc, GMMVAE) and (enc.latent_size, enc.num_components) == (32, 3)
    assert enc.mean_fc.in_features == 64 and enc.mean_fc.out_features == 96
    assert hp["synthetic"]["md_labels"] is False  # the plain corpus is enough


def test_h_vae_yaml_resolves_with_the_reference_keys():
    from modules.fc_block import FCBlock
    from modules.h_vae import HierarchicalVAE
    from modules.lstm import LSTM
    hp, m, ref = _resolve("test_h_vae")
    _common("test_h_vae", m, ref)
    assert ref["modules"] == ["rnn", "pi_fc", "encoder", "decoder"]
    # the recoverables rule: the reference's list is a prefix of ours, the extras are rnn and pi_fc
    ours = list(m["checkpointer"].recoverables.keys())
    assert ref["recoverables"] == ["encoder", "decoder", "epoch_counter"]
    assert ours[:len(ref["recoverables"])] == ref["recoverables"]
    assert ours[len(ref["recoverables"]):] == ["rnn", "pi_fc"]
    assert m["metric_keys"] == ["vae_kld_loss", "recon_loss"] and m["vae_kld_weight"] == 0.001
    assert (m["rnn_hidden_size"], m["rnn_num_layers"], m["rnn_dropout"], m["pi_fc_size"]) == (512, 2, 0.15, 128)
    rnn = m["rnn"]
    assert isinstance(rnn, LSTM) and not rnn.bidirectional and rnn.batch_first
    assert (rnn.input_size, rnn.hidden_size, rnn.num_layers, rnn.dropout) == (120, 512, 2, 0.15)
    assert isinstance(m["pi_fc"], FCBlock)
    sizes = [(b.in_features, b.out_features) for b in m["pi_fc"].blocks if isinstance(b, torch.nn.Linear)]
    assert sizes == [(512, 128), (128, 64), (64, 2)]
    enc = m["encoder"]
    assert isinstance(enc, HierarchicalVAE) and enc.fused is m["fused_latent"]
    assert enc.gmm_vae.num_components == 3 and enc.vanilla_vae.latent_size == 32
    assert enc.vanilla_vae.fc[0].linear_plan()[0][0].in_features == 512
    assert hp["synthetic"]["md_labels"] is False


def test_fused_flag_reaches_the_encoder():
    from hyperpyyaml import load_hyperpyyaml
    for flag in (True, False):
        ov = ("dataset: synthetic\nmodel_class: test_h_vae\nmodel_name: ci\n"
              "model: !include:../models/test_h_vae/model.yaml\n")
        with open(os.path.join(PKG, "config", "run.yaml")) as f:
            hp = load_hyperpyyaml(f, [{"model": {"fused_latent": flag, "rnn_hidden_size": 16,
                                                 "dec_rnn_hidden_size": 16}}, ov])
        assert hp["model"]["encoder"].fused is flag
    from modules.h_vae import HierarchicalVAE
    assert HierarchicalVAE([4, 4], 2, 2).fused is False  # the default: the composed path


@pytest.mark.parametrize("recipe,keys", [("test_gmm_vae", ["kld_loss", "recon_loss"]),
                                         ("test_h_vae", ["vae_kld_loss", "recon_loss"])])
def test_recipe_builds_its_loss_stats_on_every_stage(recipe, keys, tmp_path):
    import importlib
    from brain import Stage
    from models.md_model import MDModel
    from utils.metric_stats.loss_metric_stats import LossMetricStats
    SBModel = importlib.import_module(f"models.{recipe}.model").SBModel
    assert issubclass(SBModel, MDModel) and SBModel.dp_exact is True
    # test_gmm_vae makes its two loggers itself, whatever metric_keys says (as the reference);
    # test_h_vae's come from metric_keys
    mk = ["x.y"] if recipe == "test_gmm_vae" else keys
    m = SBModel(modules={}, hparams={"metric_keys": mk, "output_dir": str(tmp_path)}, run_opts={"device": "cpu"})
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        m.on_stage_start(stage, 1)
        assert set(m.stats_loggers) == {k + "_stats" for k in keys}
        assert all(isinstance(s, LossMetricStats) for s in m.stats_loggers.values())


@pytest.mark.parametrize("recipe", ["test_gmm_vae", "test_h_vae"])
def test_fused_engine_declines_the_recipe(recipe):
    import importlib
    _, m, _ = _resolve(recipe)
    SBModel = importlib.import_module(f"models.{recipe}.model").SBModel
    b = SBModel(modules=m["modules"], hparams=dict(m), run_opts={"device": "cpu"})
    assert b._fused_candidate(b._optimizer_infos()) is None


@pytest.mark.parametrize("recipe", ["test_gmm_vae", "test_h_vae"])
def test_fixture_contents(recipe):
    path = os.path.join(GOLD, recipe + "_tiny.npz")
    assert os.path.getsize(path) < 300 * 1024
    d = np.load(path)
    meta = json.loads(str(d["meta_json"]))
    assert meta["B"] == 3 and len(set(d["feat_lens"].tolist())) == 3  # three unequal lengths
    if meta["quirk_len"]:  # one length whose fp32 product with T lands above the frame count
        T = meta["T"]
        assert any(float(np.float32(l) * np.float32(T)) > round(float(l) * T) for l in d["feat_lens"])
    for name in ("TRAIN", "TEST"):
        assert f"{name}/loss" in d.files and any(k.startswith(f"{name}/loss/") for k in d.files)
    with_grad = [n for n in meta["param_names"] if n not in meta["none_grads"]]
    assert with_grad and all(f"TRAIN/grad/{n}" in d.files for n in with_grad)
    if recipe == "test_h_vae":
        assert meta["none_grads"] and all(n.startswith("pi_fc.") for n in meta["none_grads"])
        labels = d["pi_labels"]
        assert 0 < labels.sum() < labels.size


def test_latent_ops_check_their_arguments_before_any_launch():
    from mlvae_hip import ops
    B, T, N, Z = 2, 3, 3, 4
    ml, P, pi = torch.zeros(B, T, 2 * Z), torch.zeros(B, T, 4 * N * Z + N), torch.zeros(B, T, 2)
    eps_v, eps_g, expo = torch.zeros(B, T, Z), torch.zeros(B, T, N * Z), torch.ones(B, T, N)
    with pytest.raises(ValueError, match=r"N must be in \[1, 64\]"):
        ops.hvae_latent(ml, P, pi, eps_v, eps_g, expo, 65, Z, 0.1, 0)
    with pytest.raises(ValueError, match="stacked heads need"):
        ops.hvae_latent(ml, P[..., :-1], pi, eps_v, eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="eps_g"):
        ops.hvae_latent(ml, P, pi, eps_v, eps_g[..., :-1], expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="expo"):
        ops.hvae_latent(ml, P, pi, eps_v, eps_g, expo[:1], N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="are required"):
        ops.hvae_latent(None, P, pi, eps_v, eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="are required"):
        ops.hvae_latent(ml, P, None, eps_v, eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="ml "):
        ops.hvae_latent(ml[..., :-1], P, pi, eps_v, eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="pi "):
        ops.hvae_latent(ml, P, pi[..., :1], eps_v, eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="eps_v"):
        ops.hvae_latent(ml, P, pi, eps_v[..., :-1], eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match="stacked heads need"):
        ops.gmm_collapsed(P[..., :-1], eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(ValueError, match=r"N must be in \[1, 64\]"):
        ops.gmm_collapsed(P, eps_g, expo, 0, Z, 0.1, 0)
    # good shapes on the host: refused by the HIP path itself, which has no CPU fallback
    with pytest.raises(TypeError, match="float32 HIP tensor"):
        ops.hvae_latent(ml, P, pi, eps_v, eps_g, expo, N, Z, 0.1, 0)
    with pytest.raises(TypeError, match="float32 HIP tensor"):
        ops.gmm_collapsed(P, eps_g, expo, N, Z, 0.1, 0)
