"""The single-encoder VAE recipes (models/test_gmm_vae, models/test_h_vae) on the HIP path, each
against the reference's own numbers (tests/golden/test_gmm_vae_tiny.npz, test_h_vae_tiny.npz,
make_golden_vae_recipes.py), fp32, with ``fused_latent`` off and on:

* compute_forward + compute_objectives, TRAIN and TEST (the argmax pi): the loss and every per-key
  loss at 1e-5, gmm_weight exactly, every parameter gradient at 1e-4 relative-max (the bounds of
  test_gpu_upstream_recipes.py), ``.grad is None`` where the reference has no gradient;
* test_h_vae: pi_fc has no gradient and comes through fit_batch bit-unchanged while every other
  module moves; a checkpoint round trip through the yaml's recoverables restores rnn and pi_fc;
* train.py / test.py end to end on the plain synthetic corpus, one tiny epoch.
Reference ops: ref:src/models/test_gmm_vae/model.py:17-65, ref:src/models/test_h_vae/model.py:13-66."""
import functools
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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECIPES = {"gmm": "test_gmm_vae", "hvae": "test_h_vae"}
KEYS = {"gmm": ["kld_loss", "recon_loss"], "hvae": ["vae_kld_loss", "recon_loss"]}
CASES = [(w, f) for w in RECIPES for f in (False, True)]


def load_gold(which):
    d = np.load(os.path.join(GOLDEN, RECIPES[which] + "_tiny.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def golds():
    return {w: load_gold(w) for w in RECIPES}


def make_modules(which, meta, fused):
    from modules.decoder import Decoder
    F, H, E, Z, NC = meta["F"], meta["H"], meta["E"], meta["Z"], meta["NC"]
    dec = lambda: Decoder(Z, H, 2, 0.0, [2 * H, E, E, F])
    if which == "gmm":
        from modules.gmm_vae import GMMVAE
        return {"encoder": GMMVAE([F, E, E], Z, NC), "decoder": dec()}
    from modules.fc_block import FCBlock
    from modules.h_vae import HierarchicalVAE
    from modules.lstm import LSTM
    return {"rnn": LSTM(input_size=F, hidden_size=H, num_layers=2, batch_first=True, dropout=0.0),
            "pi_fc": FCBlock([H, H, H // 2, 2]),
            "encoder": HierarchicalVAE([H, E, E], Z, NC, fused=fused), "decoder": dec()}


def make_model(which, gold, tmp_path, fused, **extra):
    import importlib
    SBModel = importlib.import_module(f"models.{RECIPES[which]}.model").SBModel
    meta = json.loads(str(gold["meta_json"]))
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1),
                   normalizer=lambda feats, lens, epoch=None: feats, batch_size=meta["B"],
                   metric_keys=KEYS[which], output_dir=str(tmp_path), fused_latent=fused,
                   **meta["weights"], **extra)
    m = SBModel(modules=make_modules(which, meta, fused), hparams=hparams, run_opts={"device": "cuda:0"})
    assert [n for n, _ in m.modules.named_parameters()] == meta["param_names"]
    m.modules.load_state_dict({n: torch.from_numpy(gold["param/" + n]) for n in meta["param_names"]})
    t = lambda k: torch.from_numpy(gold[k]).cuda()
    if which == "gmm":
        m.noise = {"eps": t("eps"), "expo": t("expo")}
    else:
        # pi_u replays the recorded Categorical.sample labels: label = (u >= p0)
        pi_u = torch.where(torch.from_numpy(gold["pi_labels"]) == 1, 1.0 - 2.0 ** -24, 0.0)
        m.noise = {"pi_u": pi_u.float().cuda(), "eps_v": t("eps_v"), "eps_g": t("eps_g"), "expo": t("expo")}
    return m, meta


def make_batch(gold, meta):
    from brain.dataio import PaddedBatch
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    b.update({"id": [f"utt{i}" for i in range(meta["B"])],
              "feat": (torch.from_numpy(gold["feat"]), torch.from_numpy(gold["feat_lens"]))})
    return b


def run_stage(which, m, batch, stage, name, gold):
    means = {}
    orig = m.compute_and_save_losses
    m.compute_and_save_losses = lambda losses: (means.update(losses), orig(losses))[1]
    try:
        m.on_stage_start(stage, 1)
        pred = m.compute_forward(batch, stage)
        loss = m.compute_objectives(pred, batch, stage)
    finally:
        del m.compute_and_save_losses
    want = {k[len(name) + 6:]: v for k, v in gold.items() if k.startswith(name + "/loss/")}
    assert set(means) == set(want) == set(KEYS[which])
    for k, v in want.items():
        e = rel_err(means[k], torch.from_numpy(v))
        print(f"{which} {name} {k}: {float(means[k].detach()):.7f} ref {float(v):.7f} rel {e:.2e}")
        assert e < 1e-5, k
    e = rel_err(loss, torch.from_numpy(gold[name + "/loss"]))
    print(f"{which} {name} loss rel {e:.2e}")
    assert e < 1e-5
    assert np.array_equal(pred["encoder_out"]["gmm_weight"].detach().cpu().numpy(), gold[name + "/gmm_weight"])
    for key in KEYS[which]:  # the stats the stage made took the values
        assert len(m.stats_loggers[key + "_stats"].loss_list) == 1
    return pred, loss


@pytest.mark.parametrize("which,fused", CASES)
def test_train_matches_reference(which, fused, golds, tmp_path):
    need_gpu()
    from brain import Stage
    gold = golds[which]
    m, meta = make_model(which, gold, tmp_path, fused)
    m.modules.train()
    pred, loss = run_stage(which, m, make_batch(gold, meta), Stage.TRAIN, "TRAIN", gold)
    assert ("weighted_h" in pred["encoder_out"]) == (fused and which == "gmm")
    loss.backward()
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        if n in meta["none_grads"]:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        e = rel_err(p.grad, torch.from_numpy(gold[f"TRAIN/grad/{n}"]))
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (n, e)
    print(f"{which} fused={fused} TRAIN: worst gradient {worst[0]} rel {worst[1]:.2e}")
    if which == "hvae":
        assert meta["none_grads"] == [n for n in meta["param_names"] if n.startswith("pi_fc.")]
        assert np.array_equal(pred["sampled_pi"][..., 1].cpu().numpy(), gold["pi_labels"].astype(np.float32))


@pytest.mark.parametrize("which,fused", CASES)
def test_test_matches_reference(which, fused, golds, tmp_path):
    need_gpu()
    from brain import Stage
    gold = golds[which]
    m, meta = make_model(which, gold, tmp_path, fused)
    m.modules.eval()
    with torch.no_grad():
        pred, _ = run_stage(which, m, make_batch(gold, meta), Stage.TEST, "TEST", gold)
    if which == "hvae":  # the argmax pi, whatever pi_u says
        want = torch.from_numpy(gold["pi_logits"]).argmax(-1).float()
        assert torch.equal(pred["sampled_pi"][..., 1].cpu(), want)
    m.on_stage_end(Stage.TEST, 0.0, None)
    metrics = open(tmp_path / "test_output" / "test_metrics.txt").read()
    for k in KEYS[which]:
        assert k in metrics, (k, metrics)


@pytest.mark.parametrize("fused", [False, True])
def test_h_vae_pi_fc_is_left_alone_by_fit_batch(fused, golds, tmp_path):
    need_gpu()
    from brain import Stage
    from mlvae_hip import optim as hip_optim
    gold = golds["hvae"]
    m, meta = make_model("hvae", gold, tmp_path, fused, optimizer=functools.partial(hip_optim.Adam, lr=1e-3))
    m.init_optimizers()
    assert m.engine is None  # four modules: module mode
    m.modules.train()
    m.on_stage_start(Stage.TRAIN, 1)
    before = {n: p.detach().clone() for n, p in m.modules.named_parameters()}
    m.fit_batch(make_batch(gold, meta))
    torch.cuda.synchronize()
    for n, p in m.modules.named_parameters():
        if n.startswith("pi_fc."):
            assert torch.equal(p.detach(), before[n]), n
        else:
            assert not torch.equal(p.detach(), before[n]), n
    # and a backward alone leaves pi_fc without gradient
    m.compute_objectives(m.compute_forward(make_batch(gold, meta), Stage.TRAIN),
                         make_batch(gold, meta), Stage.TRAIN).backward()
    assert all(p.grad is None for p in m.modules["pi_fc"].parameters())
    assert all(p.grad is not None for p in m.modules["rnn"].parameters())


def test_h_vae_checkpoint_restores_rnn_and_pi_fc(golds, tmp_path):
    need_gpu()
    from hyperpyyaml import load_hyperpyyaml
    ov = ("dataset: synthetic\nmodel_class: test_h_vae\nmodel_name: ci\n"
          f"output_dir: {tmp_path}\nmodel: !include:../models/test_h_vae/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{"model": {"rnn_hidden_size": 16, "dec_rnn_hidden_size": 16}}, ov])
    mdl = hp["model"]
    ck = mdl["checkpointer"]
    saved = {k: {n: p.detach().clone() for n, p in mdl[k].named_parameters()} for k in ("rnn", "pi_fc", "encoder")}
    ck.save_checkpoint(meta={"loss": 1.0})
    with torch.no_grad():
        for k in saved:
            for p in mdl[k].parameters():
                p.add_(1.0)
    assert ck.recover_if_possible() is not None
    for k, params in saved.items():
        for n, p in mdl[k].named_parameters():
            assert torch.equal(p.detach().cpu(), params[n].cpu()), (k, n)
    ckpts = glob.glob(str(tmp_path / "checkpoints" / "CKPT+*"))
    assert len(ckpts) == 1 and os.path.exists(os.path.join(ckpts[0], "rnn.ckpt"))
    assert os.path.exists(os.path.join(ckpts[0], "pi_fc.ckpt"))


@pytest.mark.parametrize("which", ["gmm", "hvae"])
def test_train_and_test_scripts(which, tmp_path):
    need_gpu()
    name = RECIPES[which]
    sizes = "rnn_hidden_size: 16, " if which == "hvae" else ""
    overrides = ("{synthetic: {n_train: 16, n_valid: 8, n_test: 8, min_frames: 40, max_frames: 60}, "
                 f"model: {{n_epochs: 1, {sizes}dec_rnn_hidden_size: 16, fused_latent: true}}}}")
    common = ["config/run.yaml", "--model_class", name, "--model_name", which + "_ci",
              "--model", f"!include:../models/{name}/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    res = _script(["train.py"] + common, PKG)
    assert res.returncode == 0, res.stderr[-3000:]  # the run stops here: test.py is not started
    log = open(tmp_path / "out" / "train_log.txt").read()
    lines = [l for l in log.splitlines() if KEYS[which][0] in l]
    assert len(lines) == 2, log[-2000:]
    assert lines[0].startswith("stage: train, epoch: 1") and lines[1].startswith("stage: valid, epoch: 1")
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1
    want = {"encoder.ckpt", "decoder.ckpt"} | ({"rnn.ckpt", "pi_fc.ckpt"} if which == "hvae" else set())
    assert want <= set(os.listdir(ckpts[0])), os.listdir(ckpts[0])
    if which == "hvae":
        from modules.lstm import LSTM
        rnn = LSTM(input_size=120, hidden_size=16, num_layers=2, batch_first=True, dropout=0.15)
        rnn.load_state_dict(torch.load(os.path.join(ckpts[0], "rnn.ckpt"), weights_only=True))  # strict
        assert all(bool(torch.isfinite(p).all()) for p in rnn.parameters())
    res = _script(["test.py"] + common, PKG)
    assert res.returncode == 0, res.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    for key in KEYS[which]:
        assert key in metrics, (key, metrics)
