"""The joint MD-VAE recipes (models/MD_VAE_joint, models/MD_VAE_joint_ll) on the HIP path.

* compute_forward + compute_objectives against the reference's own numbers
  (tests/golden/md_vae_joint_tiny.npz, md_vae_joint_ll_tiny.npz, make_golden_md_joint.py) at TRAIN
  and TEST, fp32, with the recorded noise injected through ``SBModel.noise``, once with each
  upstream module running its own recurrence and once with the paired one (``pair_upstream``):
  the bounds of tests/test_gpu_md_vae.py -- mean losses, total and pi_logits at 1e-5 relative-max,
  sampled_pi and the decoded sequences exactly, gradients at 1e-4 relative-max, ``.grad is None``
  exactly on the fixture's parameters without gradient.
* train.py / test.py end to end on the synthetic corpus: MD_VAE_joint evaluates and checkpoints at
  VALID of epoch 10 only; MD_VAE_joint_ll in every epoch.
Reference ops: ref:src/models/MD_VAE_joint/model.py:23-182, ref:src/models/MD_VAE_joint_ll/model.py:22-185."""
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

import test_gpu_md_vae as MD
from conftest import PKG
from gpu_utils import need_gpu, rel_err

pytestmark = pytest.mark.gpu

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECIPES = {
    "MD_VAE_joint": dict(gold="md_vae_joint_tiny.npz", model_name="md_vae_joint_tiny",
                         keys=["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "vae_kld_loss",
                               "recon_loss", "plvl_md", "boundary.f1", "boundary.r_value"]),
    "MD_VAE_joint_ll": dict(gold="md_vae_joint_ll_tiny.npz", model_name="md_vae_joint_ll_tiny",
                            keys=["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "pi_nll_loss",
                                  "vae_kld_loss", "recon_loss", "plvl_md", "boundary.f1", "boundary.r_value"]),
}
_gold = {}


def load_gold(recipe):
    """The recipe's fixture, read once and shared (never modified)."""
    if recipe not in _gold:
        d = np.load(os.path.join(GOLD_DIR, RECIPES[recipe]["gold"]))
        _gold[recipe] = {k: d[k] for k in d.files}
    return _gold[recipe]


def make_model(recipe, gold, tmp_path, pair):
    spec = RECIPES[recipe]
    SBModel = importlib.import_module(f"models.{recipe}.model").SBModel
    meta = json.loads(str(gold["meta_json"]))
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1),
                   normalizer=lambda feats, lens, epoch=None: feats,  # the fixture's: identity
                   batch_size=meta["batch_size"], metric_keys=spec["keys"], output_dir=str(tmp_path),
                   dataset_name=str(tmp_path / "ds"), model_name=spec["model_name"],
                   pair_upstream=pair, **meta["weights"])
    m = SBModel(modules=MD._modules(meta), hparams=hparams, run_opts={"device": "cuda:0"})
    assert [n for n, _ in m.modules.named_parameters()] == meta["param_names"]
    m.modules.load_state_dict({n: torch.from_numpy(gold["param/" + n]) for n in meta["param_names"]})
    # pi_u replays the recorded Categorical.sample labels: label = (u >= p0)
    pi_u = torch.where(torch.from_numpy(gold["pi_labels"]) == 1, 1.0 - 2.0 ** -24, 0.0)
    m.noise = {"boundary_u": torch.from_numpy(gold["boundary_u"]).cuda(), "pi_u": pi_u.float().cuda(),
               "eps_v": torch.from_numpy(gold["eps_v"]).cuda(), "eps_g": torch.from_numpy(gold["eps_g"]).cuda(),
               "expo": torch.from_numpy(gold["expo"]).cuda()}
    return m, meta


def _count_pairs(monkeypatch):
    from mlvae_hip import ops
    calls = []
    orig = ops.lstm_pair
    monkeypatch.setattr(ops, "lstm_pair", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    return calls


def _run(m, batch, stage, name, gold, meta, decoded):
    from utils.decode_utils import decoded_lists
    means = {}
    orig = m.compute_and_save_losses
    m.compute_and_save_losses = lambda losses: (means.update(losses), orig(losses))[1]
    try:
        pred = m.compute_forward(batch, stage)
        total = m.compute_objectives(pred, batch, stage)
    finally:
        del m.compute_and_save_losses
    want = {k[len(name) + 6:]: v for k, v in gold.items() if k.startswith(name + "/loss/")}
    assert set(means) == set(want)
    for k, v in want.items():
        e = rel_err(means[k], torch.from_numpy(v))
        print(f"{name} {k}: {float(means[k].detach()):.7f} ref {float(v):.7f} rel {e:.2e}")
        assert e < 1e-5, k
    e = rel_err(total, torch.from_numpy(gold[name + "/total"]))
    print(f"{name} total rel {e:.2e}")
    assert e < 1e-5
    e = rel_err(pred["pi_logits"], torch.from_numpy(gold[name + "/pi_logits"]))
    print(f"{name} pi_logits rel {e:.2e}")
    assert e < 1e-5
    assert np.array_equal(pred["sampled_pi"].cpu().numpy(), gold[name + "/sampled_pi"])
    assert ("decoded_device" in pred) == decoded
    if decoded:
        bnd, flvl, plvl = decoded_lists(*pred["decoded_device"])
        assert np.array_equal(MD._pad(bnd, meta["T"]), gold[name + "/decoded_boundary"])
        assert np.array_equal(MD._pad(flvl, meta["T"]), gold[name + "/decoded_flvl"])
        assert np.array_equal(MD._pad(plvl, meta["L"]), gold[name + "/decoded_plvl"])
    return pred, total


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("recipe", list(RECIPES))
def test_train_matches_reference(recipe, pair, tmp_path, monkeypatch):
    need_gpu()
    from brain import Stage
    gold = load_gold(recipe)
    m, meta = make_model(recipe, gold, tmp_path, pair)
    calls = _count_pairs(monkeypatch)
    m.modules.train()
    m.on_stage_start(Stage.TRAIN, 1)
    assert m.stats_loggers == {}
    ll = recipe == "MD_VAE_joint_ll"
    pred, total = _run(m, MD._batch(gold, meta), Stage.TRAIN, "TRAIN", gold, meta, decoded=ll)
    assert len(calls) == (1 if pair else 0)
    assert ("pi_nll_loss" in pred["losses"]) == ll
    if ll:  # the NLL read the labels where the decode left them
        assert np.array_equal(pred["decoded_device"][1].cpu().numpy(), gold["TRAIN/decoded_flvl"])
    # TRAIN materialises no host lists
    assert "decoded_boundary_seq" not in pred and "decoded_plvl_md_lbl_seq" not in pred
    total.backward()
    m.on_stage_end(Stage.TRAIN, 0.0, 1)  # reads the error words; writes nothing in TRAIN
    assert not (tmp_path / "ds").exists()
    none = set(meta["none_grads"]["TRAIN"])
    assert none and all(n.startswith(("phoneme_recognizer.", "boundary_detector.") if ll else "pi_fc.")
                        for n in none)
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        if n in none:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        e = rel_err(p.grad, torch.from_numpy(gold[f"TRAIN/grad/{n}"]))
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (n, e)
    print(f"{recipe} pair={pair}: {len(none)} parameters without gradient, worst gradient {worst[0]} "
          f"rel {worst[1]:.2e}")


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("recipe", list(RECIPES))
def test_test_stage_matches_reference(recipe, pair, tmp_path, monkeypatch):
    need_gpu()
    from brain import Stage
    gold = load_gold(recipe)
    m, meta = make_model(recipe, gold, tmp_path, pair)
    calls = _count_pairs(monkeypatch)
    m.modules.eval()
    m.on_stage_start(Stage.TEST, None)
    with torch.no_grad():
        pred, _ = _run(m, MD._batch(gold, meta), Stage.TEST, "TEST", gold, meta, decoded=True)
    assert len(calls) == (1 if pair else 0)
    assert [t.tolist() for t in pred["decoded_plvl_md_lbl_seq"]] == \
        [[v for v in row if v >= 0] for row in gold["TEST/decoded_plvl"].tolist()]
    assert m.stats_loggers["plvl_md_stats"].summarize() == json.loads(str(gold["TEST/md_summary_json"]))
    assert m.stats_loggers["boundary_stats"].summarize() == \
        json.loads(str(gold["TEST/boundary_summary_json"]))
    saved_path = tmp_path / "ds" / "saved_md_results" / (RECIPES[recipe]["model_name"] + ".json")
    if recipe == "MD_VAE_joint":
        with open(saved_path) as f:
            saved = json.load(f)
        want = json.loads(str(gold["TEST/saved_md_result_json"]))
        assert saved.keys() == want.keys()
        for k in want:
            assert len(saved[k]) == len(want[k])
            for a, b in zip(saved[k], want[k]):
                assert a[0] == b[0] and a[1:] == pytest.approx(b[1:], rel=1e-6)
    else:
        assert "TEST/saved_md_result_json" not in gold and not saved_path.exists()
    m.on_stage_end(Stage.TEST, 0.0, None)
    metrics = open(tmp_path / "test_output" / "test_metrics.txt").read()
    assert "plvl_md.F1" in metrics and "boundary.f1" in metrics and "boundary.r_value" in metrics


def _scripts(tmp_path, recipe, model_name, n_epochs):
    ds = tmp_path / "ds"
    overrides = ("{synthetic: {md_labels: true, n_train: 16, n_valid: 8, n_test: 8, min_frames: 40, "
                 f"max_frames: 60}}, model: {{n_epochs: {n_epochs}, phn_rnn_hidden_size: 64, "
                 "boundary_rnn_hidden_size: 64, rnn_hidden_size: 64, dec_rnn_hidden_size: 64, "
                 f"pair_upstream: true, dataset_name: {ds}}}}}")
    common = ["config/run.yaml", "--model_class", recipe, "--model_name", model_name,
              "--model", f"!include:../models/{recipe}/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = MD._script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    r = MD._script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    assert "plvl_md.F1" in metrics and "boundary.f1" in metrics
    return log, ds


def test_joint_train_and_test_scripts(tmp_path):
    need_gpu()
    log, ds = _scripts(tmp_path, "MD_VAE_joint", "md_vae_joint_ci", 10)
    lines = [l for l in log.splitlines() if "plvl_md.F1" in l]
    assert len(lines) == 1 and lines[0].startswith("stage: valid, epoch: 10"), log[-2000:]
    assert "boundary.f1" in lines[0] and "valid recon_loss.loss" in lines[0]
    assert not any(l.startswith("stage: train") for l in log.splitlines())
    assert len(os.listdir(tmp_path / "out" / "checkpoints")) == 1
    # the 8 test utterances: scored (test_metrics.txt, checked above) and saved
    with open(ds / "saved_md_results" / "md_vae_joint_ci.json") as f:
        saved = json.load(f)
    assert len(saved) == 8 and all(k.startswith("utt") for k in saved)


def test_joint_ll_train_and_test_scripts(tmp_path):
    need_gpu()
    log, ds = _scripts(tmp_path, "MD_VAE_joint_ll", "md_vae_joint_ll_ci", 2)
    lines = [l for l in log.splitlines() if "valid pi_nll_loss.loss" in l]
    assert [l.split(" - ")[0] for l in lines] == ["stage: valid, epoch: 1", "stage: valid, epoch: 2"], log[-2000:]
    assert all("plvl_md.F1" in l for l in lines)
    assert not (ds / "saved_md_results").exists()
