"""The MD-VAE recipe (models/MD_VAE) on the HIP path.

* compute_forward + compute_objectives against the reference's own numbers
  (tests/golden/md_vae_tiny.npz, make_golden_md_recipe.py) under the four targets, fp32, with the
  recorded noise injected through ``SBModel.noise``: every mean loss, the total and pi_logits at
  1e-5 relative-max, sampled_pi and the three decoded sequences exactly, parameter gradients at
  1e-4 relative-max, and ``.grad is None`` where the reference has no gradient.
* train.py / test.py end to end on the synthetic corpus with MD labels: the three targets in
  order, metrics and the checkpoint at epoch 3 only, test metrics and the saved MD results.
Reference ops: ref:src/models/MD_VAE/model.py:31-273."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import PKG
from gpu_utils import need_gpu, rel_err

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "md_vae_tiny.npz")
KEYS = ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "pi_nll_loss",
        "vae_kld_loss", "recon_loss", "plvl_md", "boundary"]


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLD)
    return {k: d[k] for k in d.files}


def _modules(meta):
    from modules.boundary_detector import BoundaryDetector
    from modules.decoder import Decoder
    from modules.fc_block import FCBlock
    from modules.h_vae import HierarchicalVAE
    from modules.lstm import LSTM
    from modules.phoneme_recognizer import PhonemeRecognizer
    F, H, n_ph, Z, NC = meta["F"], meta["H"], meta["n_phonemes"], meta["Z"], meta["NC"]
    return {
        "feat_fc": FCBlock([F, H, H], end_activation=True),
        "phoneme_recognizer": PhonemeRecognizer(F, H, 2, [H, H, H, n_ph + 2], n_ph),
        "phn_recog_fc": FCBlock([n_ph + 2, H, H], end_activation=True),
        "boundary_detector": BoundaryDetector(F, H, 2, [H, H, H, 1]),
        "concat_fc": FCBlock([2 * H, H, H], end_activation=True),
        "rnn": LSTM(input_size=H, hidden_size=H, num_layers=2, batch_first=True, dropout=0.0),
        "pi_fc": FCBlock([H, H, H // 2, 2]),
        "encoder": HierarchicalVAE([H, H, H], Z, NC),
        "decoder": Decoder(Z, H, 2, 0.0, [2 * H, H, H, F]),
    }


def _model(gold, tmp_path):
    from models.MD_VAE.model import SBModel
    meta = json.loads(str(gold["meta_json"]))
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1),
                   normalizer=lambda feats, lens, epoch=None: feats,  # the fixture's: identity
                   batch_size=meta["batch_size"], metric_keys=KEYS, output_dir=str(tmp_path),
                   dataset_name=str(tmp_path / "ds"), model_name="md_vae_tiny", **meta["weights"])
    m = SBModel(modules=_modules(meta), hparams=hparams, run_opts={"device": "cuda:0"})
    state = {n: torch.from_numpy(gold["param/" + n]) for n in meta["param_names"]}
    assert [n for n, _ in m.modules.named_parameters()] == meta["param_names"]
    m.modules.load_state_dict(state)
    # pi_u replays the recorded Categorical.sample labels: label = (u >= p0)
    pi_u = torch.where(torch.from_numpy(gold["pi_labels"]) == 1, 1.0 - 2.0 ** -24, 0.0)
    m.noise = {"boundary_u": torch.from_numpy(gold["boundary_u"]).cuda(), "pi_u": pi_u.float().cuda(),
               "eps_v": torch.from_numpy(gold["eps_v"]).cuda(), "eps_g": torch.from_numpy(gold["eps_g"]).cuda(),
               "expo": torch.from_numpy(gold["expo"]).cuda()}
    return m, meta


def _batch(gold, meta):
    from brain.dataio import PaddedBatch
    t = lambda k: torch.from_numpy(gold[k])
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    fl, sl = t("feat_lens"), t("seq_lens")
    b.update({"id": [f"utt{i}" for i in range(meta["B"])], "feat": (t("feat"), fl),
              "gt_cnncl_seq": (t("gt_cnncl_seq"), sl), "fa_boundary_seq": (t("fa_boundary_seq"), fl),
              "gt_boundary_seq": (t("gt_boundary_seq"), fl),
              "plvl_gt_md_lbl_seq": (t("plvl_gt_md_lbl_seq"), sl),
              "prior": (t("prior"), torch.ones(meta["B"]))})
    return b


def _pad(seqs, n):
    return np.stack([np.pad(np.asarray(s, dtype=np.int64), (0, n - len(s)), constant_values=-1)
                     for s in seqs])


def _run(m, batch, stage, name, gold, meta):
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
    if name in ("VAE", "TEST"):
        e = rel_err(pred["pi_logits"], torch.from_numpy(gold[name + "/pi_logits"]))
        print(f"{name} pi_logits rel {e:.2e}")
        assert e < 1e-5
        assert np.array_equal(pred["sampled_pi"].cpu().numpy(), gold[name + "/sampled_pi"])
        assert pred["losses"]["pi_nll_loss"].shape == (meta["B"], meta["T"])
        bnd, flvl, plvl = decoded_lists(*pred["decoded_device"])
        assert np.array_equal(_pad(bnd, meta["T"]), gold[name + "/decoded_boundary"])
        assert np.array_equal(_pad(flvl, meta["T"]), gold[name + "/decoded_flvl"])
        assert np.array_equal(_pad(plvl, meta["L"]), gold[name + "/decoded_plvl"])
        # the NLL read the labels where the decode left them
        assert np.array_equal(pred["decoded_device"][1].cpu().numpy(), gold[name + "/decoded_flvl"])
    return pred, total


@pytest.mark.parametrize("name", ["PHN_RECOG", "B_DETECTOR", "VAE"])
def test_train_targets_match_reference(gold, tmp_path, name):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = _model(gold, tmp_path)
    m.modules.train()
    m.target = Target[name]
    m.stats_loggers = {}
    pred, total = _run(m, _batch(gold, meta), Stage.TRAIN, name, gold, meta)
    # TRAIN materialises no host lists
    assert "decoded_boundary_seq" not in pred and "decoded_plvl_md_lbl_seq" not in pred
    total.backward()
    m.on_stage_end(Stage.TRAIN, 0.0, 1)  # reads the error words; writes nothing in TRAIN
    none = set(meta["none_grads"][name])
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        if n in none:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        e = rel_err(p.grad, torch.from_numpy(gold[f"{name}/grad/{n}"]))
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (n, e)
    print(f"{name}: {len(none)} parameters without gradient, worst gradient {worst[0]} rel {worst[1]:.2e}")
    # the optimizer and the gradient clip skip the parameters without gradient
    from mlvae_hip.optim import Adam
    before = {n: p.detach().clone() for n, p in m.modules.named_parameters()}
    opt = Adam(m.modules.parameters(), lr=1e-3)
    assert m.check_gradients(total)
    opt.step()
    for n, p in m.modules.named_parameters():
        if n in none:
            assert torch.equal(p, before[n]), n
        elif bool(p.grad.ne(0).any()):
            assert not torch.equal(p, before[n]), n


def test_test_target_matches_reference(gold, tmp_path):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = _model(gold, tmp_path)
    m.modules.eval()
    m.on_stage_start(Stage.TEST, None)
    assert m.target == Target.TEST
    with torch.no_grad():
        pred, _ = _run(m, _batch(gold, meta), Stage.TEST, "TEST", gold, meta)
    assert [t.tolist() for t in pred["decoded_plvl_md_lbl_seq"]] == \
        [[v for v in row if v >= 0] for row in gold["TEST/decoded_plvl"].tolist()]
    assert m.stats_loggers["plvl_md_stats"].summarize() == json.loads(str(gold["TEST/md_summary_json"]))
    assert m.stats_loggers["boundary_stats"].summarize() == \
        json.loads(str(gold["TEST/boundary_summary_json"]))
    with open(tmp_path / "ds" / "saved_md_results" / "md_vae_tiny.json") as f:
        saved = json.load(f)
    want = json.loads(str(gold["TEST/saved_md_result_json"]))
    assert saved.keys() == want.keys()
    for k in want:
        assert len(saved[k]) == len(want[k])
        for a, b in zip(saved[k], want[k]):
            assert a[0] == b[0] and a[1:] == pytest.approx(b[1:], rel=1e-6)
    m.on_stage_end(Stage.TEST, 0.0, None)
    metrics = open(tmp_path / "test_output" / "test_metrics.txt").read()
    assert "plvl_md.F1" in metrics and "boundary.f1" in metrics


def test_decode_error_word_raises_at_stage_end(gold, tmp_path):
    """TRAIN leaves the decode's error word unread until on_stage_end: a set word raises the
    reference's AssertionError there."""
    need_gpu()
    from brain import Stage
    m, _ = _model(gold, tmp_path)
    m._decode_err = torch.tensor([8], device="cuda", dtype=torch.int32)
    with pytest.raises(AssertionError):
        m.on_stage_end(Stage.TRAIN, 0.0, 1)
    m.on_stage_end(Stage.TRAIN, 0.0, 1)  # the word is consumed


def _script(args, cwd):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    return subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=600)


def test_train_and_test_scripts(tmp_path):
    need_gpu()
    ds = tmp_path / "ds"
    overrides = ("{synthetic: {md_labels: true, n_train: 16, n_valid: 8, n_test: 8, min_frames: 40, "
                 "max_frames: 60}, model: {n_epochs: 3, phn_rnn_hidden_size: 64, "
                 "boundary_rnn_hidden_size: 64, rnn_hidden_size: 64, dec_rnn_hidden_size: 64, "
                 f"dataset_name: {ds}}}}}")
    common = ["config/run.yaml", "--model_class", "MD_VAE", "--model_name", "md_vae_ci",
              "--model", "!include:../models/MD_VAE/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    order = [log.index(f"Epoch {e}, stage TRAIN: target is {t}")
             for e, t in ((1, "PHN_RECOG"), (2, "B_DETECTOR"), (3, "VAE"))]
    assert order == sorted(order), log[-2000:]
    lines = [l for l in log.splitlines() if "plvl_md.F1" in l]
    assert len(lines) == 1 and lines[0].startswith("stage: valid, epoch: 3"), log[-2000:]
    assert "boundary.f1" in lines[0] and "valid pi_nll_loss.loss" in lines[0]
    assert len(os.listdir(tmp_path / "out" / "checkpoints")) >= 1
    r = _script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    assert "plvl_md.F1" in metrics and "boundary.f1" in metrics
    with open(ds / "saved_md_results" / "md_vae_ci.json") as f:
        saved = json.load(f)
    assert len(saved) == 8 and all(k.startswith("utt") for k in saved)
