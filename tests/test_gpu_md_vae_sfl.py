"""The MD_VAE_sfl recipe (models/MD_VAE_sfl) on the HIP path.

* compute_forward + compute_objectives against the reference's own numbers
  (tests/golden/md_vae_sfl_tiny.npz, make_golden_md_sfl.py), fp32, K = 3 draws, with the recorded
  noise injected through ``SBModel.noise``.  VAE target in train: every mean loss, the total and
  pi_logits at 1e-5 relative-max, the decoded sequences and every draw's labels exactly,
  parameter gradients at 1e-4 relative-max, ``.grad is None`` where the reference has none, and
  an Adam step that moves baseline_fc and pi_fc and leaves the parameters without gradient
  bit-equal.  TEST target in eval: K = 1 (the argmax), the losses, the MD and boundary summaries
  (soft_F1 among them), the saved MD results.  The bounds are test_gpu_md_vae.py's.
* train.py / test.py end to end with --model_class MD_VAE_sfl on the synthetic corpus with MD
  labels: epoch 3's valid line carries the score-function losses and plvl_md.soft_F1, the
  checkpoint restores baseline_fc, test.py writes the metrics and the saved MD results.
Reference ops: ref:src/models/MD_VAE_sfl/model.py:54-189."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import PKG
from gpu_utils import need_gpu, rel_err
from test_gpu_md_vae import _batch, _pad, _script

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "md_vae_sfl_tiny.npz")
KEYS = ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "pi_nll_loss", "vae_kld_loss",
        "recon_loss", "rif_loss", "entropy_loss", "baseline_loss", "plvl_md", "boundary"]


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
        "phn_recog_out_fc": FCBlock([n_ph + 2, H, H], end_activation=True),
        "boundary_detector": BoundaryDetector(F, H, 2, [H, H, H, 1]),
        "concat_fc": FCBlock([2 * H, H, H], end_activation=True),
        "rnn": LSTM(input_size=H, hidden_size=H, num_layers=2, batch_first=True, dropout=0.0),
        "pi_fc": FCBlock([H, H, H // 2, 2]),
        "encoder": HierarchicalVAE([H, H, H], Z, NC),
        "decoder": Decoder(Z, H, 2, 0.0, [2 * H, H, H, F]),
        "baseline_fc": FCBlock([H, H, H, 1]),
    }


def _model(gold, tmp_path, train):
    from models.MD_VAE_sfl.model import SBModel
    meta = json.loads(str(gold["meta_json"]))
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1),
                   normalizer=lambda feats, lens, epoch=None: feats,  # the fixture's: identity
                   batch_size=meta["batch_size"], metric_keys=KEYS, output_dir=str(tmp_path),
                   dataset_name=str(tmp_path / "ds"), model_name="md_vae_sfl_tiny",
                   pi_mcmc_num=meta["K"], **meta["weights"])
    m = SBModel(modules=_modules(meta), hparams=hparams, run_opts={"device": "cuda:0"})
    state = {n: torch.from_numpy(gold["param/" + n]) for n in meta["param_names"]}
    assert [n for n, _ in m.modules.named_parameters()] == meta["param_names"]
    m.modules.load_state_dict(state)
    k = slice(None) if train else slice(0, 1)  # eval: one pass, the first recorded noise set
    m.noise = {"boundary_u": torch.from_numpy(gold["boundary_u"]).cuda(),
               "eps_v": torch.from_numpy(gold["eps_v"][k]).cuda(),
               "eps_g": torch.from_numpy(gold["eps_g"][k]).cuda(),
               "expo": torch.from_numpy(gold["expo"][k]).cuda()}
    if train:  # pi_u replays the recorded Categorical.sample labels: label = (u >= p0)
        pi_u = torch.where(torch.from_numpy(gold["pi_labels"]) == 1, 1.0 - 2.0 ** -24, 0.0)
        m.noise["pi_u"] = pi_u.float().cuda()
    return m, meta


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
    assert set(means) == set(want) and {"rif_loss", "entropy_loss", "baseline_loss"} <= set(want)
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
    B, T = meta["B"], meta["T"]
    for k in ("pi_nll_loss", "rif_loss", "entropy_loss", "baseline_loss"):
        assert pred["losses"][k].shape == (B, T)
        e = rel_err(pred["losses"][k], torch.from_numpy(gold[f"{name}/frame/{k}"]))
        print(f"{name} per-frame {k} rel {e:.2e}")
        assert e < 1e-5, k
    assert pred["losses"]["recon_loss"].shape == (B, T, meta["F"])
    assert pred["losses"]["vae_kld_loss"].shape == (B, T, meta["Z"])
    e = rel_err(pred["baseline"], torch.from_numpy(gold[name + "/baseline"]))
    print(f"{name} baseline rel {e:.2e}")
    assert e < 1e-5
    # the last draw's labels [B, T], as the reference leaves them
    assert pred["sampled_pi"].shape == (B, T)
    assert np.array_equal(pred["sampled_pi"].cpu().numpy(), gold[name + "/sampled_pi"])
    bnd, flvl, plvl = decoded_lists(*pred["decoded_device"])
    assert np.array_equal(_pad(bnd, T), gold[name + "/decoded_boundary"])
    assert np.array_equal(_pad(flvl, T), gold[name + "/decoded_flvl"])
    assert np.array_equal(_pad(plvl, meta["L"]), gold[name + "/decoded_plvl"])
    assert np.array_equal(pred["decoded_device"][1].cpu().numpy(), gold[name + "/decoded_flvl"])
    return pred, total


def test_vae_target_matches_reference(gold, tmp_path):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = _model(gold, tmp_path, train=True)
    m.modules.train()
    m.target = Target.VAE
    m.stats_loggers = {}
    pred, total = _run(m, _batch(gold, meta), Stage.TRAIN, "VAE", gold, meta)
    K = meta["K"]
    draws = pred["sampled_pi_draws"].cpu()
    assert draws.shape == (K, meta["B"], meta["T"], 2)
    for k in range(K):  # every draw's labels
        assert np.array_equal(draws[k, ..., 1].numpy(), gold["pi_labels"][k].astype(np.float32)), k
        assert torch.equal(draws[k, ..., 0], 1 - draws[k, ..., 1])
    assert "decoded_boundary_seq" not in pred  # TRAIN materialises no host lists
    total.backward()
    m.on_stage_end(Stage.TRAIN, 0.0, 1)  # reads the error words; writes nothing in TRAIN
    none = set(meta["none_grads"]["VAE"])
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        if n in none:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        e = rel_err(p.grad, torch.from_numpy(gold[f"VAE/grad/{n}"]))
        if n.startswith(("pi_fc.", "baseline_fc.")):
            print(f"VAE grad {n} rel {e:.2e}")
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (n, e)
    print(f"VAE: {len(none)} parameters without gradient, worst gradient {worst[0]} rel {worst[1]:.2e}")
    from mlvae_hip.optim import Adam
    before = {n: p.detach().clone() for n, p in m.modules.named_parameters()}
    opt = Adam(m.modules.parameters(), lr=1e-3)
    assert m.check_gradients(total)
    opt.step()
    for n, p in m.modules.named_parameters():
        if n in none:
            assert torch.equal(p, before[n]), n
        elif n.startswith(("pi_fc.", "baseline_fc.")) or bool(p.grad.ne(0).any()):
            assert not torch.equal(p, before[n]), n


def test_test_target_matches_reference(gold, tmp_path):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = _model(gold, tmp_path, train=False)
    m.modules.eval()
    m.on_stage_start(Stage.TEST, None)
    assert m.target == Target.TEST
    with torch.no_grad():
        pred, _ = _run(m, _batch(gold, meta), Stage.TEST, "TEST", gold, meta)
    assert pred["sampled_pi_draws"].shape == (1, meta["B"], meta["T"], 2)  # K = 1: the argmax
    assert torch.equal(pred["sampled_pi"], torch.argmax(pred["pi_logits"], -1).float())
    assert [t.tolist() for t in pred["decoded_plvl_md_lbl_seq"]] == \
        [[v for v in row if v >= 0] for row in gold["TEST/decoded_plvl"].tolist()]
    md = m.stats_loggers["plvl_md_stats"].summarize()
    assert "soft_F1" in md and md == json.loads(str(gold["TEST/md_summary_json"]))
    assert m.stats_loggers["boundary_stats"].summarize() == \
        json.loads(str(gold["TEST/boundary_summary_json"]))
    with open(tmp_path / "ds" / "saved_md_results" / "md_vae_sfl_tiny.json") as f:
        saved = json.load(f)
    want = json.loads(str(gold["TEST/saved_md_result_json"]))
    assert saved.keys() == want.keys()
    for k in want:
        assert len(saved[k]) == len(want[k])
        for a, b in zip(saved[k], want[k]):
            assert a[0] == b[0] and a[1:] == pytest.approx(b[1:], rel=1e-6)
    m.on_stage_end(Stage.TEST, 0.0, None)
    metrics = open(tmp_path / "test_output" / "test_metrics.txt").read()
    assert "plvl_md.soft_F1" in metrics and "rif_loss.loss" in metrics and "baseline_loss.loss" in metrics


def test_train_and_test_scripts(tmp_path):
    need_gpu()
    ds = tmp_path / "ds"
    overrides = ("{synthetic: {md_labels: true, n_train: 16, n_valid: 8, n_test: 8, min_frames: 40, "
                 "max_frames: 60}, model: {n_epochs: 3, pi_mcmc_num: 2, phn_rnn_hidden_size: 64, "
                 "boundary_rnn_hidden_size: 64, rnn_hidden_size: 64, dec_rnn_hidden_size: 64, "
                 f"dataset_name: {ds}}}}}")
    common = ["config/run.yaml", "--model_class", "MD_VAE_sfl", "--model_name", "md_vae_sfl_ci",
              "--model", "!include:../models/MD_VAE_sfl/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    order = [log.index(f"Epoch {e}, stage TRAIN: target is {t}")
             for e, t in ((1, "PHN_RECOG"), (2, "B_DETECTOR"), (3, "VAE"))]
    assert order == sorted(order), log[-2000:]
    lines = [l for l in log.splitlines() if "plvl_md.soft_F1" in l]
    assert len(lines) == 1 and lines[0].startswith("stage: valid, epoch: 3"), log[-2000:]
    for key in ("rif_loss.loss", "entropy_loss.loss", "baseline_loss.loss", "pi_nll_loss.loss"):
        assert f"valid {key}" in lines[0], (key, lines[0])
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1
    from modules.fc_block import FCBlock
    fc = FCBlock([64, 16, 16, 1])
    state = torch.load(os.path.join(ckpts[0], "baseline_fc.ckpt"), weights_only=True)
    fc.load_state_dict(state)  # strict: every key and shape of baseline_fc
    assert all(bool(torch.isfinite(p).all()) for p in fc.parameters())
    r = _script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    assert "plvl_md.soft_F1" in metrics and "rif_loss.loss" in metrics
    with open(ds / "saved_md_results" / "md_vae_sfl_ci.json") as f:
        saved = json.load(f)
    assert len(saved) == 8 and all(k.startswith("utt") for k in saved)
