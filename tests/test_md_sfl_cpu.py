"""The MD_VAE_sfl recipe's host-side parts (no GPU):

* models/MD_VAE_sfl/model.yaml through load_hyperpyyaml with the top-level config, its key names
  against the reference yaml's (tests/golden/md_vae_sfl_yaml_keys.json; use_kaldi_feat is the one
  key not carried: the recipe reads `feat` through the normaliser);
* the target schedule, the evaluation gate and the loss stats of the new metric keys;
* ops.pi_sample_k / ops.sfl_losses argument checks, which raise before any launch;
* tests/golden/md_vae_sfl_tiny.npz is self-consistent: rif, entropy and baseline_loss recomputed
  in numpy fp64 from the recorded pi_logits, draws, per-draw loss means, pi_nll and baseline give
  the recorded per-frame values (fp32 arithmetic in the reference: 1e-5 relative-max), with the
  raw loss weights inside the reward."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "pi_nll_loss", "vae_kld_loss",
        "recon_loss", "rif_loss", "entropy_loss", "baseline_loss", "plvl_md", "boundary"]


# --------------------------------------------------------------------------- yaml
def test_model_yaml_resolves_with_the_reference_keys():
    import functools
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import optim as hip_optim
    from modules.fc_block import FCBlock
    from modules.lstm import LSTM
    ov = ("dataset: synthetic\nmodel_class: MD_VAE_sfl\nmodel_name: md_vae_sfl\n"
          "model: !include:../models/MD_VAE_sfl/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    m = hp["model"]
    with open(os.path.join(GOLD, "md_vae_sfl_yaml_keys.json")) as f:
        ref = json.load(f)
    assert "pi_mcmc_num" in ref["top_level"] and "baseline_fc" in ref["modules"]
    assert list(m["modules"].keys()) == ref["modules"]
    assert list(m["checkpointer"].recoverables.keys()) == ref["recoverables"]
    assert set(ref["top_level"]) - set(m.keys()) == {"use_kaldi_feat"}
    assert m["max_key"] == "plvl_md.soft_F1"
    assert m["metric_keys"] == KEYS
    assert m["pi_mcmc_num"] == 5
    for k in ("phn_recog_bce", "boundary_bce", "boundary_kld", "pi_nll", "vae_kld", "recon", "rif",
              "entropy", "baseline"):
        assert m[k + "_weight"] == 1, k
    assert isinstance(m["rnn"], LSTM) and m["rnn"].hidden_size == 512 and m["rnn"].dropout == 0.15
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    bl = m["baseline_fc"]
    assert isinstance(bl, FCBlock) and m["modules"]["baseline_fc"] is bl
    assert m["checkpointer"].recoverables["baseline_fc"] is bl
    lin = [b for b in bl.blocks if isinstance(b, torch.nn.Linear)]
    assert [(l.in_features, l.out_features) for l in lin] == [(512, 16), (16, 16), (16, 1)]
    assert m["phn_recog_out_fc"].blocks[0].in_features == hp["n_phonemes"] + 2
    assert m["pi_fc"].blocks[-1].out_features == 2
    assert m["epoch_counter"].limit == 50


# --------------------------------------------------------------------------- schedule
def test_target_schedule_and_evaluation_gate(tmp_path):
    from brain import Stage
    from models.MD_VAE.model import SBModel as MD_VAE
    from models.MD_VAE.model import Target
    from models.MD_VAE_sfl.model import SBModel
    assert issubclass(SBModel, MD_VAE) and SBModel.compute_forward is not MD_VAE.compute_forward
    m = SBModel(modules={}, hparams={"metric_keys": KEYS, "output_dir": str(tmp_path)},
                run_opts={"device": "cpu"})
    want = [Target.PHN_RECOG, Target.B_DETECTOR, Target.VAE] * 2
    for epoch in range(1, 7):
        for stage in (Stage.TRAIN, Stage.VALID):
            m.on_stage_start(stage, epoch)
            assert m.target == want[epoch - 1]
            evaluates = stage == Stage.VALID and want[epoch - 1] == Target.VAE
            assert m.to_run_evaluation(stage) == evaluates
            assert set(m.stats_loggers) == ({k + "_stats" for k in KEYS} if evaluates else set())
    m.on_stage_start(Stage.TEST, None)
    assert m.target == Target.TEST and m.to_run_evaluation(Stage.TEST)
    assert {"rif_loss_stats", "entropy_loss_stats", "baseline_loss_stats"} <= set(m.stats_loggers)


# --------------------------------------------------------------------------- ops argument checks
def _sfl_args(K=2, B=2, T=3, F=5, Z=4):
    z = torch.zeros
    return dict(logits=z(B, T, 2), sampled_pi=z(K, B, T, 2), recon=z(K, B, T, F), kld=z(K, B, T, Z),
                pi_nll=z(B, T), baseline=z(B, T))


def _sfl(a):
    from mlvae_hip import ops
    return ops.sfl_losses(a["logits"], a["sampled_pi"], a["recon"], a["kld"], a["pi_nll"], a["baseline"],
                          0.7, 0.3, 0.5)


def test_sfl_losses_argument_checks_raise_before_any_launch():
    bad = [("logits", torch.zeros(2, 3, 3)),          # not 2 classes
           ("sampled_pi", torch.zeros(2, 3, 2)),      # no leading K
           ("sampled_pi", torch.zeros(2, 2, 4, 2)),   # frames differ
           ("sampled_pi", torch.zeros(0, 2, 3, 2)),   # K = 0
           ("recon", torch.zeros(3, 2, 3, 5)),        # another K
           ("recon", torch.zeros(2, 2, 3, 0)),        # empty rows
           ("kld", torch.zeros(2, 2, 3)),             # no row axis
           ("pi_nll", torch.zeros(2, 3, 1)),
           ("baseline", torch.zeros(2, 4))]
    for name, t in bad:
        a = _sfl_args()
        a[name] = t
        with pytest.raises(ValueError, match="sfl_losses"):
            _sfl(a)
    # well-formed shapes off the device: the HIP path has no CPU fallback
    with pytest.raises(TypeError, match="HIP tensor"):
        _sfl(_sfl_args())
    a = _sfl_args()
    a["recon"] = a["recon"].double()
    with pytest.raises(TypeError, match="HIP tensor"):
        _sfl(a)


def test_pi_sample_k_argument_checks_raise_before_any_launch():
    from mlvae_hip import ops
    l = torch.zeros(2, 3, 2)
    with pytest.raises(ValueError, match="K must be"):
        ops.pi_sample_k(l, 0, True)
    with pytest.raises(ValueError, match="K must be"):
        ops.pi_sample_k(l, 2, False)  # eval is the argmax: one draw
    with pytest.raises(ValueError, match="2 classes"):
        ops.pi_sample_k(torch.zeros(2, 3, 4), 2, True)
    with pytest.raises(TypeError, match="HIP tensor"):
        ops.pi_sample_k(l, 2, True)


# --------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLD, "md_vae_sfl_tiny.npz"))
    return {k: d[k] for k in d.files}


def _recompute(gold, name, w_recon, w_kld, w_nll):
    """(rif, entropy, baseline_loss) [B,T] in fp64 from the recorded pieces."""
    l = gold[name + "/pi_logits"].astype(np.float64)
    lp = l - np.log(np.exp(l - l.max(-1, keepdims=True)).sum(-1, keepdims=True)) - l.max(-1, keepdims=True)
    p = np.exp(lp)
    if name == "VAE":
        labels = gold["pi_labels"]
    else:
        labels = l.argmax(-1)[None]
    K = labels.shape[0]
    recon = gold[name + "/draw_recon_mean"].astype(np.float64)
    kld = gold[name + "/draw_kld_mean"].astype(np.float64)
    assert recon.shape == kld.shape == labels.shape
    nll_pi = gold[name + "/frame/pi_nll_loss"].astype(np.float64)
    b = gold[name + "/baseline"].astype(np.float64)
    rif = np.zeros_like(b)
    bl = np.zeros_like(b)
    for k in range(K):
        reward = -(w_recon * recon[k] + w_kld * kld[k] + w_nll * nll_pi)
        nll = -np.take_along_axis(lp, labels[k][..., None], -1)[..., 0]
        rif += (reward - b) * nll
        bl += (b - reward) ** 2
    return rif / K, (p * lp).sum(-1), bl / K


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", ["VAE", "TEST"])
def test_fixture_is_self_consistent(gold, name):
    meta = json.loads(str(gold["meta_json"]))
    w = meta["weights"]
    assert meta["K"] == 3 and gold["pi_labels"].shape == (3, meta["B"], meta["T"])
    assert len({w[k] for k in ("recon_weight", "vae_kld_weight", "pi_nll_weight", "rif_weight",
                               "entropy_weight", "baseline_weight")}) == 6 and 1 not in w.values()
    got = _recompute(gold, name, w["recon_weight"], w["vae_kld_weight"], w["pi_nll_weight"])
    for key, g in zip(("rif_loss", "entropy_loss", "baseline_loss"), got):
        e = _rel(g, gold[f"{name}/frame/{key}"])
        print(f"{name} {key}: recomputed against recorded, rel {e:.2e}")
        assert e < 1e-5, key
    # the reward holds the raw vae_kld_weight: the total's 2249 / batch_size scaling inside it,
    # or two weights swapped, give other numbers
    scaled = _recompute(gold, name, w["recon_weight"], w["vae_kld_weight"] / (2249 / meta["batch_size"]),
                        w["pi_nll_weight"])
    swapped = _recompute(gold, name, w["vae_kld_weight"], w["recon_weight"], w["pi_nll_weight"])
    for other in (scaled, swapped):
        assert _rel(other[0], gold[f"{name}/frame/rif_loss"]) > 1e-3
        assert _rel(other[2], gold[f"{name}/frame/baseline_loss"]) > 1e-3


def test_fixture_draws_and_gradients(gold):
    meta = json.loads(str(gold["meta_json"]))
    lab = gold["pi_labels"]
    for k in range(meta["K"]):
        assert set(np.unique(lab[k]).tolist()) == {0, 1}
        assert all(not np.array_equal(lab[k], lab[j]) for j in range(k))
    assert np.array_equal(gold["VAE/sampled_pi"], lab[-1].astype(np.float32))  # the last draw's labels
    assert np.array_equal(gold["TEST/sampled_pi"], gold["TEST/pi_logits"].argmax(-1).astype(np.float32))
    gap = gold["VAE/pi_logits"][..., 1] - gold["VAE/pi_logits"][..., 0]
    assert 1.0 < gap.max() - gap.min() < 10.0  # a few units: softmax is not saturated
    assert np.abs(gold["VAE/grad/pi_fc.blocks.4.weight"]).max() > 1e-3
    assert np.abs(gold["VAE/grad/baseline_fc.blocks.0.weight"]).max() > 1e-3
    none = set(meta["none_grads"]["VAE"])
    assert none and all(n.startswith(("phoneme_recognizer.", "boundary_detector.")) for n in none)
    assert not any(n.startswith(("baseline_fc.", "pi_fc.", "rnn.")) for n in none)
