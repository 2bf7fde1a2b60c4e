"""The upstream-module recipes (models/test_phn_classifier, models/test_b_ind_classifier) on the
HIP path, each against the reference's own numbers (tests/golden/test_*_classifier_tiny.npz,
make_golden_upstream.py), fp32:

* compute_forward + compute_objectives, TRAIN and TEST: the module output and the loss at 1e-5
  relative-max, every parameter gradient at 1e-4 (the bounds test_gpu_lstm_fc.py and
  test_gpu_md_vae.py hold these modules to in module mode); the boundary recipe's loss is the
  weighted sum of the masked means, formed here from the fixture's unreduced per-key losses with
  the golden mask rule (frame t valid iff t < len T); the chosen boundary frames exact;
* nothing comes to the host per batch (scores_list == []); summarize() equals the reference's
  recorded summary and the per-utterance scores equal its recorded scores;
* a bad gt_boundary_seq / a k > T_i does not raise in the batch: it raises in on_stage_end;
* train.py / test.py end to end on the synthetic corpus with md_labels and phn_labels.
Reference ops: ref:src/models/test_phn_classifier/model.py:17-64,
ref:src/models/test_b_ind_classifier/model.py:17-74."""
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
RECIPES = {
    "phn": dict(name="test_phn_classifier", module="phoneme_recognizer", stats="phn_acc_stats",
                keys=["phn_acc.flvl_acc", "phn_acc.plvl_acc"], out="out"),
    "bnd": dict(name="test_b_ind_classifier", module="boundary_detector", stats="boundary_stats",
                keys=["boundary.f1", "boundary.r_value"], out="boundary_v"),
}


def load_gold(which):
    d = np.load(os.path.join(GOLDEN, RECIPES[which]["name"] + "_tiny.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def gold_phn():
    return load_gold("phn")


@pytest.fixture(scope="module")
def gold_bnd():
    return load_gold("bnd")


def make_model(which, gold, tmp_path):
    import importlib
    r = RECIPES[which]
    SBModel = importlib.import_module(f"models.{r['name']}.model").SBModel
    meta = json.loads(str(gold["meta_json"]))
    H, F, N = meta["H"], meta["F"], meta["n_phonemes"]
    if which == "phn":
        from modules.phoneme_recognizer import PhonemeRecognizer
        mod = PhonemeRecognizer(input_size=F, rnn_hidden_size=H, rnn_num_layers=2,
                                fc_sizes=[H, H, H, N + 2], n_phonemes=N)
    else:
        from modules.boundary_detector import BoundaryDetector
        mod = BoundaryDetector(input_size=F, rnn_hidden_size=H, rnn_num_layers=2, fc_sizes=[H, H, H, 1])
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1),
                   normalizer=lambda feats, lens, epoch=None: feats, batch_size=meta["B"],
                   metric_keys=r["keys"], output_dir=str(tmp_path), **meta.get("weights", {}))
    m = SBModel(modules={r["module"]: mod}, hparams=hparams, run_opts={"device": "cuda:0"})
    assert [n for n, _ in m.modules.named_parameters()] == meta["param_names"]
    m.modules.load_state_dict({n: torch.from_numpy(gold["param/" + n]) for n in meta["param_names"]})
    if which == "bnd":
        m.noise = {"boundary_u": torch.from_numpy(gold["boundary_u"]).cuda()}
    return m, meta


def make_batch(gold, meta):
    from brain.dataio import PaddedBatch
    t = lambda k: torch.from_numpy(gold[k])
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    fl = t("feat_lens")
    b.update({"id": [f"utt{i}" for i in range(meta["B"])], "feat": (t("feat"), fl),
              "gt_cnncl_seq": (t("gt_cnncl_seq"), t("seq_lens")),
              "flvl_gt_cnncl_seq": (t("flvl_gt_cnncl_seq"), fl),
              "fa_boundary_seq": (t("fa_boundary_seq"), fl), "gt_boundary_seq": (t("gt_boundary_seq"), fl)})
    return b


def golden_loss(gold, name, meta):
    """sum_k weight_k * masked mean of the fixture's unreduced loss_k, in float64, under the
    golden mask rule: frame t of utterance b is valid iff t < feat_lens[b] * T (fp32 product)."""
    T = meta["T"]
    lim = torch.from_numpy(gold["feat_lens"]) * T
    mask = (torch.arange(T, dtype=torch.float32)[None, :] < lim[:, None]).double()
    total = 0.0
    for key in ("boundary_bce_loss", "boundary_kld_loss"):
        w = meta["weights"].get(key.replace("_loss", "_weight"), 1)
        le = torch.from_numpy(gold[f"{name}/loss/{key}"]).double()
        total += w * float((le * mask).sum() / mask.sum())
    return total


def check_scores(st, gold, name):
    assert st.scores_list == []  # nothing brought to the host per batch
    assert st.summarize() == json.loads(str(gold[name + "/summary_json"]))
    want = json.loads(str(gold[name + "/scores_json"]))
    assert len(st.scores_list) == len(want)
    for got, ref in zip(st.scores_list, want):
        assert {k: float(v) for k, v in got.items()} == ref
    print(f"{name}: {st.summarize()}")


def run_stage(which, m, batch, stage, name, gold, meta):
    r = RECIPES[which]
    m.on_stage_start(stage, 1)
    pred = m.compute_forward(batch, stage)
    loss = m.compute_objectives(pred, batch, stage)
    e_out = rel_err(pred[r["out"]], torch.from_numpy(gold[f"{name}/{r['out']}"]))
    want = float(gold[name + "/loss"])
    e_loss = abs(float(loss.detach()) - want) / abs(want)
    print(f"{which} {name}: {r['out']} rel {e_out:.2e}, loss {float(loss.detach()):.7f} ref {want:.7f} "
          f"rel {e_loss:.2e}")
    assert e_out < 1e-5 and e_loss < 1e-5
    if which == "bnd":
        # the recorded total is the weighted sum of the masked means of the recorded unreduced losses
        formed = golden_loss(gold, name, meta)
        assert abs(formed - want) <= 1e-6 * abs(want), (formed, want)
        assert abs(float(loss.detach()) - formed) < 1e-5 * abs(formed)
        assert np.array_equal(pred["pred_boundary_seq"].cpu().numpy(), gold[name + "/pred_boundary_seqs"])
    check_scores(m.stats_loggers[r["stats"]], gold, name)
    return pred, loss


@pytest.mark.parametrize("which", ["phn", "bnd"])
def test_train_matches_reference(which, gold_phn, gold_bnd, tmp_path):
    need_gpu()
    from brain import Stage
    gold = gold_phn if which == "phn" else gold_bnd
    m, meta = make_model(which, gold, tmp_path)
    m.modules.train()
    _, loss = run_stage(which, m, make_batch(gold, meta), Stage.TRAIN, "TRAIN", gold, meta)
    loss.backward()
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        assert p.grad is not None, n
        e = rel_err(p.grad, torch.from_numpy(gold[f"TRAIN/grad/{n}"]))
        print(f"{which} TRAIN grad {n} rel {e:.2e}")
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (n, e)
    print(f"{which} TRAIN: worst gradient {worst[0]} rel {worst[1]:.2e}")
    from mlvae_hip import ops
    ops.raise_score_err()  # what on_stage_end reads: no error bit to raise


@pytest.mark.parametrize("which", ["phn", "bnd"])
def test_test_matches_reference(which, gold_phn, gold_bnd, tmp_path):
    need_gpu()
    from brain import Stage
    gold = gold_phn if which == "phn" else gold_bnd
    m, meta = make_model(which, gold, tmp_path)
    m.modules.eval()
    with torch.no_grad():
        run_stage(which, m, make_batch(gold, meta), Stage.TEST, "TEST", gold, meta)
    m.on_stage_end(Stage.TEST, 0.0, None)
    metrics = open(tmp_path / "test_output" / "test_metrics.txt").read()
    for k in RECIPES[which]["keys"]:
        assert k in metrics, (k, metrics)


def test_phn_bad_boundaries_raise_at_the_stage_end(gold_phn, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = make_model("phn", gold_phn, tmp_path)
    m.modules.eval()
    b = make_batch(gold_phn, meta)
    gt = b["gt_boundary_seq"][0].clone()
    row = gt[1, :meta["lengths"][1]]
    row[int(torch.where(row == 0)[0][0])] = 1.0  # one flag too many in utterance 1
    b["gt_boundary_seq"] = (gt, b["feat"][1])
    m.on_stage_start(Stage.VALID, 1)
    with torch.no_grad():
        m.compute_objectives(m.compute_forward(b, Stage.VALID), b, Stage.VALID)  # no raise per batch
    with pytest.raises(AssertionError, match="one segment per phoneme"):
        m.on_stage_end(Stage.VALID, 0.0, 1)


def test_b_ind_k_past_the_length_raises_at_the_stage_end(gold_bnd, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = make_model("bnd", gold_bnd, tmp_path)
    m.modules.eval()
    b = make_batch(gold_bnd, meta)
    fa = b["fa_boundary_seq"][0].clone()
    fa[2, :] = 1.0  # T ones in the padded row of the shortest utterance: k = T > T_2
    b["fa_boundary_seq"] = (fa, b["feat"][1])
    m.on_stage_start(Stage.VALID, 1)
    with torch.no_grad():
        m.compute_objectives(m.compute_forward(b, Stage.VALID), b, Stage.VALID)  # no raise per batch
    with pytest.raises(RuntimeError, match="k out of range"):
        m.on_stage_end(Stage.VALID, 0.0, 1)


@pytest.mark.parametrize("which", ["phn", "bnd"])
def test_train_and_test_scripts(which, tmp_path):
    need_gpu()
    r = RECIPES[which]
    overrides = ("{synthetic: {md_labels: true, phn_labels: true, n_train: 16, n_valid: 8, n_test: 8, "
                 "min_frames: 40, max_frames: 60}, model: {n_epochs: 1, rnn_hidden_size: 16}}")
    common = ["config/run.yaml", "--model_class", r["name"], "--model_name", which + "_ci",
              "--model", f"!include:../models/{r['name']}/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    res = _script(["train.py"] + common, PKG)
    assert res.returncode == 0, res.stderr[-3000:]  # the run stops here: test.py is not started
    log = open(tmp_path / "out" / "train_log.txt").read()
    lines = [l for l in log.splitlines() if r["keys"][0] in l]
    assert len(lines) == 2, log[-2000:]  # TRAIN and VALID both score, as the reference
    assert lines[0].startswith("stage: train, epoch: 1") and lines[1].startswith("stage: valid, epoch: 1")
    for key in r["keys"]:
        assert f"train {key}" in lines[0] and f"valid {key}" in lines[1], (key, lines)
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1
    if which == "phn":
        from modules.phoneme_recognizer import PhonemeRecognizer
        mod = PhonemeRecognizer(input_size=120, rnn_hidden_size=16, rnn_num_layers=2,
                                fc_sizes=[16, 128, 128, 41], n_phonemes=39)
    else:
        from modules.boundary_detector import BoundaryDetector
        mod = BoundaryDetector(input_size=120, rnn_hidden_size=16, rnn_num_layers=2, fc_sizes=[16, 128, 128, 1])
    mod.load_state_dict(torch.load(os.path.join(ckpts[0], r["module"] + ".ckpt"), weights_only=True))  # strict
    assert all(bool(torch.isfinite(p).all()) for p in mod.parameters())
    res = _script(["test.py"] + common, PKG)
    assert res.returncode == 0, res.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    for key in r["keys"]:
        assert key in metrics, (key, metrics)
