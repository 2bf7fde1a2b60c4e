"""The MD-VAE recipe's host-side parts (no GPU):

* utils/metric_stats/{md,boundary}_metric_stats.py against the reference's numbers
  (tests/golden/md_metrics.json, make_golden_md_metrics.py);
* SyntheticSet(md_labels=True): the invariants phn_bce, the decode and boundary_md_scoring
  assert, and md_labels=False leaving the features bit-identical;
* the target schedule of models/MD_VAE/model.py and to_run_evaluation;
* models/MD_VAE/model.yaml through load_hyperpyyaml with the top-level config, its key names
  against the reference yaml's (tests/golden/md_vae_yaml_keys.json)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# --------------------------------------------------------------------------- metrics
@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "md_metrics.json")) as f:
        return json.load(f)


def _close(got, want):
    assert set(got) == set(want)
    for k in want:
        # fp32 arithmetic in the reference's order; the tolerance is an fp32 ulp of a percentage
        assert float(got[k]) == pytest.approx(want[k], rel=1e-6, abs=1e-5), k


def test_per_utterance_scores_match_reference(gold):
    from utils.metric_stats.boundary_metric_stats import boundary_scoring
    from utils.metric_stats.md_metric_stats import binary_seq_md_scoring, boundary_md_scoring
    kinds = set()
    for u in gold["utterances"]:
        pb = np.asarray(u["pred_boundary"], dtype=np.int64)
        _close(binary_seq_md_scoring(u["pred_md"], u["gt_md"]), u["binary"])
        _close(boundary_md_scoring(pb, u["gt_boundary"], u["pred_md"], u["gt_md"]), u["boundary_md"])
        _close(boundary_scoring(pb, u["gt_boundary"]), u["boundary"])
        kinds.add("none" if not any(u["gt_md"]) else "all" if all(u["gt_md"]) else "mixed")
    assert kinds == {"none", "all", "mixed"}  # the fixture's edge utterances are there


def test_stats_summaries_match_reference(gold):
    from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
    from utils.metric_stats.md_metric_stats import MDMetricStats
    md, bnd = MDMetricStats(), BoundaryMetricStats()
    with pytest.raises(ValueError):
        md.summarize()
    for lo, hi in gold["batches"]:
        part = gold["utterances"][lo:hi]
        pbs = [np.asarray(u["pred_boundary"], dtype=np.int64) for u in part]
        md.append(ids=[u["id"] for u in part], pred_md_lbl_seqs=[u["pred_md"] for u in part],
                  gt_md_lbl_seqs=[u["gt_md"] for u in part], pred_boundary_seqs=pbs,
                  gt_boundary_seqs=[u["gt_boundary"] for u in part])
        bnd.append(ids=[u["id"] for u in part], predictions=pbs,
                   targets=[u["gt_boundary"] for u in part])
    # equality after the reference's own rounding (2 decimals; F1 from the mean PRE and REC)
    assert md.summarize() == gold["md_summary"]
    assert md.summarize("F1") == gold["md_F1"]
    assert bnd.summarize() == gold["boundary_summary"]
    assert bnd.summarize("f1") == gold["boundary_f1"]
    assert md.ids == [u["id"] for u in gold["utterances"]]
    assert md.saved_seqs["pred_md_lbl_seqs"] == [u["pred_md"] for u in gold["utterances"]]


def test_scoring_rejects_bad_input():
    from utils.metric_stats.boundary_metric_stats import batch_boundary_scoring
    from utils.metric_stats.md_metric_stats import batch_seq_md_scoring, binary_seq_md_scoring
    with pytest.raises(ValueError):
        binary_seq_md_scoring([0, 1, 2], [0, 1, 1])
    with pytest.raises(ValueError):
        binary_seq_md_scoring([0, 1], [0, 1, 1])
    with pytest.raises(TypeError):
        batch_seq_md_scoring(pred_md_lbl_seqs=np.zeros(3), gt_md_lbl_seqs=[[0]])
    with pytest.raises(TypeError):
        batch_boundary_scoring(np.zeros(3), [[0]])


def test_boundary_seq_to_seg_seq_keeps_the_last_segment_quirk():
    from utils.data_utils import boundary_seq_to_seg_seq
    seg = boundary_seq_to_seg_seq(torch.tensor([1, 0, 0, 1, 0, 1, 0, 0, 0, 0]))
    # the last end is the number of boundaries (3), not T (10)
    assert seg.tolist() == [[0, 3], [3, 5], [5, 3]]


# --------------------------------------------------------------------------- synthetic labels
def _sets():
    from utils.data_io import SyntheticSet
    kw = dict(n_utts=12, feat_dim=8, min_frames=40, max_frames=90, seed=77)
    return SyntheticSet(**kw), SyntheticSet(md_labels=False, **kw), \
        SyntheticSet(md_labels=True, n_phonemes=11, **kw)


def test_md_labels_leave_the_features_bit_identical():
    plain, off, on = _sets()
    assert [e["id"] for e in plain.items] == [e["id"] for e in off.items] == [e["id"] for e in on.items]
    for a, b, c in zip(plain.items, off.items, on.items):
        assert set(b) == {"id", "feat"}
        assert torch.equal(a["feat"], b["feat"]) and torch.equal(a["feat"], c["feat"])


def test_md_label_invariants():
    from brain.dataio import PaddedBatch
    _, _, on = _sets()
    n_ph = 11
    for e in on.items:
        T = e["feat"].shape[0]
        L = e["gt_cnncl_seq"].shape[0]
        assert e["gt_cnncl_seq"].dtype == torch.int64 and e["plvl_gt_md_lbl_seq"].dtype == torch.int64
        assert 2 <= L <= T and e["plvl_gt_md_lbl_seq"].shape == (L,)
        assert int(e["gt_cnncl_seq"].min()) >= 0 and int(e["gt_cnncl_seq"].max()) < n_ph
        assert set(e["plvl_gt_md_lbl_seq"].tolist()) <= {0, 1}
        for key in ("fa_boundary_seq", "gt_boundary_seq"):
            b = e[key]
            assert b.shape == (T,) and b.dtype == torch.float32
            assert set(b.tolist()) <= {0.0, 1.0} and b[0] == 1 and int(b.sum()) == L
        moved = (torch.where(e["fa_boundary_seq"] == 1)[0] - torch.where(e["gt_boundary_seq"] == 1)[0]).abs()
        assert int(moved.max()) <= 2
        assert e["prior"].shape == (n_ph + 2,)
        assert float(e["prior"].min()) > 0.05 and float(e["prior"].max()) < 0.5
    assert any(not torch.equal(e["fa_boundary_seq"], e["gt_boundary_seq"]) for e in on.items)
    assert any(int(e["plvl_gt_md_lbl_seq"].sum()) > 0 for e in on.items)
    # reproducible, and through PaddedBatch: padded shapes and the relative lengths' round trip
    _, _, again = _sets()
    assert all(torch.equal(a["gt_boundary_seq"], b["gt_boundary_seq"]) for a, b in zip(on.items, again.items))
    batch = PaddedBatch(on.items[:4])
    Tm = max(e["feat"].shape[0] for e in on.items[:4])
    Lm = max(e["gt_cnncl_seq"].shape[0] for e in on.items[:4])
    assert batch["feat"][0].shape[:2] == (4, Tm) and batch["fa_boundary_seq"][0].shape == (4, Tm)
    assert batch["gt_cnncl_seq"][0].shape == (4, Lm) and batch["prior"][0].shape == (4, n_ph + 2)
    assert torch.equal(batch["prior"][0][0], on.items[0]["prior"])
    for i, e in enumerate(on.items[:4]):
        assert int(torch.round(batch["feat"][1][i] * Tm)) == e["feat"].shape[0]
        assert int(torch.round(batch["gt_cnncl_seq"][1][i] * Lm)) == e["gt_cnncl_seq"].shape[0]
        assert torch.equal(batch["fa_boundary_seq"][1], batch["feat"][1])


def test_prepare_datasets_passes_md_labels():
    from utils.data_io import prepare_datasets
    hp = {"dataset": "synthetic", "seed": 5, "n_phonemes": 9, "model": {"input_size": 6},
          "prepare": {"dataset_dir": "/nonexistent/original_dataset"},
          "synthetic": {"n_train": 3, "n_valid": 2, "n_test": 2, "min_frames": 40, "max_frames": 50}}
    (tr, _, _), _ = prepare_datasets(hp)
    assert set(tr.items[0]) == {"id", "feat"}
    hp["synthetic"]["md_labels"] = True
    (tr2, _, te2), _ = prepare_datasets(hp)
    assert tr2.items[0]["prior"].shape == (11,) and "plvl_gt_md_lbl_seq" in te2.items[0]
    assert torch.equal(tr.items[0]["feat"], tr2.items[0]["feat"])


# --------------------------------------------------------------------------- schedule
def test_target_schedule_and_evaluation_gate(tmp_path):
    from brain import Stage
    from models.MD_VAE.model import SBModel, Target
    keys = ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "pi_nll_loss",
            "vae_kld_loss", "recon_loss", "plvl_md", "boundary"]
    m = SBModel(modules={}, hparams={"metric_keys": keys, "output_dir": str(tmp_path)},
                run_opts={"device": "cpu"})
    want = [Target.PHN_RECOG, Target.B_DETECTOR, Target.VAE] * 2
    for epoch in range(1, 7):
        for stage in (Stage.TRAIN, Stage.VALID):
            m.on_stage_start(stage, epoch)
            assert m.target == want[epoch - 1]
            evaluates = stage == Stage.VALID and want[epoch - 1] == Target.VAE
            assert m.to_run_evaluation(stage) == evaluates
            if evaluates:
                assert set(m.stats_loggers) == {k + "_stats" for k in keys}
            else:
                assert m.stats_loggers == {}
    m.on_stage_start(Stage.TEST, None)
    assert m.target == Target.TEST and m.to_run_evaluation(Stage.TEST)
    assert set(m.stats_loggers) == {k + "_stats" for k in keys}
    with pytest.raises(AssertionError):
        m.on_stage_start(Stage.TRAIN, None)


# --------------------------------------------------------------------------- yaml
def test_model_yaml_resolves_with_the_reference_keys():
    import functools
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import optim as hip_optim
    from modules.lstm import LSTM
    ov = ("dataset: synthetic\nmodel_class: MD_VAE\nmodel_name: md_vae\n"
          "model: !include:../models/MD_VAE/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    assert hp["synthetic"]["md_labels"] is False
    m = hp["model"]
    with open(os.path.join(GOLD, "md_vae_yaml_keys.json")) as f:
        ref = json.load(f)
    assert list(m["modules"].keys()) == ref["modules"]
    assert list(m["checkpointer"].recoverables.keys()) == ref["recoverables"]
    assert set(ref["top_level"]) <= set(m.keys())
    assert m["max_key"] == "plvl_md.F1"
    assert m["metric_keys"] == ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss",
                                "pi_nll_loss", "vae_kld_loss", "recon_loss", "plvl_md", "boundary"]
    assert (m["boundary_kld_weight"], m["vae_kld_weight"], m["pi_nll_weight"]) == (1e-5, 1e-5, 1e-3)
    assert isinstance(m["rnn"], LSTM) and m["rnn"].hidden_size == 512 and m["rnn"].dropout == 0.15
    assert m["modules"]["rnn"] is m["rnn"] and m["checkpointer"].recoverables["rnn"] is m["rnn"]
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    assert m["phoneme_recognizer"].fc.blocks[-1].out_features == hp["n_phonemes"] + 2
    assert m["pi_fc"].blocks[-1].out_features == 2
    assert m["epoch_counter"].limit == 50
