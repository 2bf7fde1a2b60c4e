"""The upstream-module recipes' host-side parts (no GPU):

* models/test_phn_classifier and models/test_b_ind_classifier: model.yaml through load_hyperpyyaml
  with the top-level config, key names against the reference yamls' (tests/golden/*_yaml_keys.json);
  the stats logger on every stage;
* the host scoring functions and counts_phn_acc_scoring / counts_boundary_scoring against the
  reference's own scores of every case of tests/golden/score_cases.npz (make_golden_score.py), ``==``;
* append_counts / summarize against the list append on the same cases; ``__pad__`` rows dropped;
  two ranks' states merged into the single-process order;
* SyntheticSet(phn_labels=True): one more field, flvl_gt_cnncl_seq, every other field and the
  features bit-identical;
* ops.phn_acc_counts / boundary_topk / boundary_counts argument checks, which raise before any
  launch."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases():
    d = np.load(os.path.join(GOLD, "score_cases.npz"))
    return {k: d[k] for k in d.files}


# --------------------------------------------------------------------------- yaml, hooks
def _resolve(recipe):
    from hyperpyyaml import load_hyperpyyaml
    ov = (f"dataset: synthetic\nmodel_class: {recipe}\nmodel_name: ci\n"
          f"model: !include:../models/{recipe}/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    with open(os.path.join(GOLD, f"{recipe}_yaml_keys.json")) as f:
        return hp, hp["model"], json.load(f)


def _common_yaml(m, ref, module_key):
    import functools
    from brain.features import InputNormalization
    from mlvae_hip import optim as hip_optim
    assert ref["modules"] == [module_key] and ref["recoverables"] == [module_key, "epoch_counter"]
    assert list(m["modules"].keys()) == ref["modules"]
    assert list(m["checkpointer"].recoverables.keys()) == ref["recoverables"]
    assert set(ref["top_level"]) <= set(m.keys())  # every reference key is carried
    assert m["modules"][module_key] is m[module_key] is m["checkpointer"].recoverables[module_key]
    assert (m["n_epochs"], m["lr"], m["rnn_hidden_size"], m["rnn_num_layers"], m["fc_size"]) == \
        (50, 0.001, 512, 2, 128)
    assert isinstance(m["normalizer"], InputNormalization)
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    assert m["optimizer"].keywords == {"lr": 0.001}
    assert m["epoch_counter"].limit == 50
    rnn = m[module_key].rnn
    assert (rnn.input_size, rnn.hidden_size, rnn.num_layers) == (120, 512, 2) and rnn.batch_first


def _fc_sizes(fc):
    return [(b.in_features, b.out_features) for b in fc.blocks if isinstance(b, torch.nn.Linear)]


def test_phn_yaml_resolves_with_the_reference_keys():
    from modules.phoneme_recognizer import PhonemeRecognizer
    hp, m, ref = _resolve("test_phn_classifier")
    _common_yaml(m, ref, "phoneme_recognizer")
    assert m["metric_keys"] == ["phn_acc.flvl_acc", "phn_acc.plvl_acc"] and m["max_key"] == "phn_acc.flvl_acc"
    rec = m["phoneme_recognizer"]
    assert isinstance(rec, PhonemeRecognizer) and rec.n_phonemes == hp["n_phonemes"]
    assert _fc_sizes(rec.fc) == [(512, 128), (128, 128), (128, hp["n_phonemes"] + 2)]
    assert hp["synthetic"]["phn_labels"] is False and hp["synthetic"]["md_labels"] is False


def test_b_ind_yaml_resolves_with_the_reference_keys():
    from modules.boundary_detector import BoundaryDetector
    _, m, ref = _resolve("test_b_ind_classifier")
    _common_yaml(m, ref, "boundary_detector")
    assert m["metric_keys"] == ["boundary.f1", "boundary.r_value"] and m["max_key"] == "boundary.f1"
    det = m["boundary_detector"]
    assert isinstance(det, BoundaryDetector)
    for head in (det.fc_alpha, det.fc_beta):
        assert _fc_sizes(head[0]) == [(512, 128), (128, 128), (128, 1)]


@pytest.mark.parametrize("recipe,key,cls", [
    ("test_phn_classifier", "phn_acc_stats", "PhnAccMetricStats"),
    ("test_b_ind_classifier", "boundary_stats", "BoundaryMetricStats")])
def test_recipe_builds_its_stats_on_every_stage(recipe, key, cls, tmp_path):
    import importlib
    from brain import Stage
    from models.md_model import MDModel
    SBModel = importlib.import_module(f"models.{recipe}.model").SBModel
    assert issubclass(SBModel, MDModel) and SBModel.dp_exact is True
    m = SBModel(modules={}, hparams={"metric_keys": ["x.y"], "output_dir": str(tmp_path)},
                run_opts={"device": "cpu"})
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        m.on_stage_start(stage, 1)
        assert set(m.stats_loggers) == {key}
        assert type(m.stats_loggers[key]).__name__ == cls
        assert hasattr(m.stats_loggers[key], "append_counts")


# --------------------------------------------------------------------------- scores of the cases
def _phn_lists(c, i):
    Ti, Li = int(c["T"][i]), int(c["L"][i])
    t = lambda k, n: torch.from_numpy(c[k][i, :n])
    return t("logits", Ti), t("flvl_tgt", Ti), t("plvl_tgt", Li), t("phn_boundary", Ti)


def _bnd_lists(c, i):
    Ti = int(c["T"][i])
    return torch.from_numpy(c["chosen"][i, :Ti]).float(), torch.from_numpy(c["gt_boundary"][i, :Ti])


def test_cases_cover_the_edges(cases):
    c = cases
    N = len(c["T"])
    assert N >= 40 and c["logits"].shape[1:] == (64, 7)
    assert (c["k"] == 0).any() and (c["k"] == c["T"]).any() and (c["k"] == 1).any() and (c["T"] == 1).any()
    assert (c["n_target"] == 0).any() and (c["n_pred"] == 0).any()
    assert any(c["gt_boundary"][i, 0] == 0 and c["n_target"][i] > 0 for i in range(N))
    for key in ("flvl_acc", "plvl_acc", "pre", "rec"):
        assert ((c[key] > 0) & (c[key] < 100)).any(), key
    # the chosen frames are k ones among the valid frames, -1 past them
    for i in range(N):
        Ti = int(c["T"][i])
        assert (c["chosen"][i, Ti:] == -1).all() and int((c["chosen"][i, :Ti] == 1).sum()) == c["k"][i]
        assert c["fa_boundary"][i].sum() == c["k"][i]


def test_host_functions_reproduce_the_reference_scores(cases):
    from utils.metric_stats.boundary_metric_stats import boundary_scoring
    from utils.metric_stats.phn_acc_metric_stats import flvl_phn_acc_scoring, plvl_phn_acc_scoring
    c = cases
    for i in range(len(c["T"])):
        out, ft, pt, pb = _phn_lists(c, i)
        assert flvl_phn_acc_scoring(out, ft) == c["flvl_acc"][i]
        assert plvl_phn_acc_scoring(out, pt, pb) == c["plvl_acc"][i]
        pred, gt = _bnd_lists(c, i)
        s = boundary_scoring(pred, gt)
        for k in ("pre", "rec", "f1", "r_value"):
            assert s[k] == c[k][i], (i, k)


def test_counts_scoring_reproduces_the_reference_scores(cases):
    from utils.metric_stats.boundary_metric_stats import counts_boundary_scoring
    from utils.metric_stats.phn_acc_metric_stats import counts_phn_acc_scoring
    c = cases
    pc = np.stack([c["flvl_correct"], c["T"], c["plvl_correct"], c["L"]], 1)
    bc = np.stack([c["correct"], c["n_pred"], c["n_target"]], 1)
    ps, bs = counts_phn_acc_scoring(torch.from_numpy(pc)), counts_boundary_scoring(torch.from_numpy(bc))
    for i in range(len(c["T"])):
        assert ps[i]["flvl_acc"] == c["flvl_acc"][i] and ps[i]["plvl_acc"] == c["plvl_acc"][i], i
        for k in ("pre", "rec", "f1", "r_value"):
            assert bs[i][k] == c[k][i], (i, k)
    # no phoneme targets: plvl_acc is the reference's 0
    assert counts_phn_acc_scoring(torch.tensor([[3, 4, 0, 0]]))[0] == {"flvl_acc": 75.0, "plvl_acc": 0}
    for fn, n in ((counts_phn_acc_scoring, 4), (counts_boundary_scoring, 3)):
        with pytest.raises(ValueError, match="counts must be"):
            fn(torch.zeros(2, n + 1, dtype=torch.int32))


def _both(c, which, rows, pad_at=None):
    """(list-fed stats, counts-fed stats) over the given cases, in batches of 4; pad_at: a filler
    row put into every batch of the counts-fed one at that position."""
    from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
    from utils.metric_stats.phn_acc_metric_stats import PhnAccMetricStats
    cls = PhnAccMetricStats if which == "phn" else BoundaryMetricStats
    a, b = cls(), cls()
    for lo in range(0, len(rows), 4):
        idx = rows[lo:lo + 4]
        ids = [f"utt{i}" for i in idx]
        if which == "phn":
            ls = [_phn_lists(c, i) for i in idx]
            a.append(ids, predictions=[l[0] for l in ls], flvl_targets=[l[1] for l in ls],
                     plvl_targets=[l[2] for l in ls], boundary_seqs=[l[3] for l in ls])
            counts = np.stack([c["flvl_correct"][idx], c["T"][idx], c["plvl_correct"][idx], c["L"][idx]], 1)
        else:
            ls = [_bnd_lists(c, i) for i in idx]
            a.append(ids, predictions=[l[0] for l in ls], targets=[l[1] for l in ls])
            counts = np.stack([c["correct"][idx], c["n_pred"][idx], c["n_target"][idx]], 1)
        counts = torch.from_numpy(counts.astype(np.int32))
        if pad_at is not None:
            p = min(pad_at, len(ids))
            ids = ids[:p] + ["__pad__"] + ids[p:]
            counts = torch.cat([counts[:p], torch.zeros(1, counts.shape[1], dtype=torch.int32), counts[p:]])
        b.append_counts(ids, counts)
    return a, b


@pytest.mark.parametrize("which", ["phn", "bnd"])
@pytest.mark.parametrize("pad_at", [None, 1])
def test_append_counts_equals_append(cases, which, pad_at):
    rows = list(range(len(cases["T"])))
    a, b = _both(cases, which, rows, pad_at)
    assert b.scores_list == []  # nothing read before the summary
    assert b.summarize() == a.summarize()
    assert b.ids == a.ids and b.order == a.order and "__pad__" not in b.ids
    assert len(b.scores_list) == len(rows)
    for x, y in zip(a.scores_list, b.scores_list):
        assert x == y
    key = "flvl_acc" if which == "phn" else "f1"
    assert b.summarize(key) == a.summarize()[key]
    with pytest.raises(ValueError, match="counts must be"):
        b.append_counts(["u"], torch.zeros(2, b.n_counts, dtype=torch.int32))


@pytest.mark.parametrize("which", ["phn", "bnd"])
def test_merge_gives_the_single_process_order(cases, which):
    """Global batches of 4 split over two ranks (2 + 2 rows each): the merged entries are the
    single process's, in its order, and so is the fp32 mean."""
    from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
    from utils.metric_stats.phn_acc_metric_stats import PhnAccMetricStats
    rows = list(range(22))  # the last global batch is short: rank 1 holds fillers alone
    single, _ = _both(cases, which, rows)
    cls = PhnAccMetricStats if which == "phn" else BoundaryMetricStats
    ranks = [cls(), cls()]
    c = cases
    for g, lo in enumerate(range(0, len(rows), 4)):
        glob = rows[lo:lo + 4]
        for r in range(2):
            idx = glob[2 * r:2 * r + 2]
            ids = [f"utt{i}" for i in idx] + ["__pad__"] * (2 - len(idx))
            if which == "phn":
                cols = [c["flvl_correct"], c["T"], c["plvl_correct"], c["L"]]
            else:
                cols = [c["correct"], c["n_pred"], c["n_target"]]
            counts = np.zeros((2, len(cols)), np.int32)
            for j, i in enumerate(idx):
                counts[j] = [col[i] for col in cols]
            ranks[r].append_counts(ids, torch.from_numpy(counts), batch_index=g)
    merged = cls()
    merged.merge([st.state() for st in ranks])
    assert merged.ids == single.ids
    assert merged.summarize() == single.summarize()
    for x, y in zip(single.scores_list, merged.scores_list):
        # merge() keeps the scores as fp32 tensors, what summarize()'s mean reads them as
        assert {k: torch.tensor(float(v)) for k, v in x.items()} == dict(y)


def test_batch_phn_acc_scoring_errors():
    from utils.metric_stats.phn_acc_metric_stats import (batch_phn_acc_scoring, flvl_phn_acc_scoring,
                                                         plvl_phn_acc_scoring)
    x, t = torch.randn(4, 3), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError, match="must be list"):
        batch_phn_acc_scoring(x, [t])
    with pytest.raises(ValueError, match="Inconsistent batch size"):
        batch_phn_acc_scoring([x], [t, t])
    with pytest.raises(ValueError, match="boundary_seqs must be provided"):
        batch_phn_acc_scoring([x], [t], plvl_targets=[t[:2]])
    with pytest.raises(ValueError, match="two dimensions"):
        flvl_phn_acc_scoring(x[0], t)
    with pytest.raises(ValueError, match="Inconsistent input lengths"):
        flvl_phn_acc_scoring(x, t[:3])
    with pytest.raises(AssertionError):  # three flags, two phonemes
        plvl_phn_acc_scoring(x, t[:2], torch.tensor([1.0, 1.0, 1.0, 0.0]))
    with pytest.raises(AssertionError):  # no flag at frame 0: the durations do not cover T
        plvl_phn_acc_scoring(x, t[:2], torch.tensor([0.0, 1.0, 1.0, 0.0]))
    assert batch_phn_acc_scoring([x], [t])[0]["plvl_acc"] == 0


# --------------------------------------------------------------------------- synthetic labels
def test_phn_labels_add_one_field():
    from utils.data_io import SyntheticSet
    kw = dict(n_utts=6, feat_dim=5, min_frames=30, max_frames=70, seed=11, sorting="descending")
    md = SyntheticSet(md_labels=True, n_phonemes=9, **kw)
    both = SyntheticSet(md_labels=True, phn_labels=True, n_phonemes=9, **kw)
    alone = SyntheticSet(phn_labels=True, **kw)  # without md_labels there is nothing to derive from
    for a, b, e in zip(md.items, both.items, alone.items):
        assert set(b) - set(a) == {"flvl_gt_cnncl_seq"} and set(a) <= set(b)
        assert set(e) == {"id", "feat"}
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
            else:
                assert a[k] == b[k]
        assert torch.equal(e["feat"], b["feat"])
        f = b["flvl_gt_cnncl_seq"]
        T = b["feat"].shape[0]
        assert f.dtype == torch.int64 and f.shape == (T,)
        starts = torch.where(b["gt_boundary_seq"] == 1)[0].tolist() + [T]
        assert starts[0] == 0 and len(starts) - 1 == len(b["gt_cnncl_seq"])
        for l, (s, t) in enumerate(zip(starts[:-1], starts[1:])):
            assert bool((f[s:t] == b["gt_cnncl_seq"][l]).all())


def test_prepare_datasets_passes_phn_labels():
    from utils.data_io import prepare_datasets
    hp = {"dataset": "synthetic", "seed": 5, "n_phonemes": 9, "model": {"input_size": 6},
          "prepare": {"dataset_dir": "/nonexistent/corpus"},
          "synthetic": {"n_train": 3, "n_valid": 2, "n_test": 2, "min_frames": 40, "max_frames": 50,
                        "md_labels": True}}
    sets, _ = prepare_datasets(hp)
    assert all("flvl_gt_cnncl_seq" not in e for s in sets for e in s.items)
    hp["synthetic"]["phn_labels"] = True
    sets, _ = prepare_datasets(hp)
    assert all("flvl_gt_cnncl_seq" in e for s in sets for e in s.items)


# --------------------------------------------------------------------------- op argument checks
def test_score_ops_check_their_arguments_before_any_launch():
    from mlvae_hip import ops
    out, lens = torch.zeros(2, 5, 3), torch.ones(2)
    ft, pt, bnd = torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 5)
    with pytest.raises(ValueError, match=r"\[B, T, C\]"):
        ops.phn_acc_counts(out[0], lens, ft)
    with pytest.raises(TypeError, match="float32 HIP tensor"):
        ops.phn_acc_counts(out, lens, ft, pt, lens, bnd)
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        ops.boundary_topk(out, lens, bnd)
    with pytest.raises(TypeError, match="float32 HIP tensor"):
        ops.boundary_topk(bnd, lens, bnd)
    with pytest.raises(TypeError, match="int32"):
        ops.boundary_counts(bnd, bnd, lens)
    assert ops.SCORE_ERR_SEGMENTS == 128 and ops.SCORE_ERR_K == 256
