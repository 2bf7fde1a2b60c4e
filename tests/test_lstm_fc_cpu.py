"""The LSTM_FC recipe's host-side parts (no GPU):

* models/LSTM_FC/model.yaml through load_hyperpyyaml with the top-level config, its key names
  against the reference yaml's (tests/golden/lstm_fc_yaml_keys.json; log_softmax, a SpeechBrain
  class the recipe never calls, is the one key not carried);
* SyntheticSet's flvl_gt_md_lbl_seq: [T], binary, each phoneme's label over its gt_boundary_seq
  segment; every other field and the features unchanged by it;
* counts_md_scoring / MDMetricStats.append_counts against binary_seq_md_scoring, torch.equal;
* ops.flvl_md_head argument checks, which raise before any launch;
* tests/golden/lstm_fc_tiny.npz is self-consistent: the masked class-weighted BCE recomputed in
  numpy fp64 from the recorded logits, labels and lengths gives the recorded loss (1e-6 relative),
  and the recorded sequences are the argmax and the labels cut to length."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ["flvl_md.ACC", "flvl_md.PRE", "flvl_md.REC", "flvl_md.F1"]


# --------------------------------------------------------------------------- yaml
def test_model_yaml_resolves_with_the_reference_keys():
    import functools
    from brain.features import InputNormalization
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import optim as hip_optim
    from modules.fc_block import FCBlock
    from modules.lstm import LSTM
    ov = ("dataset: synthetic\nmodel_class: LSTM_FC\nmodel_name: lstm_fc\n"
          "model: !include:../models/LSTM_FC/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    m = hp["model"]
    with open(os.path.join(GOLD, "lstm_fc_yaml_keys.json")) as f:
        ref = json.load(f)
    assert ref["modules"] == ["normalizer", "lstm", "fc"]
    assert list(m["modules"].keys()) == ref["modules"]
    assert list(m["checkpointer"].recoverables.keys()) == ref["recoverables"]
    assert set(ref["top_level"]) - set(m.keys()) == {"log_softmax"}
    assert m["metric_keys"] == KEYS and m["max_key"] == "flvl_md.F1"
    assert m["misp_weight"] == 10 and m["lr"] == 1.0 and m["n_epochs"] == 50
    assert (m["fc_size"], m["fc_dropout"], m["output_size"]) == (64, 0, 2)
    lstm = m["lstm"]
    assert isinstance(lstm, LSTM) and m["modules"]["lstm"] is lstm
    assert (lstm.input_size, lstm.hidden_size, lstm.num_layers, lstm.dropout) == (120, 1024, 4, 0.1)
    assert lstm.batch_first and not lstm.bidirectional
    fc = m["fc"]
    assert isinstance(fc, FCBlock) and m["checkpointer"].recoverables["fc"] is fc
    lin = [b for b in fc.blocks if isinstance(b, torch.nn.Linear)]
    assert [(l.in_features, l.out_features) for l in lin] == [(1024, 64), (64, 64), (64, 2)]
    assert [act for _, act in fc.linear_plan()] == [True, True, False]
    assert isinstance(m["normalizer"], InputNormalization)
    assert m["checkpointer"].recoverables["normalizer"] is m["normalizer"]
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    assert m["optimizer"].keywords == {"lr": 1.0}
    assert m["epoch_counter"].limit == 50


def test_recipe_hooks_and_field_names(tmp_path):
    from brain import Stage
    from models.LSTM_FC.model import SBModel
    from models.md_model import MDModel
    from utils.metric_stats.md_metric_stats import MDMetricStats
    assert issubclass(SBModel, MDModel)
    m = SBModel(modules={}, hparams={"metric_keys": KEYS, "output_dir": str(tmp_path)},
                run_opts={"device": "cpu"})
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):  # the stats on every stage
        m.on_stage_start(stage, 1)
        assert set(m.stats_loggers) == {"flvl_md_stats"}
        assert isinstance(m.stats_loggers["flvl_md_stats"], MDMetricStats)
    plain = {"feat": 0, "flvl_gt_md_lbl_seq": 0}
    aug = dict(plain, aug_feat=0, aug_flvl_gt_md_lbl_seq=0)
    assert m._fields(aug, Stage.TRAIN) == ("aug_feat", "aug_flvl_gt_md_lbl_seq")
    assert m._fields(plain, Stage.TRAIN) == ("feat", "flvl_gt_md_lbl_seq")
    for stage in (Stage.VALID, Stage.TEST):
        assert m._fields(aug, stage) == ("feat", "flvl_gt_md_lbl_seq")


# --------------------------------------------------------------------------- labels
def test_synthetic_frame_level_labels():
    from utils.data_io import SyntheticSet
    kw = dict(n_utts=12, feat_dim=6, min_frames=11, max_frames=90, seed=7, sorting=None)
    with_md = SyntheticSet(md_labels=True, n_phonemes=9, **kw)
    without = SyntheticSet(md_labels=False, **kw)
    seen = set()
    for e, p in zip(with_md.items, without.items):
        assert set(p) == {"id", "feat"} and p["id"] == e["id"]
        assert torch.equal(p["feat"], e["feat"])  # the labels take no draw from the feature stream
        assert set(e) == {"id", "feat", "gt_cnncl_seq", "fa_boundary_seq", "gt_boundary_seq",
                          "plvl_gt_md_lbl_seq", "flvl_gt_md_lbl_seq", "prior"}
        T = e["feat"].shape[0]
        flvl, plvl, gt = e["flvl_gt_md_lbl_seq"], e["plvl_gt_md_lbl_seq"], e["gt_boundary_seq"]
        assert flvl.shape == (T,) and flvl.dtype == torch.int64
        assert bool(((flvl == 0) | (flvl == 1)).all())
        starts = torch.where(gt == 1)[0].tolist()
        assert starts[0] == 0 and len(starts) == len(plvl)
        for k, (s, t) in enumerate(zip(starts, starts[1:] + [T])):
            assert t > s and bool((flvl[s:t] == plvl[k]).all()), (e["id"], k)
        seen |= set(flvl.tolist())
    assert seen == {0, 1}


def test_existing_md_fields_are_bit_identical():
    """The fields drawn before flvl_gt_md_lbl_seq existed: the same generator calls in the same
    order (restated here), so every one of them is unchanged."""
    from utils.data_io import JITTER, MIN_SEG, _label_generator, _synthetic_md_labels
    for i, T in enumerate((10, 24, 57, 200)):
        got = _synthetic_md_labels(T, 39, _label_generator(3, i))
        g = _label_generator(3, i)
        lo, hi = max(2, T // 12), max(2, T // 8)
        L = min(int(torch.randint(lo, hi + 1, (1,), generator=g)), max(T // MIN_SEG, 1))
        extra = torch.randint(0, L, (max(T - MIN_SEG * L, 0),), generator=g)
        dur = torch.bincount(extra, minlength=L) + min(MIN_SEG, T // L)
        starts = torch.cumsum(dur, 0) - dur
        fa = torch.zeros(T)
        fa[starts] = 1.0
        move = torch.randint(-JITTER, JITTER + 1, (L,), generator=g)
        move[0] = 0
        if min(MIN_SEG, T // L) < MIN_SEG:
            move.zero_()
        gt = torch.zeros(T)
        gt[starts + move] = 1.0
        assert torch.equal(got["gt_cnncl_seq"], torch.randint(0, 39, (L,), generator=g, dtype=torch.int64))
        assert torch.equal(got["plvl_gt_md_lbl_seq"], (torch.rand(L, generator=g) < 0.2).to(torch.int64))
        assert torch.equal(got["fa_boundary_seq"], fa) and torch.equal(got["gt_boundary_seq"], gt)


# --------------------------------------------------------------------------- metrics
def _host_counts(pred, gt):
    p, g = torch.as_tensor(pred), torch.as_tensor(gt)
    return [int(((1 - p) * (1 - g)).sum()), int((p * g).sum()), int(((1 - p) * g).sum()),
            int((p * (1 - g)).sum())]


def test_counts_scoring_equals_sequence_scoring():
    from utils.metric_stats.md_metric_stats import (MDMetricStats, binary_seq_md_scoring,
                                                    counts_md_scoring)
    g = torch.Generator().manual_seed(5)
    pairs = []
    for n in (2, 3, 17, 240, 1999):
        for p1 in (0.1, 0.5, 0.9):
            pairs.append(((torch.rand(n, generator=g) < p1).long().tolist(),
                          (torch.rand(n, generator=g) < 0.3).long().tolist()))
    pairs += [([0] * 9, [0] * 9),            # all correct
              ([1] * 9, [1] * 9),            # all mispronounced
              ([0] * 9, [0, 1, 1, 0, 0, 0, 1, 0, 0]),   # empty prediction set
              ([1, 0, 1, 1], [0] * 4)]       # no mispronunciation to find
    counts = torch.tensor([_host_counts(p, t) for p, t in pairs], dtype=torch.int32)
    got = counts_md_scoring(counts)
    assert len(got) == len(pairs)
    for (p, t), s in zip(pairs, got):
        want = binary_seq_md_scoring(p, t)
        assert list(s) == list(want) == ["ACC", "PRE", "REC", "F1"]
        for k in want:
            assert s[k].dtype == want[k].dtype and torch.equal(s[k], want[k]), (k, s[k], want[k])
    # int64 counts score the same; a wrong shape is refused
    assert all(torch.equal(a[k], b[k]) for a, b in zip(got, counts_md_scoring(counts.long())) for k in a)
    with pytest.raises(ValueError, match=r"\[B, 4\]"):
        counts_md_scoring(torch.zeros(3, 5, dtype=torch.int32))
    # the accumulator: two batches of counts against the sequences
    ids = [f"u{i}" for i in range(len(pairs))]
    a, b = MDMetricStats(), MDMetricStats()
    h = len(pairs) // 2
    a.append_counts(ids[:h], counts[:h])
    a.append_counts(ids[h:], counts[h:])
    b.append(ids, pred_md_lbl_seqs=[p for p, _ in pairs], gt_md_lbl_seqs=[t for _, t in pairs])
    assert a.summarize() == b.summarize() and a.ids == b.ids
    assert a.summarize("F1") == b.summarize("F1")
    with pytest.raises(ValueError, match="counts must be"):
        a.append_counts(ids[:2], counts[:3])


# --------------------------------------------------------------------------- ops argument checks
def _head_args(B=2, T=3, E=5):
    z = torch.zeros
    return dict(h=z(B, T, E), weight=z(2, E), bias=z(2), labels=z(B, T), lens=torch.ones(B))


def _head(a, pos_weight=(1.0, 10.0)):
    from mlvae_hip import ops
    return ops.flvl_md_head(a["h"], a["weight"], a["bias"], a["labels"], a["lens"], pos_weight)


def test_flvl_md_head_argument_checks_raise_before_any_launch():
    bad = [("h", torch.zeros(6, 5)),            # no [B, T, E]
           ("h", torch.zeros(2, 3, 0)),         # no features
           ("weight", torch.zeros(3, 5)),       # not two classes
           ("weight", torch.zeros(2, 4)),       # another E
           ("bias", torch.zeros(3)),
           ("labels", torch.zeros(2, 4)),
           ("labels", torch.zeros(2, 3, 1)),
           ("lens", torch.ones(3))]
    for name, t in bad:
        a = _head_args()
        a[name] = t
        with pytest.raises(ValueError, match="flvl_md_head"):
            _head(a)
    with pytest.raises(ValueError):
        _head(_head_args(), pos_weight=(1.0,))
    # well-formed shapes off the device: the HIP path has no CPU fallback
    with pytest.raises(TypeError, match="HIP tensor"):
        _head(_head_args())
    a = _head_args()
    a["h"] = a["h"].double()
    with pytest.raises(TypeError, match="HIP tensor"):
        _head(a)


# --------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(GOLD, "lstm_fc_tiny.npz"))
    return {k: d[k] for k in d.files}


@pytest.mark.parametrize("name", ["TRAIN", "TEST"])
def test_fixture_is_self_consistent(gold, name):
    meta = json.loads(str(gold["meta_json"]))
    B, T = meta["B"], meta["T"]
    assert (B, T, meta["F"], meta["H"], meta["L"]) == (3, 24, 8, 16, 2)
    assert meta["fc_sizes"] == [16, 8, 8, 2] and meta["misp_weight"] == 10
    lens = meta["lengths"]
    assert len(set(lens)) == B
    assert np.array_equal(np.round(gold["feat_lens"].astype(np.float64) * T).astype(int), lens)
    x = gold[name + "/out"].astype(np.float64)
    l = gold["flvl_gt_md_lbl_seq"].astype(np.float64)
    assert x.shape == (B, T, 2) and l.shape == (B, T)
    y = np.stack([1 - l, l], -1)
    pw = np.array([1.0, meta["misp_weight"]])
    sp = lambda v: np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v)))
    loss_e = pw * y * sp(-x) + (1 - y) * sp(x)
    mask = (np.arange(T)[None, :] < np.array(lens)[:, None]).astype(np.float64)[..., None]
    want = (loss_e * mask).sum() / (mask.sum() * 2)
    got = float(gold[name + "/loss"])
    print(f"{name}: loss recomputed {want:.9f} recorded {got:.9f}")
    assert abs(want - got) <= 1e-6 * abs(want)
    # with the mask over one class only, or without the class weight, the number differs
    assert abs((loss_e * mask).sum() / mask.sum() - got) > 1e-3 * abs(got)
    assert abs(((y * sp(-x) + (1 - y) * sp(x)) * mask).sum() / (mask.sum() * 2) - got) > 1e-3 * abs(got)
    # the recorded sequences: the argmax and the labels, cut to length; the seed's conditions
    pred, gt = gold[name + "/pred_md_lbl_seqs"], gold[name + "/gt_md_lbl_seqs"]
    valid = mask[..., 0] > 0
    assert np.array_equal(pred, np.where(valid, x.argmax(-1), -1))
    assert np.array_equal(gt, np.where(valid, l.astype(np.int64), -1))
    assert set(pred[valid].tolist()) == {0, 1} and set(gt[valid].tolist()) == {0, 1}
    assert np.abs(x[..., 1] - x[..., 0])[valid].min() >= 1e-3
    if name == "TRAIN":
        for n in meta["param_names"]:
            g = gold["TRAIN/grad/" + n]
            assert g.shape == gold["param/" + n].shape and np.isfinite(g).all() and np.abs(g).max() > 0
