"""The HMM_DNN_ALI aligner's host-side parts (no GPU):

* the float64 oracle tests/hmm_np.py -- forward score, Viterbi score and path, occupancy gradient
  -- against brute-force enumeration of every path at T = 7, L = 3, spp = 2 with a repeated
  phoneme (6 states in 7 frames: C(6, 5) = 6 paths) and at T = 9 (C(8, 5) = 56 paths);
* its CTC against torch.nn.functional.ctc_loss in float64 (reduction 'none' per utterance, 'mean'
  as the recipe's), with blank = C - 1, an infeasible utterance and a repeated target;
* models/HMM_DNN_ALI/model.yaml through load_hyperpyyaml, its key names against the reference
  yaml's (tests/golden/hmm_dnn_ali_yaml_keys.json), the four omissions listed;
* SyntheticSet's ali_labels: gt_phn_end_seq strictly increasing, ending at T * samples_per_frame,
  every other field bit-identical with and without it;
* AlignAccMetricStats and the ops' argument checks, which raise before any launch."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import hmm_np
from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# --------------------------------------------------------------------------- oracle vs brute force
def _hmm_paths(T, N):
    """Every monotone path s_0 = 0, steps in {0, 1}, s_{T-1} = N - 1."""
    out = []
    for steps in itertools.product((0, 1), repeat=T - 1):
        if sum(steps) == N - 1:
            out.append(np.concatenate([[0], np.cumsum(steps)]))
    return out


def _lp(T, C, seed, scale=1.0):
    g = np.random.default_rng(seed)
    x = g.standard_normal((T, C)) * scale
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def test_oracle_hmm_equals_path_enumeration():
    T, spp, C = 7, 2, 8
    phns = [1, 1, 3]                      # a repeated phoneme: classes 2 3 2 3 6 7
    cls = hmm_np.expand(phns, spp)
    assert cls.tolist() == [2, 3, 2, 3, 6, 7]
    lp = _lp(T, C, 11)
    paths = _hmm_paths(T, len(cls))
    assert len(paths) == 6                # C(6, 5): where the one extra frame is spent
    scores = np.array([lp[np.arange(T), cls[p]].sum() for p in paths])
    want = np.logaddexp.reduce(scores)
    nodes, skip = hmm_np.nodes(cls, hmm_np.HMM)
    got, gamma = hmm_np.forward_backward(lp, nodes, skip, hmm_np.HMM)
    assert abs(got - want) < 1e-12
    # occupancies: the posterior path weights summed where the path sits
    w = np.exp(scores - want)
    occ = np.zeros((T, len(cls)))
    for p, wp in zip(paths, w):
        occ[np.arange(T), p] += wp
    assert np.abs(gamma - occ).max() < 1e-12
    assert np.allclose(gamma.sum(1), 1.0, atol=1e-12)
    # Viterbi: the best enumerated path
    vs, path = hmm_np.viterbi(lp, cls)
    best = int(np.argmax(scores))
    assert abs(vs - scores[best]) < 1e-12 and path.tolist() == paths[best].tolist()


def test_oracle_hmm_more_paths_and_the_tie_rule():
    T, spp, C = 9, 2, 8
    cls = hmm_np.expand([1, 1, 3], spp)
    lp = _lp(T, C, 5)
    paths = _hmm_paths(T, len(cls))
    assert len(paths) == 56               # C(8, 5)
    scores = np.array([lp[np.arange(T), cls[p]].sum() for p in paths])
    nodes, skip = hmm_np.nodes(cls, hmm_np.HMM)
    got, gamma = hmm_np.forward_backward(lp, nodes, skip, hmm_np.HMM)
    assert abs(got - np.logaddexp.reduce(scores)) < 1e-12
    vs, path = hmm_np.viterbi(lp, cls)
    assert abs(vs - scores.max()) < 1e-12 and path.tolist() == paths[int(np.argmax(scores))].tolist()
    # all-equal log-probs: every path ties.  The backpointer of a node reachable by both keeps
    # "stay", so walking back from the end the path stays in the last state for as long as that
    # state was reachable: it climbs first and rests at the end
    flat = np.full((T, C), -np.log(C))
    _, path = hmm_np.viterbi(flat, cls)
    assert path.tolist() == [0, 1, 2, 3, 4, 5, 5, 5, 5]


def test_oracle_batch_lengths_and_infeasible():
    B, T, C, L, spp = 3, 8, 10, 3, 2
    g = np.random.default_rng(2)
    pout = np.stack([_lp(T, C, 20 + b) for b in range(B)])
    phns = g.integers(0, C // spp, (B, L))
    lens = np.array([1.0, 0.5, 0.3125], dtype=np.float32)      # T_b = 8, 4, 2 (2.5 rounds to even)
    phn_lens = np.array([1.0, 2 / 3, 2 / 3], dtype=np.float32)  # U_b = 6, 4, 4
    assert [hmm_np.round_len(v, T) for v in lens] == [8, 4, 2]
    score, dp, ok = hmm_np.lattice_batch(pout, lens, phns, phn_lens, spp, hmm_np.HMM)
    assert ok.tolist() == [True, True, False] and score[2] == 0 and not dp[2].any()
    # T_b == U_b: one path, the diagonal
    diag = sum(pout[1, t, hmm_np.expand(phns[1, :2], spp)[t]] for t in range(4))
    assert abs(score[1] - diag) < 1e-12
    assert not dp[1, 4:].any() and np.allclose(dp[0].sum(-1), 1.0)
    vs, al = hmm_np.viterbi_batch(pout, lens, phns, phn_lens, spp)
    assert abs(vs[1] - diag) < 1e-12 and al[1].tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    assert (al[2] == -1).all() and vs[2] == 0


# --------------------------------------------------------------------------- CTC vs torch
def _torch_ctc(pout, Tb, targets, Ub, blank, reduction):
    lp = torch.from_numpy(pout).transpose(0, 1)  # [T, B, C]
    return torch.nn.functional.ctc_loss(lp, torch.as_tensor(targets), torch.as_tensor(Tb),
                                        torch.as_tensor(Ub), blank=blank, reduction=reduction,
                                        zero_infinity=True)


def test_oracle_ctc_equals_torch_float64():
    B, T, C, L, spp = 4, 12, 9, 4, 1
    blank = C - 1
    pout = np.stack([_lp(T, C, 40 + b) for b in range(B)])
    phns = np.array([[1, 1, 2, 1],      # a repeated target: the blank between is forced
                     [3, 0, 5, 2],
                     [4, 4, 4, 4],      # 4 equal targets need 7 frames; it has 6: infeasible
                     [6, 2, 0, 0]])
    lens = np.array([1.0, 0.75, 0.5, 1.0], dtype=np.float32)
    phn_lens = np.array([1.0, 1.0, 1.0, 0.5], dtype=np.float32)
    Tb = [hmm_np.round_len(v, T) for v in lens]
    Ub = [hmm_np.round_len(v, L) * spp for v in phn_lens]
    assert Tb == [12, 9, 6, 12] and Ub == [4, 4, 4, 2]
    score, dp, ok = hmm_np.lattice_batch(pout, lens, phns, phn_lens, spp, hmm_np.CTC, blank)
    assert ok.tolist() == [True, True, False, True]
    want = _torch_ctc(pout, Tb, phns, Ub, blank, "none").numpy()
    assert want[2] == 0  # zero_infinity
    assert np.abs(-score - want).max() < 1e-10
    mean = _torch_ctc(pout, Tb, phns, Ub, blank, "mean").item()
    assert abs(np.mean(-score / np.maximum(Ub, 1)) - mean) < 1e-12
    # the gradient at the logits: torch folds the log-softmax backward in
    x = torch.from_numpy(pout).clone().requires_grad_(True)
    lp = torch.log_softmax(x, -1)
    torch.nn.functional.ctc_loss(lp.transpose(0, 1), torch.as_tensor(phns), torch.as_tensor(Tb),
                                 torch.as_tensor(Ub), blank=blank, reduction="sum",
                                 zero_infinity=True).backward()
    p = torch.softmax(torch.from_numpy(pout), -1).numpy()
    dx = -(dp - p * dp.sum(-1, keepdims=True))  # d(-score)/dx through the log-softmax
    assert np.abs(dx - x.grad.numpy()).max() < 1e-10
    # spp = 2 expands the targets
    phns2 = np.array([[0, 1], [2, 2], [3, 0], [1, 3]])
    ones = np.ones(B, dtype=np.float32)
    s2, _, ok2 = hmm_np.lattice_batch(pout, ones, phns2, ones, 2, hmm_np.CTC, blank)
    tg = np.stack([hmm_np.expand(r, 2) for r in phns2])
    w2 = _torch_ctc(pout, [T] * B, tg, [4] * B, blank, "none").numpy()
    assert ok2.all() and np.abs(-s2 - w2).max() < 1e-10


# --------------------------------------------------------------------------- yaml
OMITTED = {"log_softmax", "compute_cost_ctc", "compute_cost_nll", "lr_annealing"}


def test_model_yaml_resolves_with_the_reference_keys():
    import functools
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import optim as hip_optim
    from modules.hmm_aligner import HMMAligner
    from modules.linear import Linear
    from modules.vanilla_nn import VanillaNN
    ov = ("dataset: synthetic\nmodel_class: HMM_DNN_ALI\nmodel_name: ali\n"
          "model: !include:../models/HMM_DNN_ALI/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    m = hp["model"]
    with open(os.path.join(GOLD, "hmm_dnn_ali_yaml_keys.json")) as f:
        ref = json.load(f)
    assert set(ref["top_level"]) - set(m.keys()) == OMITTED
    assert list(m["modules"].keys()) == ref["modules"] == ["model", "output", "aligner"]
    # the scheduler recoverable goes with lr_annealing
    assert ref["recoverables"] == ["model", "output", "scheduler", "counter"]
    assert list(m["checkpointer"].recoverables.keys()) == ["model", "output", "counter"]
    assert m["metric_keys"] == ["accuracy.average"] and m["max_key"] == "accuracy.average"
    assert (m["states_per_phoneme"], m["output_neurons"], m["blank_index"]) == (3, 123, 122)
    assert (m["dnn_blocks"], m["dnn_neurons"], m["lr"], m["n_epochs"]) == (1, 2000, 0.0003, 50)
    assert m["number_of_epochs"] == 10 and m["samples_per_frame"] == 320
    assert hp["sample_rate"] * hp["hop_length"] // 1000 == m["samples_per_frame"]
    assert (m["init_training_type"], m["switch_training_type"], m["switch_training_epoch"]) == \
        ("forward", "forward", 2)
    assert isinstance(m["model"], VanillaNN) and len(m["model"].blocks) == 1
    assert tuple(m["model"].blocks[0].w.weight.shape) == (2000, 120)
    assert isinstance(m["output"], Linear) and tuple(m["output"].w.weight.shape) == (123, 2000)
    assert m["output"].w.bias is not None
    a = m["aligner"]
    assert isinstance(a, HMMAligner) and m["modules"]["aligner"] is a
    assert (a.states_per_phoneme, a.batch_reduction, a.input_len_norm, a.target_len_norm) == \
        (3, "mean", True, False)
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    assert m["optimizer"].keywords == {"lr": 0.0003}
    assert m["epoch_counter"].limit == 50


def test_modules_surface():
    from modules.hmm_aligner import HMMAligner
    from modules.vanilla_nn import VanillaNN
    a = HMMAligner(states_per_phoneme=3)
    phns = torch.tensor([[0, 40, 2], [5, 0, 0]])
    exp = a.expand_phns_by_states_per_phoneme(phns, torch.tensor([1.0, 1 / 3]))
    assert exp.tolist() == [[0, 1, 2, 120, 121, 122, 6, 7, 8], [15, 16, 17, 0, 1, 2, 0, 1, 2]]
    assert exp.dtype == phns.dtype
    a.store_alignments(["u0", "u1"], torch.tensor([[0, 1], [2, -1]]))
    assert a.align_dict["u1"].tolist() == [2, -1]
    with pytest.raises(ValueError, match="batch_reduction"):
        HMMAligner(batch_reduction="max")
    with pytest.raises(ValueError, match="dp_algorithm"):
        a(torch.zeros(1, 2, 3), torch.ones(1), torch.zeros(1, 1, dtype=torch.long), torch.ones(1), "x")
    with pytest.raises(ValueError, match="LeakyReLU"):
        VanillaNN([None, None, 4], activation=torch.nn.ReLU, dnn_blocks=1, dnn_neurons=4)
    net = VanillaNN([None, None, 4], activation=torch.nn.LeakyReLU, dnn_blocks=2, dnn_neurons=6)
    assert [n for n, _ in net.named_parameters()] == ["blocks.0.w.weight", "blocks.0.w.bias",
                                                      "blocks.1.w.weight", "blocks.1.w.bias"]


def test_recipe_hooks(tmp_path):
    from brain import Stage
    from models.HMM_DNN_ALI.model import SBModel
    from models.md_model import MDModel
    from utils.metric_stats.align_acc_metric_stats import AlignAccMetricStats
    assert issubclass(SBModel, MDModel) and SBModel.dp_exact is False
    m = SBModel(modules={}, hparams={"metric_keys": ["accuracy.average"], "output_dir": str(tmp_path),
                                     "init_training_type": "viterbi"}, run_opts={"device": "cpu"})
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        m.on_stage_start(stage, 1)
        assert set(m.stats_loggers) == {"accuracy_stats"}
        assert isinstance(m.stats_loggers["accuracy_stats"], AlignAccMetricStats)
        assert m.training_type == "viterbi"


# --------------------------------------------------------------------------- corpus
def test_ali_labels_are_derived():
    from utils.data_io import SyntheticSet
    kw = dict(n_utts=12, feat_dim=6, min_frames=11, max_frames=90, seed=7, sorting=None, md_labels=True,
              n_phonemes=9, phn_labels=True)
    with_ali = SyntheticSet(ali_labels=True, samples_per_frame=320, **kw)
    without = SyntheticSet(**kw)
    for e, p in zip(with_ali.items, without.items):
        assert set(e) == set(p) | {"gt_phn_end_seq"}
        for k, v in p.items():
            assert torch.equal(e[k], v) if torch.is_tensor(v) else e[k] == v, k
        ends, T = e["gt_phn_end_seq"], e["feat"].shape[0]
        assert ends.dtype == torch.int64 and ends.shape == e["gt_cnncl_seq"].shape
        assert bool((ends[1:] > ends[:-1]).all()) and ends[0] > 0 and int(ends[-1]) == T * 320
        starts = torch.where(e["gt_boundary_seq"] == 1)[0]
        assert torch.equal(ends[:-1], starts[1:] * 320)
    with pytest.raises(ValueError, match="md_labels"):
        SyntheticSet(n_utts=2, feat_dim=6, min_frames=11, max_frames=20, seed=7, ali_labels=True)


# --------------------------------------------------------------------------- stats, argument checks
def test_align_acc_stats_from_counts():
    from utils.metric_stats.align_acc_metric_stats import AlignAccMetricStats
    counts = torch.tensor([[10, 10], [3, 9], [0, 7], [5, 8]], dtype=torch.int32)
    st = AlignAccMetricStats()
    st.append_counts(["a", "b"], counts[:2])
    st.append_counts(["c", "d"], counts[2:])
    assert st.scores_list == []
    want = hmm_np.accuracy_average(counts.numpy())
    assert st.summarize("average") == pytest.approx(want, rel=1e-6)
    assert st.ids == ["a", "b", "c", "d"] and list(st.summarize()) == ["average"]
    with pytest.raises(ValueError, match="counts must be"):
        st.append_counts(["a"], torch.zeros(1, 4, dtype=torch.int32))


def test_oracle_align_counts():
    phns = np.array([[4, 7, 4]])
    ends = np.array([[3 * 320, 5 * 320, 8 * 320]])
    ones = np.ones(1, dtype=np.float32)
    truth = np.array([[0, 0, 0, 1, 1, 2, 2, 2]]) * 2  # spp = 2: the first state of each phoneme
    assert hmm_np.align_counts(truth, ones, phns, ones, 2, ends, 320).tolist() == [[8, 8]]
    # phoneme 2 has phoneme 0's id: frame 2 of segment 0 aligned to it still counts; frame 5 (of
    # segment 2) aligned to phoneme 1 does not
    late = np.array([[0, 1, 4, 2, 2, 3, 4, 5]])
    assert hmm_np.align_counts(late, ones, phns, ones, 2, ends, 320).tolist() == [[7, 8]]


def test_lattice_ops_argument_checks_raise_before_any_launch():
    from mlvae_hip import ops
    pout, lens = torch.zeros(2, 5, 7), torch.ones(2)
    phns = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="hmm_forward"):
        ops.hmm_forward(torch.zeros(5, 7), lens, phns, lens, 1)
    with pytest.raises(ValueError, match="hmm_forward"):
        ops.hmm_forward(pout, lens, phns[:1], lens, 1)
    with pytest.raises(ValueError, match="states per phoneme"):
        ops.hmm_viterbi(pout, lens, phns, lens, 0)
    with pytest.raises(ValueError, match="lengths"):
        ops.ctc_nll(pout, torch.ones(3), phns, lens, 1, 6)
    with pytest.raises(TypeError, match="HIP tensor"):  # no CPU fallback
        ops.hmm_forward(pout, lens, phns, lens, 1)
    with pytest.raises(ValueError, match="center_log_softmax"):
        ops.center_log_softmax(torch.zeros(5, 7))
    with pytest.raises(TypeError, match="HIP tensor"):
        ops.center_log_softmax(pout)
    with pytest.raises(TypeError, match="align_counts"):
        ops.align_counts(torch.zeros(2, 5, dtype=torch.int32), lens, phns, lens, 1, phns, 320)
