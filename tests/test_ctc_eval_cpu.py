"""The CRDNN_CTC recipes' host-side parts (no GPU):

* the numpy oracle tests/ctc_np.py -- the definition of the kernels in csrc/ctc_eval.hip -- against
  hand-written cases: the greedy decode, the alignment's tie rule, an empty hypothesis, the
  Viterbi chain of a repeated phoneme (infeasible at T_b = 2, feasible at 3), the boundary count;
  its edit distance against a plain Levenshtein and its Viterbi score against the enumeration of
  every path;
* ErrorRateStats and MDMetricStats' aligned path from given counts, state() / merge() included,
  and the aligned path against the sequence path (the reference's PER branch);
* modules.crdnn.CRDNN's limits, both model yamls through load_hyperpyyaml with the reference's key
  names (tests/golden/crdnn_ctc_yaml_keys.json), the recipe's hooks and the ops' argument checks,
  which raise before any launch."""
import functools
import itertools
import json
import os

import numpy as np
import pytest
import torch

import ctc_np
from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLANK = 0


def _onehot(classes, C):
    lp = np.full((len(classes), C), -4.0)
    lp[np.arange(len(classes)), classes] = -0.5
    return lp


# --------------------------------------------------------------------------- greedy decode
def test_oracle_greedy_merges_repeats_and_drops_blanks():
    b = BLANK
    lp = _onehot([b, 1, 1, b, 1, 2, 2, b], 4)
    assert ctc_np.greedy_decode(lp, 8, b) == [1, 1, 2]
    assert ctc_np.greedy_decode(lp, 3, b) == [1]           # frames t >= T_b never contribute
    assert ctc_np.greedy_decode(lp, 0, b) == []
    tie = lp.copy()
    tie[1, 3] = tie[1, 1]                                  # classes 1 and 3 tie: the lowest wins
    assert ctc_np.greedy_decode(tie, 8, b) == [1, 1, 2]
    pred, n = ctc_np.greedy_batch(np.stack([lp, lp]), np.array([1.0, 0.5], dtype=np.float32), b)
    assert n.tolist() == [3, 1] and pred[0].tolist() == [1, 1, 2, -1, -1, -1, -1, -1]
    assert pred[1].tolist() == [1] + [-1] * 7


# --------------------------------------------------------------------------- edit alignment
def _levenshtein(a, b):
    d = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(b) + 1):
            prev, d[j] = d[j], min(prev + (a[i - 1] != b[j - 1]), d[j] + 1, d[j - 1] + 1)
    return d[len(b)]


def test_oracle_alignment_tie_rule():
    # the second 2 is the deletion: at (3, 2) the diagonal (1) ties the deletion (1) and loses
    ali, ops = ctc_np.edit_align([1, 2, 2, 3], [1, 2, 3])
    assert ali == [1, 2, -1, 3] and ops == (0, 1, 0, 4)
    ali, ops = ctc_np.edit_align([1, 2, 3], [])
    assert ali == [-1, -1, -1] and ops == (0, 3, 0, 3)       # an empty hypothesis: all deletions
    ali, ops = ctc_np.edit_align([], [4, 5])
    assert ali == [] and ops == (2, 0, 0, 0)                  # insertions are dropped
    ali, ops = ctc_np.edit_align([1, 2, 3], [1, 9, 3])
    assert ali == [1, 9, 3] and ops == (0, 0, 1, 3)
    ali, ops = ctc_np.edit_align([1, 2], [7, 1, 2, 8])
    assert ali == [1, 2] and ops == (2, 0, 0, 2)


def test_oracle_alignment_cost_is_the_edit_distance():
    g = np.random.default_rng(3)
    for _ in range(200):
        a = g.integers(0, 3, g.integers(0, 9)).tolist()
        b = g.integers(0, 3, g.integers(0, 9)).tolist()
        ali, (ins, dele, sub, n) = ctc_np.edit_align(a, b)
        assert n == len(a) == len(ali) and ins + dele + sub == _levenshtein(a, b)
        assert dele == sum(v == -1 for v in ali) and len(b) - ins == len(a) - dele
        kept = [v for v in ali if v != -1]                   # a subsequence of b, in order
        it = iter(b)
        assert all(any(v == w for w in it) for v in kept)


def test_oracle_md_counts():
    phn, cn, ali = [1, 2, 5, 4, 6], [1, 2, 3, 4, 7], [1, 9, 5, -1, 7]
    # pred_md = 0 1 1 1 0, gt_md = 0 0 1 0 1, wrong = 0 1 0 1 1
    assert ctc_np.md_counts(ali, phn, cn) == [1, 1, 1, 2, 3, 2, 2, 1]
    pred = np.array([[1, 9, 5, 7, -1]], dtype=np.int32)
    one = np.ones(1, dtype=np.float32)
    a, o, c = ctc_np.align_batch(pred, [4], np.array([phn]), one, np.array([cn]), one)
    assert a.shape == (1, 2, 5) and o.shape == (1, 2, 4) and c.shape == (1, 8)
    assert o[0, 0, 3] == o[0, 1, 3] == 5 and c[0, 4] + c[0, 6] == 5


# --------------------------------------------------------------------------- Viterbi
def _ctc_paths(T, N, skip):
    """Every node sequence of the CTC chain: start in 0 or 1, stay / next / allowed skip, end in
    one of the last two nodes."""
    out = []
    for start in range(min(2, N)):
        for steps in itertools.product((0, 1, 2), repeat=T - 1):
            u, path = start, [start]
            for s in steps:
                u += s
                if u >= N or (s == 2 and not skip[u]):
                    break
                path.append(u)
            else:
                if u >= N - 2:
                    out.append(path)
    return out


def test_oracle_viterbi_equals_path_enumeration():
    g = np.random.default_rng(8)
    for phns, T in (([1, 2], 5), ([3, 3], 5), ([2], 3), ([1, 2, 1], 6)):
        lp = g.standard_normal((T, 5))
        N = 2 * len(phns) + 1
        cls = np.full(N, BLANK)
        cls[1::2] = phns
        skip = [n >= 3 and n % 2 == 1 and cls[n] != cls[n - 2] for n in range(N)]
        paths = _ctc_paths(T, N, skip)
        scores = [sum(lp[t, cls[u]] for t, u in enumerate(p)) for p in paths]
        best = paths[int(np.argmax(scores))]
        score, bound, inf = ctc_np.ctc_viterbi(lp, phns, BLANK)
        assert not inf and abs(score - max(scores)) < 1e-12
        want = [int(t == 0 or (best[t] != best[t - 1] and best[t] % 2 == 1 and best[t] >= 3)) for t in range(T)]
        assert bound.tolist() == want and int(bound.sum()) == len(phns)


def test_oracle_viterbi_repeated_phoneme_needs_a_blank_between():
    lp = np.zeros((3, 5))
    score, bound, inf = ctc_np.ctc_viterbi(lp[:2], [3, 3], BLANK)
    assert inf and score == 0.0 and bound.tolist() == [1, 1]      # frames 0 .. min(L, T_b) - 1
    score, bound, inf = ctc_np.ctc_viterbi(lp, [3, 3], BLANK)
    assert not inf and bound.tolist() == [1, 0, 1]                 # 3, blank, 3: the only path
    score, bound, inf = ctc_np.ctc_viterbi(lp[:2], [3, 4], BLANK)
    assert not inf and bound.tolist() == [1, 1]                    # different classes: the skip
    score, bound, inf = ctc_np.ctc_viterbi(lp[:1], [3, 4], BLANK)
    assert inf and bound.tolist() == [1]
    score, bound, inf = ctc_np.ctc_viterbi(lp[:0], [3], BLANK)
    assert inf and bound.tolist() == []
    # all-equal emissions: every path ties; stay wins, so walking back the path rests in the final
    # blank for as long as it was reachable and the phonemes open as early as they can
    score, bound, inf = ctc_np.ctc_viterbi(np.zeros((6, 5)), [1, 2], BLANK)
    assert not inf and int(bound.sum()) == 2 and bound[0] == 1
    # a chain of 141 nodes: exactly L ones, one frame each, in T_b = L frames the diagonal
    long = np.arange(1, 71) % 4 + 1                                # no two neighbours alike
    score, bound, inf = ctc_np.ctc_viterbi(np.zeros((150, 5)), long, BLANK)
    assert not inf and int(bound.sum()) == 70
    score, bound, inf = ctc_np.ctc_viterbi(np.zeros((70, 5)), long, BLANK)
    assert not inf and bound.tolist() == [1] * 70
    vs, bd, infs = ctc_np.viterbi_batch(np.zeros((2, 4, 5)), np.array([1.0, 0.5], dtype=np.float32),
                                        np.array([[3, 3], [3, 3]]), np.ones(2, dtype=np.float32), BLANK)
    assert infs.tolist() == [0, 1] and bd[1].tolist() == [1, 1, -1, -1] and int((bd[0] == 1).sum()) == 2


# --------------------------------------------------------------------------- stats
def test_error_rate_stats_from_counts_and_merge():
    from utils.metric_stats.error_rate_stats import ErrorRateStats
    rows = torch.tensor([[1, 0, 2, 10], [0, 3, 0, 7], [0, 0, 0, 5], [2, 2, 2, 0]], dtype=torch.int32)
    st = ErrorRateStats()
    with pytest.raises(ValueError, match="No metrics"):
        st.summarize()
    st.append_counts(["a", "b"], rows[:2])
    st.append_counts(["c", "__pad__"], rows[2:])  # the filler row is not an utterance
    assert st.ids == []                            # nothing read before the summary
    s = st.summarize()
    assert s == {"error_rate": 100.0 * 6 / 22, "insertions": 1, "deletions": 3, "substitutions": 2,
                 "num_ref_tokens": 22}
    assert st.summarize("error_rate") == ctc_np.error_rate(rows[:3].numpy())
    assert st.ids == ["a", "b", "c"]
    with pytest.raises(ValueError, match="counts must be"):
        st.append_counts(["a"], rows[:1, :3])
    # two ranks: the rows come back in the single-process order
    r0, r1 = ErrorRateStats(), ErrorRateStats()
    r0.append_counts(["a"], rows[:1], batch_index=0)
    r1.append_counts(["b"], rows[1:2], batch_index=0)
    r0.append_counts(["c"], rows[2:3], batch_index=1)
    r1.append_counts(["__pad__"], rows[3:], batch_index=1)
    merged = ErrorRateStats()
    merged.merge([r0.state(), r1.state()])
    assert merged.ids == ["a", "b", "c"] and merged.summarize() == s
    empty = ErrorRateStats()
    empty.append_counts(["x"], torch.zeros(1, 4, dtype=torch.int32))
    assert empty.summarize("error_rate") == 0.0


def _aligned_case():
    phns = np.array([[1, 2, 5, 4, 6], [3, 3, 8, 0, 0]])
    cns = np.array([[1, 2, 3, 4, 7], [3, 4, 8, 0, 0]])
    pl = np.array([1.0, 0.6], dtype=np.float32)
    pred = np.array([[1, 9, 5, 7, -1, -1], [3, 8, -1, -1, -1, -1]], dtype=np.int32)
    ali, ops, counts = ctc_np.align_batch(pred, [4, 2], phns, pl, cns, pl)
    pb = np.array([[1, 0, 1, 1, 0, 1, 0, 1], [1, 1, 0, 1, 0, 0, -1, -1]], dtype=np.int32)
    gb = np.array([[1, 1, 0, 1, 0, 1, 1, 0], [1, 0, 1, 0, 1, 0, 0, 0]], dtype=np.float32)
    return phns, cns, ali, counts, pb, gb


def test_md_stats_aligned_path_equals_the_sequence_path(tmp_path):
    from utils.metric_stats.md_metric_stats import MDMetricStats, per_scoring
    phns, cns, ali, counts, pb, gb = _aligned_case()
    n = [5, 3]
    seq = MDMetricStats()
    seq.append(["u0", "u1"],
               pred_phn_seqs=[ali[i, 0, :n[i]].tolist() for i in range(2)],
               gt_phn_seqs=[phns[i, :n[i]].tolist() for i in range(2)],
               gt_cnncl_seqs=[cns[i, :n[i]].tolist() for i in range(2)],
               pred_boundary_seqs=[torch.tensor(pb[0]), torch.tensor(pb[1, :6])],
               gt_boundary_seqs=[torch.tensor(gb[0]), torch.tensor(gb[1, :6])])
    dev = MDMetricStats()
    dev.append_aligned(["u0", "u1"], torch.from_numpy(counts), torch.from_numpy(ali[:, 0]),
                       torch.from_numpy(phns), torch.from_numpy(cns),
                       pred_boundary=torch.from_numpy(pb), gt_boundary=torch.from_numpy(gb))
    assert dev.scores_list == []  # deferred to the summary
    a, b = seq.summarize(), dev.summarize()
    assert list(a) == list(b) and a == b
    assert {"ACC", "PRE", "REC", "F1", "soft_F1", "ave_iou", "correct_per", "misp_per"} <= set(a)
    for x, y in zip(seq.scores_list, dev.scores_list):
        assert {k: float(v) for k, v in x.items()} == {k: float(v) for k, v in y.items()}
    assert seq.saved_seqs == dev.saved_seqs
    # per_scoring by hand: 3 canonical positions of which 2 wrong, 2 mispronounced of which 1 wrong
    s = per_scoring([1, 9, 5, -1, 7], phns[0].tolist(), cns[0].tolist())
    assert float(s["correct_per"]) == pytest.approx(200 / 3, rel=1e-5)
    assert float(s["misp_per"]) == pytest.approx(50.0, rel=1e-5)
    # without boundaries: the plain scores and the PERs
    plain = MDMetricStats()
    plain.append_aligned(["u0", "u1"], torch.from_numpy(counts), torch.from_numpy(ali[:, 0]),
                         torch.from_numpy(phns), torch.from_numpy(cns))
    assert list(plain.summarize()) == ["ACC", "PRE", "REC", "F1", "correct_per", "misp_per"]
    assert plain.summarize("F1") == a["F1"]
    # merge of two ranks = the single process
    r0, r1 = MDMetricStats(), MDMetricStats()
    for r, st in enumerate((r0, r1)):
        st.append_aligned([f"u{r}"], torch.from_numpy(counts[r:r + 1]), torch.from_numpy(ali[r:r + 1, 0]),
                          torch.from_numpy(phns[r:r + 1]), torch.from_numpy(cns[r:r + 1]),
                          pred_boundary=torch.from_numpy(pb[r:r + 1]), gt_boundary=torch.from_numpy(gb[r:r + 1]),
                          batch_index=0)
    merged = MDMetricStats()
    merged.merge([r0.state(), r1.state()])
    assert merged.summarize() == b and merged.saved_seqs["utt_ids"] == ["u0", "u1"]
    dev.write_seqs_to_file(tmp_path / "seqs.txt")
    text = open(tmp_path / "seqs.txt").read()
    assert "ID: u0\nphn: 1 2 5 4 6\ncnncl: 1 2 3 4 7\npred_phn: " in text and "pred_md_lbl: " in text
    # a boundary count that does not match the phonemes is named
    bad = MDMetricStats()
    bad.append_aligned(["u0"], torch.from_numpy(counts[:1]), torch.from_numpy(ali[:1, 0]),
                       torch.from_numpy(phns[:1]), torch.from_numpy(cns[:1]),
                       pred_boundary=torch.from_numpy(pb[1:]), gt_boundary=torch.from_numpy(gb[:1]))
    with pytest.raises(ValueError, match="boundaries"):
        bad.summarize()


def test_md_stats_existing_call_forms_are_unchanged():
    from utils.metric_stats.md_metric_stats import batch_seq_md_scoring
    scores, seqs = batch_seq_md_scoring([[0, 1, 1]], [[0, 1, 0]])
    assert list(scores[0]) == ["ACC", "PRE", "REC", "F1"]
    assert seqs["gt_phn_seqs"] == seqs["pred_phn_seqs"] == seqs["gt_cnncl_seqs"] == [[7, 7, 7]]
    with pytest.raises(TypeError, match="must be list"):
        batch_seq_md_scoring(None, [[0]])


# --------------------------------------------------------------------------- module, yamls, recipe
def test_crdnn_limits_and_surface():
    from modules.crdnn import CRDNN
    from modules.lstm import LSTM
    with pytest.raises(NotImplementedError, match="cnn_blocks"):
        CRDNN(input_size=12, cnn_blocks=2)
    with pytest.raises(NotImplementedError, match="time_pooling"):
        CRDNN(input_size=12, time_pooling=True)
    with pytest.raises(ValueError, match="LeakyReLU"):
        CRDNN(input_size=12, activation=torch.nn.ReLU)
    net = CRDNN(input_size=12, activation=torch.nn.LeakyReLU, dropout=0.15, cnn_blocks=0,
                cnn_channels=(128, 256), cnn_kernelsize=(3, 3), time_pooling=False, rnn_layers=2,
                rnn_neurons=8, rnn_bidirectional=True, dnn_blocks=2, dnn_neurons=6)
    assert isinstance(net.rnn, LSTM) and net.rnn.bidirectional and net.rnn.num_layers == 2
    assert net.rnn.dropout == 0.15 and net.output_size == 6
    assert tuple(net.dnn[0].w.weight.shape) == (6, 16) and tuple(net.dnn[1].w.weight.shape) == (6, 6)
    with pytest.raises(RuntimeError, match="HIP device"):
        net(torch.zeros(1, 3, 12))  # no CPU fallback


@pytest.mark.parametrize("name", ["CRDNN_CTC", "CRDNN_CTC_cnncl"])
def test_model_yaml_resolves_with_the_reference_keys(name):
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import optim as hip_optim
    from modules.crdnn import CRDNN
    from modules.linear import Linear
    ov = (f"dataset: synthetic\nmodel_class: {name}\nmodel_name: ctc\n"
          f"model: !include:../models/{name}/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    m = hp["model"]
    with open(os.path.join(GOLD, "crdnn_ctc_yaml_keys.json")) as f:
        ref = json.load(f)
    assert set(ref["top_level"]) - set(m.keys()) == {"log_softmax", "scheduler", "compute_cost", "jit_module_keys"}
    assert {"blank_index", "time_pooling"} <= set(m.keys())
    assert list(m["modules"].keys()) == ref["modules"]
    assert list(m["checkpointer"].recoverables.keys()) == [k for k in ref["recoverables"] if k != "scheduler"]
    assert m["metric_keys"] == ref["metric_keys"][name] and m["max_key"] == "plvl_md.F1"
    assert (m["rnn_layers"], m["rnn_neurons"], m["rnn_bidirectional"], m["dnn_blocks"], m["dnn_neurons"]) == \
        (4, 512, True, 2, 512)
    assert (m["cnn_blocks"], m["time_pooling"], m["dropout"], m["lr"], m["n_epochs"]) == (0, False, 0.15, 1.0, 50)
    # the corpus ids are 0 .. n_phonemes - 1: the blank is a class none of them can take
    assert m["output_neurons"] == hp["n_phonemes"] + 2 == 41 and m["blank_index"] == 40 >= hp["n_phonemes"]
    assert isinstance(m["crdnn"], CRDNN) and m["crdnn"].rnn.input_size == 120
    assert (m["crdnn"].rnn.hidden_size, m["crdnn"].rnn.num_layers, m["crdnn"].rnn.bidirectional) == (512, 4, True)
    assert isinstance(m["output"], Linear) and tuple(m["output"].w.weight.shape) == (41, 512)
    assert isinstance(m["optimizer"], functools.partial) and m["optimizer"].func is hip_optim.Adam
    assert m["optimizer"].keywords == {"lr": 1.0}


def test_recipe_hooks_and_missing_fields(tmp_path):
    from brain import Stage
    from brain.dataio import PaddedBatch
    from models.CRDNN_CTC.model import SBModel
    from models.CRDNN_CTC_cnncl.model import SBModel as Cnncl
    from models.md_model import MDModel
    from utils.metric_stats.error_rate_stats import ErrorRateStats
    assert issubclass(SBModel, MDModel) and issubclass(Cnncl, SBModel) and SBModel.dp_exact is False
    # the subclass differs in compute_loss alone
    own = {k for k, v in vars(Cnncl).items() if callable(v)}
    assert own == {"compute_loss"}
    m = SBModel(modules={}, hparams={"metric_keys": ["phn_per.error_rate"], "output_dir": str(tmp_path),
                                     "blank_index": 40}, run_opts={"device": "cpu"})
    for stage in (Stage.TRAIN, Stage.VALID, Stage.TEST):
        m.on_stage_start(stage, 1)
        assert set(m.stats_loggers) == {"phn_per_stats", "cnncl_per_stats", "plvl_md_stats", "boundary_stats"}
        assert isinstance(m.stats_loggers["phn_per_stats"], ErrorRateStats)
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    b.update({"id": ["u"], "feat": (torch.zeros(1, 4, 3), torch.ones(1)),
              "gt_cnncl_seq": (torch.zeros(1, 2, dtype=torch.long), torch.ones(1))})
    with pytest.raises(ValueError, match="gt_phn_seq.*waveforms: true"):
        m.compute_forward(b, Stage.TRAIN)


def test_applied_normaliser_round_trips_through_a_checkpoint():
    # the recipe applies its normaliser and checkpoints it: the statistics (shaped by the first
    # batch) load into a freshly built one, which test.py does
    from brain.features import InputNormalization
    g = torch.Generator().manual_seed(1)
    x, lens = torch.randn(3, 9, 6, generator=g) * 2 + 1, torch.tensor([1.0, 0.75, 0.5])
    seen = InputNormalization(norm_type="global")
    seen.train()
    seen(x, lens, epoch=1)
    fresh = InputNormalization(norm_type="global")
    fresh.load_state_dict(seen.state_dict())
    assert torch.equal(fresh.glob_mean, seen.glob_mean) and torch.equal(fresh.glob_std, seen.glob_std)
    assert fresh.glob_mean.shape == (6,) and fresh.count == 1
    seen.eval(), fresh.eval()
    assert torch.equal(fresh(x, lens, epoch=1), seen(x, lens, epoch=1))
    empty = InputNormalization(norm_type="global")
    empty.load_state_dict(InputNormalization(norm_type="global").state_dict())  # never applied: as before
    assert empty.glob_mean.numel() == 0 and empty.count == 0


def test_ops_argument_checks_raise_before_any_launch():
    from mlvae_hip import ops
    pout, lens = torch.zeros(2, 5, 7), torch.ones(2)
    phns = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(TypeError, match="float32 HIP tensor"):
        ops.ctc_greedy_decode(pout, lens, 6)
    with pytest.raises(ValueError, match=r"pout must be \[B, T, C\]"):
        ops.ctc_greedy_decode(pout[0], lens, 6)
    with pytest.raises(ValueError, match=r"pout must be \[B, T, C\]"):
        ops.ctc_viterbi(pout[0], lens, phns, lens, 6)
    with pytest.raises(TypeError, match="int32"):
        ops.edit_align(torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), phns, lens,
                       phns, lens)
    with pytest.raises(TypeError, match="int32"):
        ops.ctc_md_counts(torch.zeros(2, 2, 3), phns, lens, phns, lens)
    with pytest.raises(ValueError, match="C >= 1"):
        ops.log_softmax(torch.zeros(3, 0))
