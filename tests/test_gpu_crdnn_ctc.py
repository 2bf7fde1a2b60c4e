"""The CRDNN_CTC recipes (models/CRDNN_CTC, models/CRDNN_CTC_cnncl) on the HIP path, on a tiny
spoken corpus (16 utterances of 40-60 frames, 7 phonemes), rnn_neurons = dnn_neurons = 32,
rnn_layers = 2, batch 4.

* One training batch: the loss and every parameter gradient against the composed form --
  F.ctc_loss(reduction='mean', zero_infinity=True) on the same device log-posteriors under
  autograd -- at the bounds tests/test_gpu_align.py holds the lattice to: 1e-5 relative on the
  loss, 1e-4 relative-max on the gradients.  Both recipes (they differ in the target sequence).
* A VALID pass: nothing comes to the host per batch; the metrics the stage logs equal the numpy
  oracle tests/ctc_np.py run on the pass's own log-posteriors and scored through the stats' host
  paths (counts exact, so the rounded scores are equal; the error rates to 1e-9).
* train.py then test.py through the command line for both recipes: checkpoint, test_metrics.txt
  with every metric key, md_result_seqs.txt, and a training loss that went down.
(The reference recipes need SpeechBrain and ctc_segmentation and cannot run here: there is no
recorded fixture.)  Reference ops: ref:src/models/CRDNN_CTC/model.py:22-176."""
import glob
import os
import re
import types

import numpy as np
import pytest
import torch

import ctc_np
from conftest import PKG
from gpu_utils import need_gpu, rel_err
from test_gpu_md_vae import _script

pytestmark = pytest.mark.gpu

NPH, H, BS = 7, 32, 4
C, BLANK = NPH + 2, NPH + 1
KEYS = ["phn_per.error_rate", "cnncl_per.error_rate", "plvl_md", "boundary"]


@pytest.fixture(scope="module")
def corpus():
    need_gpu()
    from brain.features import Fbank
    from utils.data_io import SyntheticSet
    cf = Fbank(deltas=True, sample_rate=16000, hop_length=20, n_fft=400, n_mels=40)
    return SyntheticSet(16, 120, 40, 60, 4242, md_labels=True, n_phonemes=NPH, waveforms=True, compute_features=cf)


def _model(tmp_path, name="CRDNN_CTC"):
    import importlib
    from brain.features import InputNormalization
    from modules.crdnn import CRDNN
    from modules.linear import Linear
    SBModel = importlib.import_module(f"models.{name}.model").SBModel
    torch.manual_seed(3)
    norm = InputNormalization(norm_type="global")
    modules = {"crdnn": CRDNN(120, torch.nn.LeakyReLU, 0.15, 0, (128, 256), (3, 3), False, 2, H, True, 2, H),
               "output": Linear(H, C), "normalizer": norm}
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1), normalizer=norm, blank_index=BLANK,
                   batch_size=BS, metric_keys=KEYS, max_key="plvl_md.F1", output_dir=str(tmp_path))
    return SBModel(modules=modules, hparams=hparams, run_opts={"device": "cuda:0"})


def _lengths(batch, key, width=None):
    seqs, lens = batch[key]
    n = seqs.shape[1] if width is None else width
    return torch.tensor([ctc_np.round_len(v, n) for v in lens.float().cpu().numpy()])


def _train_batch(tmp_path, corpus, name, composed_target=None):
    """One training batch on a freshly built model (the same weights and the same dropout key every
    time: _model and this function seed torch): (loss, {name: gradient}, pout, model, predictions,
    batch).  composed_target: the loss is F.ctc_loss on the model's device log-posteriors instead of
    the recipe's."""
    from brain import Stage
    m = _model(tmp_path, name)
    m.modules.train()  # inter-layer dropout on
    # a batch with a mispronunciation in it: the pronounced and the canonical targets differ
    batch = next(b for b in corpus.batches(batch_size=BS)
                 if not torch.equal(b["gt_phn_seq"][0], b["gt_cnncl_seq"][0]))
    m.on_stage_start(Stage.TRAIN, 1)
    torch.manual_seed(11)  # the dropout key is drawn from torch's generator
    pred = m.compute_forward(batch, Stage.TRAIN)
    pout = pred["pout"]
    if composed_target is None:
        loss = m.compute_objectives(pred, batch, Stage.TRAIN)
    else:
        Tb, Ub = _lengths(batch, "feat", pout.shape[1]), _lengths(batch, composed_target)
        loss = torch.nn.functional.ctc_loss(pout.transpose(0, 1), batch[composed_target][0].cuda(), Tb, Ub,
                                            blank=BLANK, reduction="mean", zero_infinity=True)
    loss.backward()  # one backward per graph: the recurrence's backward consumes its saved gates
    return loss.item(), {n: p.grad.clone() for n, p in m.modules.named_parameters()}, pout.detach(), m, pred, batch


@pytest.mark.parametrize("name,target", [("CRDNN_CTC", "gt_phn_seq"), ("CRDNN_CTC_cnncl", "gt_cnncl_seq")])
def test_training_batch_equals_the_composed_ctc_loss(tmp_path, corpus, name, target):
    from mlvae_hip import ops
    loss, got, pout, m, pred, batch = _train_batch(tmp_path, corpus, name)
    ref, want, pout_ref, _, _, _ = _train_batch(tmp_path, corpus, name, composed_target=target)
    assert pout.shape[0] == BS and pout.shape[2] == C and torch.equal(pout, pout_ref)  # the same forward
    assert len(got) == 2 * 2 * 4 + 2 * 2 + 2  # 2 layers x 2 directions x 4, the DNN, the output
    e_loss = abs(loss - ref) / abs(ref)
    print(f"{name}: loss {loss:.7f} composed {ref:.7f} rel {e_loss:.2e}")
    assert e_loss < 1e-5 and ref > 0
    for n in got:
        e = rel_err(got[n], want[n])
        print(f"{name} grad {n} rel {e:.2e}")
        assert e < 1e-4, (n, e)
    if name == "CRDNN_CTC_cnncl":  # the two recipes train on different sequences
        with torch.no_grad():
            other = m._ctc_loss(pred, batch, "gt_phn_seq")
        assert abs(other.item() - loss) > 1e-6 * abs(loss)
    ops.raise_ctc_eval_err()


def test_valid_pass_metrics_equal_the_oracle(tmp_path, corpus):
    from brain import Stage
    from brain.train_logger import FileTrainLogger
    from utils.data_utils import undo_padding
    from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
    from utils.metric_stats.md_metric_stats import MDMetricStats
    m = _model(tmp_path)
    m.modules.eval()
    m.train_logger = FileTrainLogger(tmp_path / "train_log.txt")
    m.on_stage_start(Stage.VALID, 1)
    dumped = []
    with torch.no_grad():
        for batch in corpus.batches(batch_size=BS):
            pred = m.compute_forward(batch, Stage.VALID)
            m.compute_objectives(pred, batch, Stage.VALID)
            dumped.append((batch, pred["pout"].cpu().numpy()))
    assert len(dumped) == 4
    for key in ("phn_per_stats", "cnncl_per_stats", "plvl_md_stats", "boundary_stats"):
        st = m.stats_loggers[key]
        assert st.ids == [] and getattr(st, "scores_list", []) == []  # nothing brought to the host per batch
    assert m.infeasible.is_cuda and int(m.infeasible) == 0
    m.on_stage_end(Stage.VALID, 0.0, 1)
    log = m._collect_metrics(0.0)
    line = open(tmp_path / "train_log.txt").read()
    assert all(f"valid {k}" in line for k in log)

    # the oracle on the dumped log-posteriors, scored through the stats' host paths
    md, bnd, edits = MDMetricStats(), BoundaryMetricStats(), {0: [], 1: []}
    for batch, pout in dumped:
        lens = batch["feat"][1].cpu().numpy()  # compute_forward moved the batch to the device
        phns, pl = (x.cpu().numpy() for x in batch["gt_phn_seq"])
        cns, cl = (x.cpu().numpy() for x in batch["gt_cnncl_seq"])
        hyp, n = ctc_np.greedy_batch(pout, lens, BLANK)
        ali, ops_, _ = ctc_np.align_batch(hyp, n, phns, pl, cns, cl)
        _, bd, inf = ctc_np.viterbi_batch(pout, lens, cns, cl, BLANK)
        assert not inf.any()
        for r in (0, 1):
            edits[r].append(ops_[:, r])
        L = [ctc_np.round_len(v, phns.shape[1]) for v in pl]
        T = [ctc_np.round_len(v, pout.shape[1]) for v in lens]
        pb = [torch.from_numpy(bd[i, :T[i]]) for i in range(len(L))]
        gb = [torch.tensor(s) for s in undo_padding(*(x.cpu() for x in batch["gt_boundary_seq"]))]
        md.append(batch["id"], pred_phn_seqs=[ali[i, 0, :L[i]].tolist() for i in range(len(L))],
                  gt_phn_seqs=[phns[i, :L[i]].tolist() for i in range(len(L))],
                  gt_cnncl_seqs=[cns[i, :L[i]].tolist() for i in range(len(L))],
                  pred_boundary_seqs=pb, gt_boundary_seqs=gb)
        bnd.append(batch["id"], predictions=pb, targets=gb)
    want = {"phn_per.error_rate": round(ctc_np.error_rate(np.concatenate(edits[0])), 2),
            "cnncl_per.error_rate": round(ctc_np.error_rate(np.concatenate(edits[1])), 2)}
    want.update({f"plvl_md.{k}": v for k, v in md.summarize().items()})
    want.update({f"boundary.{k}": v for k, v in bnd.summarize().items()})
    print({k: (log[k], want[k]) for k in want})
    assert set(want) | {"loss"} == set(log)
    for k, v in want.items():
        if k.endswith("error_rate"):
            assert log[k] == pytest.approx(v, abs=1e-9), k
        else:
            assert log[k] == v, k
    # the counts themselves, exactly
    for r, key in enumerate(("phn_per_stats", "cnncl_per_stats")):
        assert m.stats_loggers[key].rows == np.concatenate(edits[r]).tolist()
    assert m.stats_loggers["plvl_md_stats"].saved_seqs == md.saved_seqs
    assert 0 < log["phn_per.error_rate"] and "plvl_md.correct_per" in log and "plvl_md.soft_F1" in log


@pytest.mark.parametrize("name", ["CRDNN_CTC", "CRDNN_CTC_cnncl"])
def test_train_and_test_scripts(tmp_path, name):
    need_gpu()
    overrides = ("{n_phonemes: 7, batch_size: 4, synthetic: {md_labels: true, waveforms: true, n_train: 16, "
                 "n_valid: 8, n_test: 8, min_frames: 40, max_frames: 60}, model: {n_epochs: 4, rnn_neurons: 32, "
                 "rnn_layers: 2, dnn_neurons: 32, lr: 0.01}}")
    common = ["config/run.yaml", "--model_class", name, "--model_name", "crdnn_ctc_ci",
              "--model", f"!include:../models/{name}/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    losses = [float(x) for x in re.findall(r"train loss: ([-+0-9.eE]+)", log)]
    print(f"{name}: training CTC loss per epoch {losses}")
    assert len(losses) == 4 and losses[-1] < losses[0], log[-2000:]
    assert len([l for l in log.splitlines() if "valid plvl_md.F1" in l]) == 4
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1 and all(os.path.exists(os.path.join(ckpts[0], f"{k}.ckpt")) for k in ("crdnn", "output"))
    assert any("plvl_md.F1" in open(os.path.join(c, "CKPT.yaml")).read() for c in ckpts)
    r = _script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    print(metrics.splitlines()[-1])
    keys = (["phn_per.error_rate", "cnncl_per.error_rate"] +
            [f"plvl_md.{k}" for k in ("ACC", "PRE", "REC", "F1")] +
            (["plvl_md.correct_per", "plvl_md.misp_per", "plvl_md.soft_F1", "boundary.f1", "boundary.r_value"]
             if name == "CRDNN_CTC" else []))
    assert all(f"{k}: " in metrics for k in keys), metrics
    seqs = open(tmp_path / "out" / "test_output" / "md_result_seqs.txt").read()
    assert seqs.count("ID: ") == 8 and seqs.count("pred_md_lbl: ") == 8
    blocks = dict(b.split("\n", 1) for b in seqs.strip().split("\n\nID: "))
    assert all(len({len(l.split(": ", 1)[1].split()) for l in body.strip().splitlines()}) == 1
               for body in blocks.values())  # five rows of one length per utterance
