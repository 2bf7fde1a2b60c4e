"""The CRDNN_CTC recipes with the convolutional front end (model_cnn.yaml: modules.crdnn.ConvCRDNN,
2 CNN blocks, time pooling) on the HIP path, on the tiny spoken corpus of test_gpu_crdnn_ctc.py
(16 utterances of 40-60 frames, 7 phonemes, batch 4); the net: channels (16, 32), 2 x 32 LSTM, a
32-wide DNN, bf16 operands (the Conv2d kernels' only form).

* One training batch: pout has T // 2 frames; the loss and every gradient, the front's included,
  against F.ctc_loss(reduction='mean', zero_infinity=True) composed on the same device pout
  (1e-5 relative on the loss, 1e-4 relative-max on the gradients: test_gpu_crdnn_ctc.py's bounds).
* A VALID pass: no infeasible utterance; the logged metrics equal the numpy oracle tests/ctc_np.py
  on the dumped pout -- greedy decode and alignments on its T // 2 frames, the Viterbi boundaries
  on pout resampled to the features' frames by the reference's rule (each frame repeated T // T'
  times, then cut or zero-padded), restated here in numpy.  Counts exact, error rates to 1e-9.
* train.py then test.py through the command line with model_cnn.yaml for both recipes."""
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
from test_gpu_crdnn_ctc import BLANK, BS, C, H, KEYS, NPH, _lengths, corpus  # noqa: F401  (corpus: the fixture)
from test_gpu_md_vae import _script

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _bf16_products():
    from mlvae_hip import ops
    with ops.precision("bf16"):
        yield


def _model(tmp_path, name="CRDNN_CTC"):
    import importlib
    from brain.features import InputNormalization
    from modules.crdnn import ConvCRDNN
    from modules.linear import Linear
    SBModel = importlib.import_module(f"models.{name}.model").SBModel
    torch.manual_seed(3)
    norm = InputNormalization(norm_type="global")
    modules = {"crdnn": ConvCRDNN(120, torch.nn.LeakyReLU, 0.15, 2, (16, 32), (3, 3), True, 2, H, True, 2, H),
               "output": Linear(H, C), "normalizer": norm}
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1), normalizer=norm, blank_index=BLANK,
                   batch_size=BS, metric_keys=KEYS, max_key="plvl_md.F1", output_dir=str(tmp_path))
    return SBModel(modules=modules, hparams=hparams, run_opts={"device": "cuda:0"})


def _train_batch(tmp_path, corpus, name, composed_target=None):
    """As test_gpu_crdnn_ctc._train_batch: the same weights, dropout key and Dropout2d masks every
    time (torch.manual_seed seeds the device generator the masks are drawn from)."""
    from brain import Stage
    m = _model(tmp_path, name)
    m.modules.train()
    batch = next(b for b in corpus.batches(batch_size=BS)
                 if not torch.equal(b["gt_phn_seq"][0], b["gt_cnncl_seq"][0]))
    m.on_stage_start(Stage.TRAIN, 1)
    torch.manual_seed(11)
    pred = m.compute_forward(batch, Stage.TRAIN)
    pout = pred["pout"]
    if composed_target is None:
        loss = m.compute_objectives(pred, batch, Stage.TRAIN)
    else:
        Tb, Ub = _lengths(batch, "feat", pout.shape[1]), _lengths(batch, composed_target)
        loss = torch.nn.functional.ctc_loss(pout.transpose(0, 1), batch[composed_target][0].cuda(), Tb, Ub,
                                            blank=BLANK, reduction="mean", zero_infinity=True)
    loss.backward()
    return loss.item(), {n: p.grad.clone() for n, p in m.modules.named_parameters()}, pout.detach(), batch


@pytest.mark.parametrize("name,target", [("CRDNN_CTC", "gt_phn_seq"), ("CRDNN_CTC_cnncl", "gt_cnncl_seq")])
def test_training_batch_equals_the_composed_ctc_loss(tmp_path, corpus, name, target):
    from mlvae_hip import ops
    loss, got, pout, batch = _train_batch(tmp_path, corpus, name)
    ref, want, pout_ref, _ = _train_batch(tmp_path, corpus, name, composed_target=target)
    T = batch["feat"][0].shape[1]
    assert pout.shape == (BS, T // 2, C) and torch.equal(pout, pout_ref)  # time-pooled; the same forward
    assert len(got) == 16 + 2 * 2 * 4 + 2 * 2 + 2  # the front's 2 blocks x 8, the LSTM, the DNN, the output
    assert sum(n.startswith("crdnn.front.block_") for n in got) == 16
    e_loss = abs(loss - ref) / abs(ref)
    print(f"{name}: loss {loss:.7f} composed {ref:.7f} rel {e_loss:.2e}")
    assert e_loss < 1e-5 and ref > 0
    for n in got:
        e = rel_err(got[n], want[n])
        print(f"{name} grad {n} rel {e:.2e}")
        assert want[n].abs().max() > 0 and e < 1e-4, (n, e)
    ops.raise_ctc_eval_err()


def _resample_np(pout, T):
    """The reference's resample_tensor rule on [B, T', C]."""
    f = T // pout.shape[1]
    out = np.repeat(pout, f, axis=1)[:, :T]
    if out.shape[1] < T:
        out = np.concatenate([out, np.zeros((out.shape[0], T - out.shape[1], out.shape[2]), out.dtype)], axis=1)
    return out


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
            assert pred["pout"].shape[1] == batch["feat"][0].shape[1] // 2
            dumped.append((batch, pred["pout"].cpu().numpy()))
    assert len(dumped) == 4
    assert m.infeasible.is_cuda and int(m.infeasible) == 0
    m.on_stage_end(Stage.VALID, 0.0, 1)
    log = m._collect_metrics(0.0)

    md, bnd, edits = MDMetricStats(), BoundaryMetricStats(), {0: [], 1: []}
    for batch, pout in dumped:
        lens = batch["feat"][1].cpu().numpy()
        Tf = batch["feat"][0].shape[1]
        phns, pl = (x.cpu().numpy() for x in batch["gt_phn_seq"])
        cns, cl = (x.cpu().numpy() for x in batch["gt_cnncl_seq"])
        hyp, n = ctc_np.greedy_batch(pout, lens, BLANK)          # on the pooled frames
        ali, ops_, _ = ctc_np.align_batch(hyp, n, phns, pl, cns, cl)
        up = _resample_np(pout, Tf)                               # the boundaries on the features' frames
        assert up.shape[1] == Tf
        _, bd, inf = ctc_np.viterbi_batch(up, lens, cns, cl, BLANK)
        assert not inf.any()
        for r in (0, 1):
            edits[r].append(ops_[:, r])
        L = [ctc_np.round_len(v, phns.shape[1]) for v in pl]
        T = [ctc_np.round_len(v, Tf) for v in lens]
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
    for r, key in enumerate(("phn_per_stats", "cnncl_per_stats")):
        assert m.stats_loggers[key].rows == np.concatenate(edits[r]).tolist()
    assert m.stats_loggers["plvl_md_stats"].saved_seqs == md.saved_seqs


@pytest.mark.parametrize("name", ["CRDNN_CTC", "CRDNN_CTC_cnncl"])
def test_train_and_test_scripts_with_model_cnn_yaml(tmp_path, name):
    """lr 0.01 and 4 epochs, the settings of test_gpu_crdnn_ctc.py's script test."""
    need_gpu()
    overrides = ("{n_phonemes: 7, batch_size: 4, synthetic: {md_labels: true, waveforms: true, n_train: 16, "
                 "n_valid: 8, n_test: 8, min_frames: 40, max_frames: 60}, model: {n_epochs: 4, cnn_channels: [16, 32], "
                 "rnn_neurons: 32, rnn_layers: 2, dnn_neurons: 32, lr: 0.01}}")
    common = ["config/run.yaml", "--model_class", name, "--model_name", "crdnn_cnn_ci",
              "--model", f"!include:../models/{name}/model_cnn.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    losses = [float(x) for x in re.findall(r"train loss: ([-+0-9.eE]+)", log)]
    print(f"{name} (model_cnn.yaml): training CTC loss per epoch {losses}")
    assert len(losses) == 4 and losses[-1] < losses[0], log[-2000:]
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1 and all(os.path.exists(os.path.join(ckpts[0], f"{k}.ckpt")) for k in ("crdnn", "output"))
    state = torch.load(os.path.join(ckpts[0], "crdnn.ckpt"), map_location="cpu")
    assert tuple(state["front.block_1.conv_2.weight"].shape) == (32, 32, 3, 3)
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
