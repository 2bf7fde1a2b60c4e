"""The HMM_DNN_ALI recipe (models/HMM_DNN_ALI) on the HIP path.

* compute_forward + compute_objectives at B = 3, T = 24, F = 8, dnn_neurons = 16, 5 phonemes,
  spp = 3 for the 'forward' and 'ctc' objectives against the same network in torch CPU float64
  with the losses of the float64 oracle tests/hmm_np.py: the loss at 1e-5 relative, every
  parameter gradient at 1e-4 relative-max.  (The reference recipe needs SpeechBrain and cannot
  run here: there is no recorded fixture.)
* 'viterbi' training raises NotImplementedError.
* Nothing comes to the host per batch: the stats hold device counts only, accuracy.average is the
  oracle's on the model's own posteriors, and a bad batch raises at the stage's end.
* train.py / test.py end to end on the synthetic corpus with md_labels and ali_labels.
Reference ops: ref:src/models/HMM_DNN_ALI/model.py:16-91."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

import hmm_np
from conftest import PKG
from gpu_utils import need_gpu, rel_err
from test_gpu_md_vae import _script

pytestmark = pytest.mark.gpu

B, T, F, H, NPH, SPP, L, SPF = 3, 24, 8, 16, 5, 3, 3, 320
C = SPP * (NPH + 2)
LENS = [1.0, 0.75, 0.5]        # 24, 18, 12 frames
PHN_LENS = [1.0, 1.0, 2 / 3]   # 3, 3, 2 phonemes: 9, 9, 6 states


def _model(tmp_path, training_type):
    from models.HMM_DNN_ALI.model import SBModel
    from modules.hmm_aligner import HMMAligner
    from modules.linear import Linear
    from modules.vanilla_nn import VanillaNN
    torch.manual_seed(5)
    aligner = HMMAligner(SPP, "mean", True, False)
    modules = {"model": VanillaNN([None, None, F], torch.nn.LeakyReLU, 1, H),
               "output": Linear(H, C), "aligner": aligner}
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1), aligner=aligner, blank_index=C - 1,
                   samples_per_frame=SPF, init_training_type=training_type, states_per_phoneme=SPP,
                   batch_size=B, metric_keys=["accuracy.average"], max_key="accuracy.average",
                   output_dir=str(tmp_path))
    m = SBModel(modules=modules, hparams=hparams, run_opts={"device": "cuda:0"})
    assert [n for n, _ in m.modules.named_parameters()] == [
        "model.blocks.0.w.weight", "model.blocks.0.w.bias", "output.w.weight", "output.w.bias"]
    return m


def _batch(lens=LENS):
    from brain.dataio import PaddedBatch
    g = torch.Generator().manual_seed(11)
    feat = torch.randn(B, T, F, generator=g)  # padded rows non-zero: they enter the mean
    phns = torch.tensor([[1, 1, 4], [0, 3, 2], [2, 0, 0]])
    ends = torch.tensor([[7, 15, 24], [5, 11, 18], [6, 12, 0]]) * SPF
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    pl = torch.tensor(PHN_LENS, dtype=torch.float32)
    b.update({"id": [f"utt{i}" for i in range(B)], "feat": (feat, torch.tensor(lens, dtype=torch.float32)),
              "gt_cnncl_seq": (phns, pl), "gt_phn_end_seq": (ends, pl)})
    return b


def _reference(m, batch, training_type):
    """The same network in torch CPU float64; the loss and d loss / d pout from the oracle."""
    p = {n: v.detach().double().cpu().requires_grad_(True) for n, v in m.modules.named_parameters()}
    x = batch["feat"][0].double().cpu()
    h = torch.nn.functional.leaky_relu(x @ p["model.blocks.0.w.weight"].T + p["model.blocks.0.w.bias"], 0.01)
    out = h @ p["output.w.weight"].T + p["output.w.bias"]
    out.retain_grad()
    pout = torch.log_softmax(out - out.mean(1).unsqueeze(1), -1)
    lens, pl = np.array(LENS, dtype=np.float32), np.array(PHN_LENS, dtype=np.float32)
    phns = batch["gt_cnncl_seq"][0].cpu().numpy()
    topo = hmm_np.HMM if training_type == "forward" else hmm_np.CTC
    score, dp, ok = hmm_np.lattice_batch(pout.detach().numpy(), lens, phns, pl, SPP, topo, C - 1)
    assert ok.all()
    if training_type == "forward":
        den = np.array([hmm_np.round_len(v, T) for v in lens], dtype=np.float64)
    else:
        den = np.array([hmm_np.round_len(v, L) * SPP for v in pl], dtype=np.float64)
    loss = float(np.mean(-score / den))
    pout.backward(torch.from_numpy(-dp / (B * den)[:, None, None]))
    grads = {n: v.grad for n, v in p.items()}
    # the output bias is the same for every frame, and the centring subtracts the mean over the
    # frames: its gradient, sum_{b,t} d out[b, t, :], is identically 0 (1e-25 in float64), so a
    # ratio to its own maximum is undefined.  It is a cancelling sum: its error is measured
    # against the largest sum of the magnitudes of its terms instead.
    assert grads["output.w.bias"].abs().max() < 1e-12 * out.grad.abs().sum((0, 1)).max()
    return pout.detach(), loss, grads, out.grad.abs().sum((0, 1)).max().item()


@pytest.mark.parametrize("training_type", ["forward", "ctc"])
def test_objectives_match_the_float64_network(tmp_path, training_type):
    need_gpu()
    from brain import Stage
    from mlvae_hip import ops
    m = _model(tmp_path, training_type)
    m.modules.train()
    batch = _batch()
    m.on_stage_start(Stage.TRAIN, 1)
    pred = m.compute_forward(batch, Stage.TRAIN)
    loss = m.compute_objectives(pred, batch, Stage.TRAIN)
    loss.backward()
    pout, want, grads, bias_terms = _reference(m, batch, training_type)
    e_out, e_loss = rel_err(pred[0], pout), abs(loss.item() - want) / abs(want)
    print(f"{training_type}: pout rel {e_out:.2e}, loss {loss.item():.7f} ref {want:.7f} rel {e_loss:.2e}")
    assert pred[0].shape == (B, T, C) and e_out < 1e-5 and e_loss < 1e-5
    for n, p in m.modules.named_parameters():
        if n == "output.w.bias":  # identically 0 (see _reference): against the sum of its terms
            e = (p.grad.double().cpu() - grads[n]).abs().max().item() / bias_terms
        else:
            e = rel_err(p.grad, grads[n])
        print(f"{training_type} grad {n} rel {e:.2e}")
        assert e < 1e-4, (n, e)
    # the alignments are stored only when training on the forward score
    stored = m.hparams.aligner.align_dict
    assert (sorted(stored) == batch["id"]) == (training_type == "forward")
    ops.raise_align_err()


def test_viterbi_training_is_not_implemented(tmp_path):
    need_gpu()
    from brain import Stage
    m = _model(tmp_path, "viterbi")
    batch = _batch()
    m.on_stage_start(Stage.TRAIN, 1)
    pred = m.compute_forward(batch, Stage.TRAIN)
    with pytest.raises(NotImplementedError, match="viterbi"):
        m.compute_objectives(pred, batch, Stage.TRAIN)


def test_counts_stay_on_the_device_and_score_as_the_oracle(tmp_path):
    need_gpu()
    from brain import Stage
    m = _model(tmp_path, "forward")
    m.modules.eval()
    batch = _batch()
    m.on_stage_start(Stage.TEST, 1)
    with torch.no_grad():
        pred = m.compute_forward(batch, Stage.TEST)
        m.compute_objectives(pred, batch, Stage.TEST)
    st = m.stats_loggers["accuracy_stats"]
    assert st.scores_list == [] and st.ids == []  # nothing brought to the host per batch
    assert all(c.is_cuda for _, c, _ in st._pending)
    lens, pl = np.array(LENS, dtype=np.float32), np.array(PHN_LENS, dtype=np.float32)
    phns, ends = batch["gt_cnncl_seq"][0].cpu().numpy(), batch["gt_phn_end_seq"][0].cpu().numpy()
    _, al = hmm_np.viterbi_batch(pred[0].cpu().numpy(), lens, phns, pl, SPP)
    want = hmm_np.accuracy_average(hmm_np.align_counts(al, lens, phns, pl, SPP, ends, SPF))
    m.on_stage_end(Stage.TEST, 0.0, 1)
    got = st.summarize("average")
    print(f"accuracy.average {got:.4f} oracle {want:.4f}")
    assert got == pytest.approx(want, rel=1e-6) and 0 < got <= 100
    assert "accuracy.average" in open(tmp_path / "test_output" / "test_metrics.txt").read()
    starts = json.load(open(tmp_path / "test_output" / "alignments.json"))
    assert sorted(starts) == batch["id"]
    for i, u in enumerate(batch["id"]):
        ph = al[i][al[i] >= 0] // SPP
        assert starts[u] == [int(np.argmax(ph == k)) for k in range(int(ph.max()) + 1)]
        assert starts[u][0] == 0 and all(a < b for a, b in zip(starts[u], starts[u][1:]))


def test_bad_batch_raises_at_the_stage_end(tmp_path):
    need_gpu()
    from brain import Stage
    m = _model(tmp_path, "forward")
    m.modules.eval()
    batch = _batch(lens=[1.0, 0.75, 0.2])  # 5 frames for 6 states
    m.on_stage_start(Stage.VALID, 1)
    with torch.no_grad():
        m.compute_objectives(m.compute_forward(batch, Stage.VALID), batch, Stage.VALID)  # no raise per batch
    with pytest.raises(AssertionError, match="fewer frames"):
        m.on_stage_end(Stage.VALID, 0.0, 1)


def test_train_and_test_scripts(tmp_path):
    need_gpu()
    overrides = ("{synthetic: {md_labels: true, ali_labels: true, n_train: 16, n_valid: 8, n_test: 8, "
                 "min_frames: 40, max_frames: 60}, model: {n_epochs: 2, dnn_neurons: 32}}")
    common = ["config/run.yaml", "--model_class", "HMM_DNN_ALI", "--model_name", "hmm_dnn_ali_ci",
              "--model", "!include:../models/HMM_DNN_ALI/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    lines = [l for l in log.splitlines() if "accuracy.average" in l]
    assert len(lines) == 4, log[-2000:]  # TRAIN and VALID of both epochs
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1
    assert any("accuracy.average" in open(os.path.join(c, "CKPT.yaml")).read() for c in ckpts)
    assert os.path.exists(os.path.join(ckpts[0], "model.ckpt")) and os.path.exists(os.path.join(ckpts[0], "output.ckpt"))
    r = _script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "accuracy.average" in open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    starts = json.load(open(tmp_path / "out" / "test_output" / "alignments.json"))
    from utils.data_io import SyntheticSet
    test_set = SyntheticSet(8, 120, 40, 60, 123456 + 2, md_labels=True, n_phonemes=39)
    assert sorted(starts) == sorted(e["id"] for e in test_set.items)
    for e in test_set.items:
        s = starts[e["id"]]
        assert len(s) == len(e["gt_cnncl_seq"]) and s[0] == 0
        assert all(a < b for a, b in zip(s, s[1:])) and s[-1] < e["feat"].shape[0]
