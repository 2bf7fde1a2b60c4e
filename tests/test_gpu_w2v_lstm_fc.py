"""The w2v_LSTM_FC recipe (models/w2v_LSTM_FC) on the HIP path.

* compute_forward + compute_objectives against the reference's own numbers
  (tests/golden/w2v_lstm_fc_tiny.npz, make_golden_w2v_lstm_fc.py), the recorded features fed through
  a stub encoder: the loss at 1e-5 and the logits at 1e-5 relative-max, the classifier's gradients
  and the gradient at the encoder's output at 1e-4 (the LSTM_FC recipe's bounds for the same
  quantities), the scored sequences equal to the recorded ones;
* 30 fit_batch steps on one fixed batch of the spoken corpus with the tiny trainable encoder: both
  optimizer groups step (the encoder's trainable tensors move, its conv stack keeps its bits) and
  the loss ends below step 0's;
* train.py then test.py end to end with the small-encoder override, 2 epochs: both stages print
  flvl_md.F1, the checkpoint holds wav2vec2 and classifier and restores.
Reference ops: ref:src/models/w2v_LSTM_FC/model.py:16-78."""
import glob
import json
import os
import types

import numpy as np
import pytest
import torch

import w2v_ref as R
from conftest import PKG
from gpu_utils import need_gpu, rel_err
from test_gpu_md_vae import _script

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w2v_lstm_fc_tiny.npz")
KEYS = ["flvl_md.ACC", "flvl_md.PRE", "flvl_md.REC", "flvl_md.F1"]
SMALL = ("wav2vec2_size: 128, wav2vec2_config: {conv_dim: [32, 32, 32, 32, 32, 32, 32], num_hidden_layers: 2, "
         "num_attention_heads: 2, intermediate_size: 256, num_conv_pos_embeddings: 16, "
         "num_conv_pos_embedding_groups: 4}")


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLD)
    return {k: d[k] for k in d.files}


class _Stub(torch.nn.Module):
    """The encoder replaced by the recorded features (a leaf, so its gradient can be read)."""

    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, wavs):
        return self.feats


def _model(modules, tmp_path, **hp):
    from models.w2v_LSTM_FC.model import SBModel
    hparams = dict(epoch_counter=types.SimpleNamespace(current=1), metric_keys=KEYS, output_dir=str(tmp_path), **hp)
    return SBModel(modules=modules, hparams=hparams, run_opts={"device": "cuda:0"})


def _gold_batch(gold, meta):
    from brain.dataio import PaddedBatch
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    rel = torch.from_numpy(gold["feat_lens"])
    b.update({"id": [f"utt{i}" for i in range(meta["B"])], "wav": (torch.zeros(meta["B"], 320 * meta["T"]), rel),
              "feat": (torch.zeros(meta["B"], meta["T"], 1), rel),
              "flvl_gt_md_lbl_seq": (torch.from_numpy(gold["flvl_gt_md_lbl_seq"]), rel)})
    return b


def _seqs(padded):
    return [[v for v in row if v >= 0] for row in padded.tolist()]


@pytest.mark.parametrize("case,name", [("short", "TRAIN"), ("short", "TEST"), ("equal", "TEST")])
def test_matches_reference(gold, tmp_path, case, name):
    need_gpu()
    from brain import Stage
    from modules.fc_block import FCBlock
    meta = json.loads(str(gold["meta_json"]))
    train = name == "TRAIN"
    feats = torch.from_numpy(gold[case + "/feats"]).cuda().requires_grad_(train)
    clf = FCBlock([meta["C"], 1])
    clf.load_state_dict({n: torch.from_numpy(gold["param/" + n]) for n in meta["param_names"]})
    m = _model({"wav2vec2": _Stub(feats), "classifier": clf}, tmp_path)
    stage = Stage.TRAIN if train else Stage.TEST
    m.modules.train(train)
    m.on_stage_start(stage, 1)
    k = f"{case}/{name}"
    batch = _gold_batch(gold, meta)  # compute_forward moves it to the device in place, as the Brain's loop relies on
    with torch.set_grad_enabled(train):
        pred = m.compute_forward(batch, stage)
        loss = m.compute_objectives(pred, batch, stage)
    e_out, e_loss = rel_err(pred["logits"], torch.from_numpy(gold[k + "/logits"])), rel_err(loss, torch.from_numpy(gold[k + "/loss"]))
    print(f"{k}: logits rel {e_out:.2e}, loss {float(loss.detach()):.7f} ref {float(gold[k + '/loss']):.7f} rel {e_loss:.2e}")
    assert pred["logits"].shape == gold[k + "/logits"].shape
    assert e_out < 1e-5 and e_loss < 1e-5
    seqs = m.stats_loggers["flvl_md_stats"].saved_seqs
    assert seqs["pred_md_lbl_seqs"] == _seqs(gold[k + "/pred_md_lbl_seqs"])
    assert seqs["gt_md_lbl_seqs"] == _seqs(gold[k + "/gt_md_lbl_seqs"])
    assert [len(s) for s in seqs["gt_md_lbl_seqs"]] == meta["lengths"][case]
    if train:
        loss.backward()
        for n, p in clf.named_parameters():
            e = rel_err(p.grad, torch.from_numpy(gold[f"{k}/grad/{n}"]))
            print(f"{k} grad {n} rel {e:.2e}")
            assert e < 1e-4, (n, e)
        e = rel_err(feats.grad, torch.from_numpy(gold[k + "/dfeats"]))
        print(f"{k} gradient at the encoder's output rel {e:.2e}")
        assert e < 1e-4


def test_thirty_steps_on_one_batch_lower_the_loss(tmp_path):
    need_gpu()
    import functools
    from brain.features import Fbank
    from modules.fc_block import FCBlock
    from modules.wav2vec2 import Wav2Vec2
    from utils.data_io import SyntheticSet
    cf = Fbank(deltas=True, sample_rate=16000, hop_length=20, n_fft=400, n_mels=40)
    ds = SyntheticSet(4, 120, 40, 60, 4242, md_labels=True, n_phonemes=7, waveforms=True, compute_features=cf)
    batch = next(iter(ds.batches(batch_size=4)))
    torch.manual_seed(3)
    enc = Wav2Vec2(config=R.TINY, precision="bf16", freeze=False, freeze_feature_extractor=True)
    enc.load_state_dict(R.fill_state(R.TINY, 20))
    mods = {"wav2vec2": enc, "classifier": FCBlock([128, 1])}
    opts = {"adam_opt": {"opt_class": functools.partial(torch.optim.Adam, lr=3e-4), "modules": ["classifier"]},
            "wav2vec_opt": {"opt_class": functools.partial(torch.optim.Adam, lr=1e-4), "modules": ["wav2vec2"]}}
    m = _model(mods, tmp_path, optimizers=opts, batch_size=4)
    m.init_optimizers()
    from mlvae_hip import optim as hip_optim
    assert set(m.optimizers) == {"adam_opt", "wav2vec_opt"}
    assert all(isinstance(o, hip_optim.Adam) for o in m.optimizers.values())  # torch.optim.Adam maps to the HIP one
    assert len(m.optimizers["wav2vec_opt"].param_groups[0]["params"]) == 41
    before = {k: v.clone() for k, v in m.modules["wav2vec2"].state_dict().items()}
    m.modules.train()
    m.on_stage_start(__import__("brain").Stage.TRAIN, 1)
    losses = [float(m.fit_batch(batch)) for _ in range(30)]
    print("fit_batch losses:", " ".join(f"{x:.4f}" for x in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    after = m.modules["wav2vec2"].state_dict()
    for k in after:
        same = torch.equal(after[k], before[k])
        assert same == (not Wav2Vec2.trainable_key(k)), k


def test_train_and_test_scripts(tmp_path):
    need_gpu()
    overrides = ("{synthetic: {md_labels: true, waveforms: true, n_train: 8, n_valid: 4, n_test: 4, min_frames: 40, "
                 "max_frames: 60}, model: {n_epochs: 2, " + SMALL + "}}")
    common = ["config/run.yaml", "--model_class", "w2v_LSTM_FC", "--model_name", "w2v_lstm_fc_ci",
              "--model", "!include:../models/w2v_LSTM_FC/model.yaml", "--output_dir", str(tmp_path / "out"),
              "--extra_overrides", overrides]
    r = _script(["train.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(tmp_path / "out" / "train_log.txt").read()
    lines = [l for l in log.splitlines() if "flvl_md.F1" in l]
    assert len(lines) == 4, log[-2000:]  # TRAIN and VALID both score, two epochs
    assert lines[0].startswith("stage: train, epoch: 1") and lines[3].startswith("stage: valid, epoch: 2")
    ckpts = glob.glob(str(tmp_path / "out" / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1
    from modules.fc_block import FCBlock
    from modules.wav2vec2 import Wav2Vec2
    enc = Wav2Vec2(config=R.TINY, freeze=False, freeze_feature_extractor=True)
    enc.load_state_dict(torch.load(os.path.join(ckpts[0], "wav2vec2.ckpt"), weights_only=True))  # strict
    clf = FCBlock([128, 1])
    clf.load_state_dict(torch.load(os.path.join(ckpts[0], "classifier.ckpt"), weights_only=True))
    assert all(bool(torch.isfinite(p).all()) for mod in (enc, clf) for p in mod.parameters())
    assert os.path.exists(os.path.join(ckpts[0], "counter.ckpt"))
    r = _script(["test.py"] + common, PKG)
    assert r.returncode == 0, r.stderr[-3000:]
    metrics = open(tmp_path / "out" / "test_output" / "test_metrics.txt").read()
    for key in KEYS:
        assert key in metrics, (key, metrics)
