"""Golden fixture for the LSTM_FC recipe (ml-vae_amd/models/LSTM_FC/model.py).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs it.  It imports
``make_golden_md_recipe`` for the import shims (the ``speechbrain`` stand-ins, ``undo_padding``)
and runs the reference's own ``models.LSTM_FC.model.SBModel.compute_forward`` +
``compute_objectives`` (ref:src/models/LSTM_FC/model.py:22-69) on a stand-in ``self``; only data
is written: ``lstm_fc_tiny.npz`` and ``lstm_fc_yaml_keys.json`` (the key names of the reference's
model.yaml).

Two more stand-ins, inside this script only:
* ``speechbrain.nnet.losses.compute_masked_loss``, written to SpeechBrain's formula on the existing
  ``_length_to_mask``: mask = ones_like(targets) * length_to_mask(length * T, max_len=T) broadcast
  over the trailing axes; loss = sum(loss_fn(predictions, targets) * mask) / sum(mask).
* a stats logger whose ``append`` records its keyword arguments.  The reference passes
  ``batch_pred_md_lbl_seqs`` / ``batch_gt_md_lbl_seqs``, which its ``batch_seq_md_scoring`` does
  not take (the real MDMetricStats raises); the recorder survives that and yields the predicted
  and true sequences, cut to length by the reference itself.

B=3, T=24, F=8, lengths 1.0 / 0.75 / 0.5, LSTM H=16, L=2, dropout 0, fc [16, 8, 8, 2],
misp_weight 10; one TRAIN pass (train mode, with backward) and one TEST pass (eval mode).  The
batch carries the same tensors under the plain and the aug_ names.  A fresh net gives
near-constant logits: fc's output layer is widened by OUT_SCALE and its bias re-centred on the
valid frames' mean logit gap.  A seed is accepted only if both labels occur among the valid
frames, both predicted classes occur, and every valid frame has |x1 - x0| >= 1e-3 (fp32
differences cannot flip an argmax).

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_lstm_fc.py
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_md_recipe as R  # noqa: E402  (shims; reference src on sys.path)


def _compute_masked_loss(loss_fn, predictions, targets, length=None, label_smoothing=0.0,
                         reduction="mean"):
    assert label_smoothing == 0.0 and reduction == "mean"
    mask = torch.ones_like(targets)
    if length is not None:
        length_mask = R.make_golden._length_to_mask(length * targets.shape[1], max_len=targets.shape[1])
        while len(length_mask.shape) < len(mask.shape):
            length_mask = length_mask.unsqueeze(-1)
        mask = mask * length_mask.type(mask.dtype)
    loss = loss_fn(predictions, targets) * mask
    return loss.sum() / torch.sum(mask)


sys.modules["speechbrain.nnet.losses"].compute_masked_loss = _compute_masked_loss

import speechbrain as sb  # noqa: E402  (the stand-in)
from models.LSTM_FC.model import SBModel  # noqa: E402  (reference)
from modules.fc_block import FCBlock  # noqa: E402  (reference)

B, T, F, H, L = 3, 24, 8, 16, 2
FC = [H, 8, 8, 2]
MISP_WEIGHT = 10
OUT_SCALE = 600.0
MIN_GAP = 1e-3
MODEL_NAME = "lstm_fc_tiny"


class _Recorder:
    def __init__(self):
        self.calls = []

    def append(self, ids, **kwargs):
        self.calls.append((list(ids), kwargs))


def _batch(g):
    rel = torch.tensor([1.0, 0.75, 0.5])
    Ti = [int(torch.round(r * T)) for r in rel]
    feat = torch.randn(B, T, F, generator=g)
    lbl = (torch.rand(B, T, generator=g) < 0.3).to(torch.int64)
    for b in range(B):
        feat[b, Ti[b]:] = 0.0
        lbl[b, Ti[b]:] = 0
    return R._Batch({"id": [f"utt{b}" for b in range(B)], "feat": (feat, rel), "aug_feat": (feat, rel),
                     "flvl_gt_md_lbl_seq": (lbl, rel), "aug_flvl_gt_md_lbl_seq": (lbl, rel)}), Ti


def _pad(seqs):
    return R._pad(seqs, T)


def run(seed):
    torch.manual_seed(seed)
    modules = torch.nn.ModuleDict({
        "lstm": torch.nn.LSTM(batch_first=True, input_size=F, hidden_size=H, num_layers=L, dropout=0.0),
        "fc": FCBlock(fc_sizes=FC, dropout=0),
    })
    g = torch.Generator().manual_seed(seed + 1)
    batch, Ti = _batch(g)
    valid = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        valid[b, :Ti[b]] = True
    m = SBModel.__new__(SBModel)
    m.modules = modules
    m.device = "cpu"
    m.hparams = types.SimpleNamespace(misp_weight=MISP_WEIGHT)

    with torch.no_grad():  # widen the output layer, centre the logit gap on the valid frames
        modules["fc"].blocks[-1].weight *= OUT_SCALE
        out = m.compute_forward(batch, sb.Stage.TEST)["out"]
        modules["fc"].blocks[-1].bias[1] -= (out[..., 1] - out[..., 0])[valid].mean()

    lbl = batch["flvl_gt_md_lbl_seq"][0]
    if len(torch.unique(lbl[valid])) != 2:
        return "one label only among the valid frames"
    rec = {"feat": batch["feat"][0].numpy(), "feat_lens": batch["feat"][1].numpy(),
           "flvl_gt_md_lbl_seq": lbl.numpy()}
    for n, p in modules.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()

    for name, stage, train in (("TRAIN", sb.Stage.TRAIN, True), ("TEST", sb.Stage.TEST, False)):
        modules.train(train)
        for p in modules.parameters():
            p.grad = None
        stats = _Recorder()
        m.stats_loggers = {"flvl_md_stats": stats}
        if train:
            pred = m.compute_forward(batch, stage)
            loss = m.compute_objectives(pred, batch, stage)
            loss.backward()
        else:
            with torch.no_grad():
                pred = m.compute_forward(batch, stage)
                loss = m.compute_objectives(pred, batch, stage)
        out = pred["out"].detach()
        gap = (out[..., 1] - out[..., 0])[valid]
        if gap.abs().min().item() < MIN_GAP:
            return f"a valid frame's logit gap is {gap.abs().min().item():.2e}"
        if len(torch.unique(out.argmax(-1)[valid])) != 2:
            return "one predicted class only"
        (ids, kw), = stats.calls
        assert ids == batch["id"] and set(kw) == {"batch_pred_md_lbl_seqs", "batch_gt_md_lbl_seqs"}
        assert [len(s) for s in kw["batch_pred_md_lbl_seqs"]] == Ti == [len(s) for s in kw["batch_gt_md_lbl_seqs"]]
        rec[f"{name}/out"] = out.numpy()
        rec[f"{name}/loss"] = loss.detach().numpy()
        rec[f"{name}/pred_md_lbl_seqs"] = _pad(kw["batch_pred_md_lbl_seqs"])
        rec[f"{name}/gt_md_lbl_seqs"] = _pad(kw["batch_gt_md_lbl_seqs"])
        if train:
            for n, p in modules.named_parameters():
                rec[f"{name}/grad/{n}"] = p.grad.numpy().copy()
    meta = dict(B=B, T=T, F=F, H=H, L=L, fc_sizes=FC, misp_weight=MISP_WEIGHT, seed=seed,
                out_scale=OUT_SCALE, min_gap=float(gap.abs().min()), max_gap=float(gap.abs().max()),
                lengths=Ti, param_names=[n for n, _ in modules.named_parameters()])
    rec["meta_json"] = np.array(json.dumps(meta))
    return rec


def yaml_keys():
    R.REF_YAML = os.path.join(R.make_golden.REF_SRC, "models", "LSTM_FC", "model.yaml")
    return R.yaml_keys()


if __name__ == "__main__":
    torch.set_num_threads(1)
    for seed in range(131, 171):
        rec = run(seed)
        if not isinstance(rec, str):
            break
        print("seed", seed, "refused:", rec)
    else:
        raise SystemExit("no seed accepted")
    path = os.path.join(R.OUT_DIR, MODEL_NAME + ".npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes, seed", seed)
    print(str(rec["meta_json"])[:400])
    with open(os.path.join(R.OUT_DIR, "lstm_fc_yaml_keys.json"), "w") as f:
        json.dump(yaml_keys(), f, indent=1)
