"""Golden fixture for the w2v_LSTM_FC recipe (ml-vae_amd/models/w2v_LSTM_FC/model.py).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs it.  It imports
``make_golden_lstm_fc`` for the import shims (the ``speechbrain`` stand-ins, ``undo_padding`` and
the ``compute_masked_loss`` stand-in written to SpeechBrain's formula) and runs the reference's own
``models.w2v_LSTM_FC.model.SBModel.compute_forward`` + ``compute_objectives``
(ref:src/models/w2v_LSTM_FC/model.py:22-78) on a stand-in ``self``; only data is written:
``w2v_lstm_fc_tiny.npz`` and ``w2v_lstm_fc_yaml_keys.json`` (the key names of the reference's
model.yaml).

The wav2vec2 module is replaced by a stub that returns a recorded feature tensor [B, T_w, C]
(requiring grad, so the gradient at the encoder's output is recorded too); the classifier is the
reference's FCBlock [C, 1].  B = 3, C = 8, label frames T = 24, lengths 1.0 / 0.75 / 0.5.  Two cases:
``short`` -- T_w = 23, the encoder one frame short of the labels, which the reference cuts to the
common length (TRAIN with backward, and TEST) -- and ``equal`` -- T_w = 24 (TEST).  The stats logger
records the keyword arguments of ``append``.  A fresh classifier gives small logits: its weight is
widened by OUT_SCALE.  A seed is
accepted only if both labels and both predictions occur among the scored frames and every scored
frame has |logit| >= 1e-3 (fp32 differences cannot flip a rounded sigmoid).

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_w2v_lstm_fc.py
"""
import json
import os
import re
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_lstm_fc as LF  # noqa: E402  (shims, compute_masked_loss stand-in; reference src on sys.path)

R = LF.R
import speechbrain as sb  # noqa: E402  (the stand-in)
from models.w2v_LSTM_FC.model import SBModel  # noqa: E402  (reference)
from modules.fc_block import FCBlock  # noqa: E402  (reference)

B, T, C = 3, 24, 8
OUT_SCALE = 40.0
MIN_GAP = 1e-3
MODEL_NAME = "w2v_lstm_fc_tiny"
REF_YAML = os.path.join(R.make_golden.REF_SRC, "models", "w2v_LSTM_FC", "model.yaml")


class _Encoder(torch.nn.Module):
    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def forward(self, wavs):
        return self.feats


def _batch(g):
    rel = torch.tensor([1.0, 0.75, 0.5])
    lbl = (torch.rand(B, T, generator=g) < 0.3).to(torch.int64)
    for b in range(B):
        lbl[b, int(torch.round(rel[b] * T)):] = 0
    wav = torch.zeros(B, 320 * T)
    return R._Batch({"id": [f"utt{b}" for b in range(B)], "wav": (wav, rel), "feat": (torch.zeros(B, T, 1), rel),
                     "flvl_gt_md_lbl_seq": (lbl, rel)})


def run(seed):
    torch.manual_seed(seed)
    clf = FCBlock(fc_sizes=[C, 1])
    g = torch.Generator().manual_seed(seed + 1)
    batch = _batch(g)
    rel = batch["feat"][1]
    feats = {"short": torch.randn(B, T - 1, C, generator=g), "equal": torch.randn(B, T, C, generator=g)}
    with torch.no_grad():
        clf.blocks[-1].weight *= OUT_SCALE
    rec = {"feat_lens": rel.numpy(), "flvl_gt_md_lbl_seq": batch["flvl_gt_md_lbl_seq"][0].numpy()}
    for n, p in clf.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()
    lens = {}
    for case, stage_name, stage, train in (("short", "TRAIN", sb.Stage.TRAIN, True),
                                           ("short", "TEST", sb.Stage.TEST, False),
                                           ("equal", "TEST", sb.Stage.TEST, False)):
        x = feats[case].clone().requires_grad_(train)
        m = SBModel.__new__(SBModel)
        m.modules = torch.nn.ModuleDict({"wav2vec2": _Encoder(x), "classifier": clf})
        m.device = "cpu"
        m.hparams = types.SimpleNamespace()
        stats = LF._Recorder()
        m.stats_loggers = {"flvl_md_stats": stats}
        clf.train(train)
        for p in clf.parameters():
            p.grad = None
        with torch.set_grad_enabled(train):
            pred = m.compute_forward(batch, stage)
            loss = m.compute_objectives(pred, batch, stage)
        if train:
            loss.backward()
        logits = pred["logits"].detach()
        n = min(logits.shape[1], T)
        Ti = [int(torch.round(r * n)) for r in rel]
        scored = torch.zeros(B, logits.shape[1], dtype=torch.bool)
        for b in range(B):
            scored[b, :Ti[b]] = True
        if logits[scored].abs().min().item() < MIN_GAP:
            return f"a scored frame's |logit| is {logits[scored].abs().min().item():.2e}"
        (ids, kw), = stats.calls
        assert ids == batch["id"] and set(kw) == {"pred_md_lbl_seqs", "gt_md_lbl_seqs"}
        assert [len(s) for s in kw["pred_md_lbl_seqs"]] == Ti == [len(s) for s in kw["gt_md_lbl_seqs"]]
        if len({v for s in kw["pred_md_lbl_seqs"] for v in s}) != 2 or len({v for s in kw["gt_md_lbl_seqs"] for v in s}) != 2:
            return "one label or one predicted class only"
        k = f"{case}/{stage_name}"
        rec[f"{case}/feats"] = feats[case].numpy()
        rec[k + "/logits"] = logits.numpy()
        rec[k + "/loss"] = loss.detach().numpy()
        rec[k + "/pred_md_lbl_seqs"] = R._pad([[int(v) for v in s] for s in kw["pred_md_lbl_seqs"]], T)
        rec[k + "/gt_md_lbl_seqs"] = R._pad(kw["gt_md_lbl_seqs"], T)
        lens[case] = Ti
        if train:
            rec[k + "/dfeats"] = x.grad.numpy().copy()
            for pn, p in clf.named_parameters():
                rec[f"{k}/grad/{pn}"] = p.grad.numpy().copy()
    meta = dict(B=B, T=T, C=C, seed=seed, out_scale=OUT_SCALE, lengths=lens,
                param_names=[n for n, _ in clf.named_parameters()])
    rec["meta_json"] = np.array(json.dumps(meta))
    return rec


def yaml_keys():
    """Key names of the reference's model.yaml: top level, ``modules:``, ``recoverables:`` and the
    optimizer groups."""
    text = open(REF_YAML).read()
    top = re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", text, flags=re.M)

    def block(name, indent=" *"):
        m = re.search(rf"^({indent}){name}:\n((?:\1 +\S.*\n?)+)", text, flags=re.M)
        lines = m.group(2).splitlines()
        ind = min(len(l) - len(l.lstrip()) for l in lines)
        return [l.strip().split(":")[0] for l in lines if len(l) - len(l.lstrip()) == ind and not l.strip().startswith("#")]

    return {"top_level": top, "modules": block("modules", ""), "recoverables": block("recoverables"),
            "optimizers": block("optimizers")}


if __name__ == "__main__":
    torch.set_num_threads(1)
    for seed in range(211, 251):
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
    with open(os.path.join(R.OUT_DIR, "w2v_lstm_fc_yaml_keys.json"), "w") as f:
        json.dump(yaml_keys(), f, indent=1)
    print(yaml_keys())
