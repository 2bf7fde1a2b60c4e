"""Golden fixtures for the upstream-module recipes (ml-vae_amd/models/test_phn_classifier and
test_b_ind_classifier): ``test_phn_classifier_tiny.npz``, ``test_b_ind_classifier_tiny.npz`` and
the key names of the two reference yamls (``*_yaml_keys.json``).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs
it.  It reuses the import shims of ``make_golden_md_recipe.py`` and runs the reference's own
``SBModel.compute_forward`` + ``compute_objectives`` of each recipe on a stand-in ``self`` built
from the reference's module and its real stats class; only data is written.

One batch per recipe: B = 3, T = 24, F = 8, frame lengths 1.0 / 0.75 / 0.5, H = 16, 2 layers,
n_phonemes = 5, 4 / 3 / 2 phonemes.  One TRAIN pass (train mode, with backward) and one TEST pass
(eval mode).  The normaliser is the identity.  The boundary detector's ten uniform draws are
recorded and replayed.  The boundary recipe's compute_objectives returns the sum of the module's
unreduced [B, T] losses (backward on it raises): the unreduced per-key losses are recorded, and
the loss whose gradients are recorded is sum_k weight_k * apply_lens_to_loss(loss_k, feat_lens)
with the reference's own apply_lens_to_loss and the weights the stand-in's hparams carry.

A seed is accepted only if every valid frame's and every segment sum's top-2 logit gap is >= 1e-3
of the largest magnitude (phoneme recipe), the k-th and (k+1)-th largest boundary_v of every
utterance differ by >= 1e-3 relative (boundary recipe), and at least one utterance scores
strictly between 0 and 100 at each level.

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_upstream.py
"""
import importlib
import json
import os
import re
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402,F401
import make_golden_md_recipe as R  # noqa: E402  (generator-only shims, reference src on sys.path)
import speechbrain as sb  # noqa: E402  (the stand-in)
from modules.boundary_detector import BoundaryDetector  # noqa: E402  (reference)
from modules.phoneme_recognizer import PhonemeRecognizer  # noqa: E402  (reference)
from utils.data_utils import apply_lens_to_loss  # noqa: E402  (reference)
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats  # noqa: E402  (reference)
from utils.metric_stats.phn_acc_metric_stats import PhnAccMetricStats  # noqa: E402  (reference)

PhnModel = importlib.import_module("models.test_phn_classifier.model").SBModel  # (reference)
BndModel = importlib.import_module("models.test_b_ind_classifier.model").SBModel  # (reference)

B, T, F, H, L, NPH = 3, 24, 8, 16, 4, 5
REL_T = [1.0, 0.75, 0.5]
REL_L = [1.0, 0.75, 0.5]
BND_WEIGHTS = dict(boundary_kld_weight=0.01)  # the bce weight is absent: 1
GAP = 1e-3


def _batch(g):
    rel_t, rel_l = torch.tensor(REL_T), torch.tensor(REL_L)
    Ti = [int(torch.round(r * T)) for r in rel_t]
    Li = [int(torch.round(r * L)) for r in rel_l]
    fa, gt = torch.zeros(B, T), torch.zeros(B, T)
    for b in range(B):
        for dst in (fa, gt):
            cuts = torch.randperm(Ti[b] - 1, generator=g)[:Li[b] - 1] + 1
            dst[b, 0] = 1.0
            dst[b, cuts] = 1.0
    seqs = torch.randint(0, NPH, (B, L), generator=g)
    flvl = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        seqs[b, Li[b]:] = 0
        seg = torch.cumsum(gt[b, :Ti[b]], 0).long() - 1
        flvl[b, :Ti[b]] = seqs[b][seg]
    return R._Batch({
        "id": [f"utt{b}" for b in range(B)],
        "feat": (torch.randn(B, T, F, generator=g), rel_t),
        "gt_cnncl_seq": (seqs, rel_l),
        "flvl_gt_cnncl_seq": (flvl, rel_t),
        "fa_boundary_seq": (fa, rel_t),
        "gt_boundary_seq": (gt, rel_t),
    }), Ti, Li


def _model(cls, modules, stats_key, stats, **hp):
    m = cls.__new__(cls)
    m.modules = modules
    m.device = "cpu"
    m.stats_loggers = {stats_key: stats}
    m.hparams = types.SimpleNamespace(epoch_counter=types.SimpleNamespace(current=1),
                                      normalizer=lambda feats, lens, epoch=None: feats, **hp)
    return m


def _record_batch(batch):
    return {"feat": batch["feat"][0].numpy(), "feat_lens": batch["feat"][1].numpy(),
            "gt_cnncl_seq": batch["gt_cnncl_seq"][0].numpy(), "seq_lens": batch["gt_cnncl_seq"][1].numpy(),
            "flvl_gt_cnncl_seq": batch["flvl_gt_cnncl_seq"][0].numpy(),
            "fa_boundary_seq": batch["fa_boundary_seq"][0].numpy(),
            "gt_boundary_seq": batch["gt_boundary_seq"][0].numpy()}


def _gap_ok(x):
    top = torch.topk(x, 2, dim=-1).values
    return bool(((top[:, 0] - top[:, 1]) >= GAP * x.abs().max()).all())


def _between(scores, key):
    return any(0 < s[key] < 100 for s in scores)


def _scores_json(stats):
    return np.array(json.dumps([{k: float(v) for k, v in s.items()} for s in stats.scores_list]))


def run_phn(seed):
    torch.manual_seed(seed)
    modules = torch.nn.ModuleDict({"phoneme_recognizer": PhonemeRecognizer(
        input_size=F, rnn_hidden_size=H, rnn_num_layers=2, fc_sizes=[H, H, H, NPH + 2], n_phonemes=NPH)})
    with torch.no_grad():  # a fresh head gives near-equal logits: widen it, as make_golden_md_recipe
        modules["phoneme_recognizer"].fc.blocks[-1].weight *= 40.0
    g = torch.Generator().manual_seed(seed + 1)
    batch, Ti, Li = _batch(g)
    rec = _record_batch(batch)
    for n, p in modules.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()
    for name, stage, train in (("TRAIN", sb.Stage.TRAIN, True), ("TEST", sb.Stage.TEST, False)):
        modules.train(train)
        stats = PhnAccMetricStats()
        m = _model(PhnModel, modules, "phn_acc_stats", stats)
        with torch.set_grad_enabled(train):
            pred = m.compute_forward(batch, stage)
            loss = m.compute_objectives(pred, batch, stage)
        out = pred["out"].detach()
        for b in range(B):
            x = out[b, :Ti[b]]
            starts = torch.where(batch["gt_boundary_seq"][0][b, :Ti[b]] == 1)[0].tolist() + [Ti[b]]
            sums = torch.stack([x[a:c].sum(0) for a, c in zip(starts[:-1], starts[1:])])
            if not (_gap_ok(x) and _gap_ok(sums)):
                return None
        if not (_between(stats.scores_list, "flvl_acc") and _between(stats.scores_list, "plvl_acc")):
            return None
        rec[f"{name}/out"] = out.numpy()
        rec[f"{name}/loss"] = loss.detach().numpy()
        rec[f"{name}/loss_e"] = pred["losses"]["phn_recog_bce_loss"].detach().numpy()
        rec[f"{name}/summary_json"] = np.array(json.dumps(stats.summarize()))
        rec[f"{name}/scores_json"] = _scores_json(stats)
        if train:
            loss.backward()
            for n, p in modules.named_parameters():
                rec[f"TRAIN/grad/{n}"] = p.grad.numpy().copy()
                p.grad = None
    rec["meta_json"] = np.array(json.dumps(dict(
        B=B, T=T, F=F, H=H, L=L, n_phonemes=NPH, seed=seed, lengths=Ti, phn_lengths=Li,
        param_names=[n for n, _ in modules.named_parameters()])))
    return rec


def run_bnd(seed):
    torch.manual_seed(seed)
    modules = torch.nn.ModuleDict({"boundary_detector": BoundaryDetector(
        input_size=F, rnn_hidden_size=H, rnn_num_layers=2, fc_sizes=[H, H, H, 1])})
    g = torch.Generator().manual_seed(seed + 1)
    batch, Ti, Li = _batch(g)
    us = [torch.rand(B, T, generator=g) for _ in range(10)]
    rec = _record_batch(batch)
    rec["boundary_u"] = torch.stack(us).numpy()
    for n, p in modules.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()
    for name, stage, train in (("TRAIN", sb.Stage.TRAIN, True), ("TEST", sb.Stage.TEST, False)):
        modules.train(train)
        stats = BoundaryMetricStats()
        m = _model(BndModel, modules, "boundary_stats", stats, **BND_WEIGHTS)
        seen = {}
        orig = stats.append

        def capture(ids, _orig=orig, _seen=seen, **kw):
            _seen.update(kw)
            return _orig(ids, **kw)

        stats.append = capture
        with R._Inject(us, [], [], None), torch.set_grad_enabled(train):
            pred = m.compute_forward(batch, stage)
            ref_total = m.compute_objectives(pred, batch, stage)  # the unreduced [B, T] sum
        v = pred["boundary_v"].detach()
        for b in range(B):
            srt = torch.sort(v[b, :Ti[b]], descending=True).values
            k = Li[b]
            if k < Ti[b] and not (srt[k - 1] - srt[k]) >= GAP * srt[k - 1].abs():
                return None
        if not (_between(stats.scores_list, "pre") and _between(stats.scores_list, "f1")):
            return None
        losses = pred["losses"]
        assert list(losses) == ["boundary_bce_loss", "boundary_kld_loss"]
        loss = 0
        for key in losses:
            weight = BND_WEIGHTS.get(key.replace("_loss", "_weight"), 1)
            loss = loss + weight * apply_lens_to_loss(losses[key], batch["feat"][1])
        rec[f"{name}/boundary_v"] = v.numpy()
        rec[f"{name}/ref_unreduced_total"] = ref_total.detach().numpy()
        for key in losses:
            rec[f"{name}/loss/{key}"] = losses[key].detach().numpy()
        rec[f"{name}/loss"] = loss.detach().numpy()
        rec[f"{name}/pred_boundary_seqs"] = R._pad([p.tolist() for p in seen["predictions"]], T)
        rec[f"{name}/summary_json"] = np.array(json.dumps(stats.summarize()))
        rec[f"{name}/scores_json"] = _scores_json(stats)
        if train:
            loss.backward()
            for n, p in modules.named_parameters():
                rec[f"TRAIN/grad/{n}"] = p.grad.numpy().copy()
                p.grad = None
    rec["meta_json"] = np.array(json.dumps(dict(
        B=B, T=T, F=F, H=H, L=L, n_phonemes=NPH, seed=seed, lengths=Ti, phn_lengths=Li,
        weights=BND_WEIGHTS, param_names=[n for n, _ in modules.named_parameters()])))
    return rec


def yaml_keys(recipe):
    """Key names of a reference model.yaml: top level, ``modules:`` and ``recoverables:``."""
    text = open(os.path.join(make_golden.REF_SRC, "models", recipe, "model.yaml")).read()
    text = re.sub(r"^\s*#.*\n", "", text, flags=re.M)
    top = re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", text, flags=re.M)

    def block(name, indent):
        body = re.search(rf"^{indent}{name}:\n((?:{indent}    \S.*\n?)+)", text, flags=re.M).group(1)
        return re.findall(r"^\s+([A-Za-z_][A-Za-z0-9_]*):", body, flags=re.M)

    return {"top_level": top, "modules": block("modules", ""), "recoverables": block("recoverables", "    ")}


if __name__ == "__main__":
    torch.set_num_threads(1)
    for recipe, fn in (("test_phn_classifier", run_phn), ("test_b_ind_classifier", run_bnd)):
        for seed in range(71, 271):
            rec = fn(seed)
            if rec is not None:
                break
        else:
            raise SystemExit(f"{recipe}: no seed accepted")
        path = os.path.join(R.OUT_DIR, f"{recipe}_tiny.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes, seed", seed)
        with open(os.path.join(R.OUT_DIR, f"{recipe}_yaml_keys.json"), "w") as f:
            json.dump(yaml_keys(recipe), f, indent=1)
