"""Golden fixture for the MD-VAE recipe (ml-vae_amd/models/MD_VAE/model.py).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs it.  It reuses the
import shims of ``make_golden.py`` (plus one more generator-only stand-in,
``speechbrain.utils.data_utils.undo_padding``) and runs the reference's own
``models.MD_VAE.model.SBModel.compute_forward`` + ``compute_objectives`` (ref:src/models/MD_VAE/
model.py:61-223) on a stand-in ``self`` built from the reference's modules; only data is written:
``md_vae_tiny.npz`` and ``md_vae_yaml_keys.json`` (the key names of the reference's model.yaml).

One set of parameters and one batch (B=3, T=24, F=8, every hidden size 16, L=6, n_phonemes=5, both
dropouts 0; frame lengths 1.0 / 0.75 / 0.5, phoneme lengths 1.0 / 5/6 / 0.5), run under the targets
PHN_RECOG, B_DETECTOR and VAE in train mode (Stage.TRAIN) and TEST in eval mode (Stage.TEST).  The
normaliser is the identity (SpeechBrain is not a dependency here).  Randomness is recorded and
replayed: ``torch.rand_like`` (Kumaraswamy uniforms), ``torch.randn_like`` and
``Tensor.exponential_`` (the H-VAE's draws, as make_golden_hvae.py) return recorded tensors, and
``Categorical.sample`` is run once under a seed and its labels recorded.

A seed is accepted only if the reference decode gives the same three sequences on inputs
perturbed by +-1e-4 with two random sign patterns: the GPU test compares decoded labels exactly,
and this keeps it away from ties.

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_md_recipe.py
"""
import json
import os
import re
import sys
import tempfile
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402,F401  (generator-only shims, reference src on sys.path)


def _undo_padding(batch, lengths):
    n = batch.shape[1]
    return [seq[:int(torch.round(l * n))].tolist() for seq, l in zip(batch, lengths)]


_du = types.ModuleType("speechbrain.utils.data_utils")
_du.undo_padding = _undo_padding
sys.modules["speechbrain.utils.data_utils"] = _du
sys.modules["speechbrain.utils"].data_utils = _du

import speechbrain as sb  # noqa: E402  (the stand-in)
from models.MD_VAE.model import SBModel, Target  # noqa: E402  (reference)
from modules.boundary_detector import BoundaryDetector  # noqa: E402  (reference)
from modules.decoder import Decoder  # noqa: E402  (reference)
from modules.fc_block import FCBlock  # noqa: E402  (reference)
from modules.h_vae import HierarchicalVAE  # noqa: E402  (reference)
from modules.phoneme_recognizer import PhonemeRecognizer  # noqa: E402  (reference)
from utils.decode_utils import decode_plvl_md_lbl_seqs_full  # noqa: E402  (reference)
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats  # noqa: E402  (reference)
from utils.metric_stats.md_metric_stats import MDMetricStats  # noqa: E402  (reference)

OUT_DIR = make_golden.OUT_DIR
REF_YAML = os.path.join(make_golden.REF_SRC, "models", "MD_VAE", "model.yaml")
B, T, F, H, L, NPH, Z, NC = 3, 24, 8, 16, 6, 5, 4, 3
WEIGHTS = dict(boundary_kld_weight=0.00001, vae_kld_weight=0.00001, pi_nll_weight=0.001)


class _Batch(dict):
    def to(self, device):
        return self


def _modules():
    fc = lambda sizes, end=False: FCBlock(fc_sizes=sizes, end_activation=end)
    return torch.nn.ModuleDict({
        "feat_fc": fc([F, H, H], True),
        "phoneme_recognizer": PhonemeRecognizer(input_size=F, rnn_hidden_size=H, rnn_num_layers=2,
                                                fc_sizes=[H, H, H, NPH + 2], n_phonemes=NPH),
        "phn_recog_fc": fc([NPH + 2, H, H], True),
        "boundary_detector": BoundaryDetector(input_size=F, rnn_hidden_size=H, rnn_num_layers=2,
                                              fc_sizes=[H, H, H, 1]),
        "concat_fc": fc([2 * H, H, H], True),
        "rnn": torch.nn.LSTM(input_size=H, hidden_size=H, num_layers=2, batch_first=True, dropout=0.0),
        "pi_fc": fc([H, H, H // 2, 2]),
        "encoder": HierarchicalVAE(fc_sizes=[H, H, H], latent_size=Z, num_components=NC),
        "decoder": Decoder(input_size=Z, rnn_hidden_size=H, rnn_num_layers=2, rnn_dropout=0.0,
                           fc_sizes=[2 * H, H, H, F]),
    })


def _batch(g):
    rel_t = torch.tensor([1.0, 0.75, 0.5])
    rel_l = torch.tensor([1.0, 5 / 6, 0.5])
    Ti = [int(torch.round(r * T)) for r in rel_t]
    Li = [int(torch.round(r * L)) for r in rel_l]
    fa, gt = torch.zeros(B, T), torch.zeros(B, T)
    for b in range(B):
        for dst in (fa, gt):
            cuts = torch.randperm(Ti[b] - 1, generator=g)[:Li[b] - 1] + 1
            dst[b, 0] = 1.0
            dst[b, cuts] = 1.0
    seqs = torch.randint(0, NPH, (B, L), generator=g)
    md = torch.randint(0, 2, (B, L), generator=g)
    for b in range(B):
        seqs[b, Li[b]:] = 0
        md[b, Li[b]:] = 0
    prior = (0.06 + 0.43 * torch.rand(NPH + 2, generator=g)).expand(B, NPH + 2).clone()
    return _Batch({
        "id": [f"utt{b}" for b in range(B)],
        "feat": (torch.randn(B, T, F, generator=g), rel_t),
        "gt_cnncl_seq": (seqs, rel_l),
        "fa_boundary_seq": (fa, rel_t),
        "gt_boundary_seq": (gt, rel_t),
        "plvl_gt_md_lbl_seq": (md, rel_l),
        "prior": (prior, torch.ones(B)),
    })


class _Inject:
    """rand_like / randn_like / exponential_ replay recorded tensors in call order;
    Categorical.sample returns the recorded labels."""

    def __init__(self, us, eps, expo, labels):
        self.us, self.eps, self.expo, self.labels = list(us), list(eps), list(expo), labels

    def __enter__(self):
        C = torch.distributions.Categorical
        self._saved = (torch.rand_like, torch.randn_like, torch.Tensor.exponential_, C.sample)
        us, eps, expo, labels = self.us, self.eps, self.expo, self.labels
        torch.rand_like = lambda t, *a, **k: us.pop(0).clone()
        torch.randn_like = lambda t, *a, **k: eps.pop(0).clone()
        torch.Tensor.exponential_ = lambda self_, *a, **k: self_.copy_(expo.pop(0))
        C.sample = lambda self_, *a, **k: labels.clone()
        return self

    def __exit__(self, *exc):
        C = torch.distributions.Categorical
        torch.rand_like, torch.randn_like, torch.Tensor.exponential_, C.sample = self._saved


def _model(modules):
    m = SBModel.__new__(SBModel)
    m.modules = modules
    m.device = "cpu"
    m.stats_loggers = {}
    m.hparams = types.SimpleNamespace(
        epoch_counter=types.SimpleNamespace(current=1),
        normalizer=lambda feats, lens, epoch=None: feats,
        batch_size=B, dataset_name="golden", model_name="md_vae_tiny", **WEIGHTS)
    return m


def _pad(seqs, n):
    return np.stack([np.pad(np.asarray(s, dtype=np.int64), (0, n - len(s)), constant_values=-1)
                     for s in seqs])


def _decode(pred, batch):
    return decode_plvl_md_lbl_seqs_full(
        pred, utt_ids=batch["id"], feat_lens=batch["feat"][1], plvl_cnnl_seqs=batch["gt_cnncl_seq"][0],
        plvl_cnnl_seq_lens=batch["gt_cnncl_seq"][1], prior=batch["prior"][0][0], weight=1.0)


def _same(a, b):
    return all(len(x) == len(y) and all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))
               for x, y in zip(a, b))


def _decode_is_robust(pred, batch, g):
    base = _decode(pred, batch)
    for _ in range(2):
        pert = {}
        for k in ("phn_recog_out", "boundary_v", "pi_logits"):
            v = pred[k].detach()
            sign = torch.randint(0, 2, v.shape, generator=g).float() * 2 - 1
            pert[k] = v + 1e-4 * sign
        pert["boundary_v"] = pert["boundary_v"].clamp(1e-6, 1 - 1e-6)
        if not _same(base, _decode(pert, batch)):
            return False
    return True


def run(seed):
    torch.manual_seed(seed)
    modules = _modules()
    # freshly initialised heads give near-zero logits, and the decode then calls every phoneme
    # correct: widen the recogniser's and the pi network's output layers so that the decoded
    # labels, the argmax and the NLL's labels are a mix of 0s and 1s
    with torch.no_grad():
        modules["phoneme_recognizer"].fc.blocks[-1].weight *= 40.0
        modules["pi_fc"].blocks[-1].weight *= 40.0
    g = torch.Generator().manual_seed(seed + 1)
    batch = _batch(g)
    us = [torch.rand(B, T, generator=g) for _ in range(10)]
    eps_v = torch.randn(B, T, Z, generator=g)
    eps_g = torch.randn(B, T, NC * Z, generator=g)
    expo = torch.empty(B, T, NC).exponential_(generator=g)
    m = _model(modules)
    rec = {"feat": batch["feat"][0].numpy(), "feat_lens": batch["feat"][1].numpy(),
           "gt_cnncl_seq": batch["gt_cnncl_seq"][0].numpy(), "seq_lens": batch["gt_cnncl_seq"][1].numpy(),
           "fa_boundary_seq": batch["fa_boundary_seq"][0].numpy(),
           "gt_boundary_seq": batch["gt_boundary_seq"][0].numpy(),
           "plvl_gt_md_lbl_seq": batch["plvl_gt_md_lbl_seq"][0].numpy(),
           "prior": batch["prior"][0].numpy(),
           "boundary_u": torch.stack(us).numpy(), "eps_v": eps_v.numpy(), "eps_g": eps_g.numpy(),
           "expo": expo.numpy()}
    for n, p in modules.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()
    none_grads = {}

    # the labels Categorical.sample draws for these pi_logits under a seed of their own
    labels = None
    for target, stage, train in ((Target.VAE, sb.Stage.TRAIN, True), (Target.PHN_RECOG, sb.Stage.TRAIN, True),
                                 (Target.B_DETECTOR, sb.Stage.TRAIN, True), (Target.TEST, sb.Stage.TEST, False)):
        name = target.name
        m.target = target
        modules.train(train)
        for p in modules.parameters():
            p.grad = None
        m.stats_loggers = {}
        if stage == sb.Stage.TEST:
            m.stats_loggers = {"plvl_md_stats": MDMetricStats(), "boundary_stats": BoundaryMetricStats()}
        if labels is None:  # first pass (VAE): find pi_logits, sample once with the real sampler
            with _Inject(us, [eps_v, eps_g], [expo], torch.zeros(B, T, dtype=torch.int64)), torch.no_grad():
                pi_logits = m.compute_forward(batch, stage)["pi_logits"]
            torch.manual_seed(seed + 2)
            labels = torch.distributions.Categorical(logits=pi_logits).sample()
            rec["pi_labels"] = labels.numpy()
        captured = {}
        orig = m.compute_and_save_losses

        def capture(losses, _orig=orig, _c=captured):
            _c.update({k: v.detach().clone() for k, v in losses.items()})
            return _orig(losses)

        m.compute_and_save_losses = capture
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp, _Inject(us, [eps_v, eps_g], [expo], labels):
            os.makedirs(os.path.join(tmp, "datasets", "golden"))
            os.chdir(tmp)
            try:
                if train:
                    pred = m.compute_forward(batch, stage)
                    loss = m.compute_objectives(pred, batch, stage)
                    loss.backward()
                else:
                    with torch.no_grad():
                        pred = m.compute_forward(batch, stage)
                        loss = m.compute_objectives(pred, batch, stage)
                    with open(os.path.join("datasets", "golden", "saved_md_results", "md_vae_tiny.json")) as f:
                        rec[f"{name}/saved_md_result_json"] = np.array(f.read())
            finally:
                os.chdir(cwd)
                del m.compute_and_save_losses
        rec[f"{name}/total"] = loss.detach().numpy()
        for k, v in captured.items():
            rec[f"{name}/loss/{k}"] = v.numpy()
        if "pi_logits" in pred:
            if not _decode_is_robust(pred, batch, g):
                return None
            rec[f"{name}/pi_logits"] = pred["pi_logits"].detach().numpy()
            rec[f"{name}/sampled_pi"] = pred["sampled_pi"].detach().numpy()
            bnd, flvl, plvl = _decode(pred, batch)
            rec[f"{name}/decoded_boundary"] = _pad(bnd, T)
            rec[f"{name}/decoded_flvl"] = _pad(flvl, T)
            rec[f"{name}/decoded_plvl"] = _pad(plvl, L)
            assert _same([bnd], [[t.numpy() for t in pred["decoded_boundary_seq"]]])
        if train:
            none_grads[name] = []
            for n, p in modules.named_parameters():
                if p.grad is None:
                    none_grads[name].append(n)
                else:
                    rec[f"{name}/grad/{n}"] = p.grad.numpy().copy()
        else:
            rec[f"{name}/md_summary_json"] = np.array(json.dumps(m.stats_loggers["plvl_md_stats"].summarize()))
            rec[f"{name}/boundary_summary_json"] = np.array(
                json.dumps(m.stats_loggers["boundary_stats"].summarize()))
    meta = dict(B=B, T=T, F=F, H=H, L=L, n_phonemes=NPH, Z=Z, NC=NC, seed=seed, weights=WEIGHTS,
                batch_size=B, none_grads=none_grads,
                param_names=[n for n, _ in modules.named_parameters()])
    rec["meta_json"] = np.array(json.dumps(meta))
    return rec


def yaml_keys():
    """Key names of the reference's model.yaml: top level, ``modules:`` and ``recoverables:``."""
    text = open(REF_YAML).read()
    top = re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", text, flags=re.M)

    def block(name, indent):
        body = re.search(rf"^{indent}{name}:\n((?:{indent}    \S.*\n?)+)", text, flags=re.M).group(1)
        return re.findall(r"^\s+([A-Za-z_][A-Za-z0-9_]*):", body, flags=re.M)

    return {"top_level": top, "modules": block("modules", ""), "recoverables": block("recoverables", "    ")}


if __name__ == "__main__":
    torch.set_num_threads(1)
    for seed in range(51, 71):
        rec = run(seed)
        if rec is not None:
            break
        print("seed", seed, "refused: the decode is within 1e-4 of a tie")
    else:
        raise SystemExit("no seed accepted")
    path = os.path.join(OUT_DIR, "md_vae_tiny.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes, seed", seed)
    with open(os.path.join(OUT_DIR, "md_vae_yaml_keys.json"), "w") as f:
        json.dump(yaml_keys(), f, indent=1)
