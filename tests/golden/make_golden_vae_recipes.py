"""Golden fixtures for the single-encoder VAE recipes (ml-vae_amd/models/test_gmm_vae and
test_h_vae): ``test_gmm_vae_tiny.npz``, ``test_h_vae_tiny.npz`` and the key names of the two
reference yamls (``*_yaml_keys.json``).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs
it.  It reuses the import shims of ``make_golden_md_recipe.py`` and runs the reference's own
``SBModel.compute_forward`` + ``compute_objectives`` of each recipe on a stand-in ``self`` built
from the reference's modules; only data is written.

One batch per recipe: B = 3, T = 24, F = 8, every hidden size 16, Z = 4, 3 components, both LSTM
dropouts 0; frame lengths 1.0, one whose fp32(L / T) * T lands above L (the mask admits one more
frame) and 0.5.  One TRAIN pass (train mode, with backward) and one TEST pass (eval mode: the
argmax pi).  The normaliser is the identity.  Randomness is recorded and replayed with
make_golden_md_recipe's ``_Inject``: ``torch.randn_like`` (eps), ``Tensor.exponential_`` (the
Gumbel draws) and ``Categorical.sample`` (the labels, drawn once under a seed of their own).

A test_h_vae seed is accepted only if the drawn labels and the argmax are both a mix of 0s and 1s
and every frame's pi logits differ by >= 1e-3 of the largest magnitude.

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_vae_recipes.py
"""
import importlib
import json
import os
import sys
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden  # noqa: E402,F401
import make_golden_md_recipe as R  # noqa: E402  (generator-only shims, reference src on sys.path)
import speechbrain as sb  # noqa: E402  (the stand-in)
from make_golden_upstream import yaml_keys  # noqa: E402
from models.md_model import MDModel  # noqa: E402  (reference)
from modules.decoder import Decoder  # noqa: E402  (reference)
from modules.fc_block import FCBlock  # noqa: E402  (reference)
from modules.gmm_vae import GMMVAE  # noqa: E402  (reference)
from modules.h_vae import HierarchicalVAE  # noqa: E402  (reference)

GmmModel = importlib.import_module("models.test_gmm_vae.model").SBModel  # (reference)
HvaeModel = importlib.import_module("models.test_h_vae.model").SBModel  # (reference)

B, T, F, H, E, Z, NC = 3, 24, 8, 16, 16, 4, 3
GMM_WEIGHTS = dict(kld_weight=0.001)
HVAE_WEIGHTS = dict(vae_kld_weight=0.001)
GAP = 1e-3


def _lens():
    quirk = make_golden.fp32_quirk_lens(T, 1)
    mid = quirk[-1] / T if quirk else 0.75
    return torch.tensor([1.0, mid, 0.5], dtype=torch.float32), bool(quirk)


def _model(cls, modules, **hp):
    m = cls.__new__(cls)
    m.modules = modules
    m.device = "cpu"
    m.stats_loggers = {}
    m.hparams = types.SimpleNamespace(epoch_counter=types.SimpleNamespace(current=1),
                                      normalizer=lambda feats, lens, epoch=None: feats,
                                      batch_size=B, **hp)
    return m


def _passes(m, modules, batch, rec, inject):
    """The TRAIN pass (with backward) and the TEST pass of one recipe, recorded into rec."""
    for name, stage, train in (("TRAIN", sb.Stage.TRAIN, True), ("TEST", sb.Stage.TEST, False)):
        modules.train(train)
        captured = {}
        orig = MDModel.compute_and_save_losses

        def capture(self_, losses, _orig=orig, _c=captured):
            _c.update({k: v.detach().clone() for k, v in losses.items()})
            return _orig(self_, losses)

        # the recipes call super().compute_and_save_losses: wrapped on the class
        MDModel.compute_and_save_losses = capture
        try:
            with inject(), torch.set_grad_enabled(train):
                pred = m.compute_forward(batch, stage)
                loss = m.compute_objectives(pred, batch, stage)
        finally:
            MDModel.compute_and_save_losses = orig
        assert captured
        rec[f"{name}/loss"] = loss.detach().numpy()
        for k, v in captured.items():
            rec[f"{name}/loss/{k}"] = v.numpy()
        rec[f"{name}/gmm_weight"] = pred["encoder_out"]["gmm_weight"].detach().numpy()
        rec[f"{name}/sampled_h"] = pred["encoder_out"]["sampled_h"].detach().numpy()
        if train:
            loss.backward()
            none = []
            for n, p in modules.named_parameters():
                if p.grad is None:
                    none.append(n)
                else:
                    rec[f"TRAIN/grad/{n}"] = p.grad.numpy().copy()
                    p.grad = None
    return none


def _decoder():
    return Decoder(input_size=Z, rnn_hidden_size=H, rnn_num_layers=2, rnn_dropout=0.0,
                   fc_sizes=[2 * H, E, E, F])


def run_gmm(seed):
    torch.manual_seed(seed)
    modules = torch.nn.ModuleDict({
        "encoder": GMMVAE(fc_sizes=[F, E, E], latent_size=Z, num_components=NC),
        "decoder": _decoder()})
    g = torch.Generator().manual_seed(seed + 1)
    lens, quirk = _lens()
    batch = R._Batch({"id": [f"utt{b}" for b in range(B)], "feat": (torch.randn(B, T, F, generator=g), lens)})
    eps = torch.randn(B, T, NC * Z, generator=g)
    expo = torch.empty(B, T, NC).exponential_(generator=g)
    rec = {"feat": batch["feat"][0].numpy(), "feat_lens": lens.numpy(), "eps": eps.numpy(),
           "expo": expo.numpy()}
    for n, p in modules.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()
    m = _model(GmmModel, modules, **GMM_WEIGHTS)
    none = _passes(m, modules, batch, rec, lambda: R._Inject([], [eps], [expo], None))
    rec["meta_json"] = np.array(json.dumps(dict(
        B=B, T=T, F=F, H=H, E=E, Z=Z, NC=NC, seed=seed, weights=GMM_WEIGHTS, quirk_len=quirk,
        none_grads=none, param_names=[n for n, _ in modules.named_parameters()])))
    return rec


def run_hvae(seed):
    torch.manual_seed(seed)
    modules = torch.nn.ModuleDict({
        "rnn": torch.nn.LSTM(input_size=F, hidden_size=H, num_layers=2, batch_first=True, dropout=0.0),
        "pi_fc": FCBlock(fc_sizes=[H, H, H // 2, 2]),
        "encoder": HierarchicalVAE(fc_sizes=[H, E, E], latent_size=Z, num_components=NC),
        "decoder": _decoder()})
    with torch.no_grad():  # a fresh head gives near-equal logits: widen it, as make_golden_md_recipe
        modules["pi_fc"].blocks[-1].weight *= 40.0
    g = torch.Generator().manual_seed(seed + 1)
    lens, quirk = _lens()
    batch = R._Batch({"id": [f"utt{b}" for b in range(B)], "feat": (torch.randn(B, T, F, generator=g), lens)})
    eps_v = torch.randn(B, T, Z, generator=g)
    eps_g = torch.randn(B, T, NC * Z, generator=g)
    expo = torch.empty(B, T, NC).exponential_(generator=g)
    with torch.no_grad():
        pi_logits = modules["pi_fc"](modules["rnn"](batch["feat"][0])[0])
    top = torch.sort(pi_logits, dim=-1).values
    if not bool(((top[..., 1] - top[..., 0]) >= GAP * pi_logits.abs().max()).all()):
        return None
    torch.manual_seed(seed + 2)
    labels = torch.distributions.Categorical(logits=pi_logits).sample()
    argmax = torch.argmax(pi_logits, dim=-1)
    if not (0 < int(labels.sum()) < labels.numel() and 0 < int(argmax.sum()) < argmax.numel()):
        return None
    rec = {"feat": batch["feat"][0].numpy(), "feat_lens": lens.numpy(), "eps_v": eps_v.numpy(),
           "eps_g": eps_g.numpy(), "expo": expo.numpy(), "pi_labels": labels.numpy(),
           "pi_logits": pi_logits.numpy()}
    for n, p in modules.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()
    m = _model(HvaeModel, modules, **HVAE_WEIGHTS)
    none = _passes(m, modules, batch, rec, lambda: R._Inject([], [eps_v, eps_g], [expo], labels))
    assert none == [n for n, _ in modules.named_parameters() if n.startswith("pi_fc.")], none
    rec["meta_json"] = np.array(json.dumps(dict(
        B=B, T=T, F=F, H=H, E=E, Z=Z, NC=NC, seed=seed, weights=HVAE_WEIGHTS, quirk_len=quirk,
        none_grads=none, param_names=[n for n, _ in modules.named_parameters()])))
    return rec


if __name__ == "__main__":
    torch.set_num_threads(1)
    for recipe, fn in (("test_gmm_vae", run_gmm), ("test_h_vae", run_hvae)):
        for seed in range(91, 191):
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
