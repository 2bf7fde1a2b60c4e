"""Golden fixture for the MD_VAE_sfl recipe (ml-vae_amd/models/MD_VAE_sfl/model.py).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs it.  It imports
``make_golden_md_recipe`` for the import shims, the batch and the modules, and runs the
reference's own ``models.MD_VAE_sfl.model.SBModel.compute_forward`` + ``compute_objectives``
(ref:src/models/MD_VAE_sfl/model.py:54-189) on a stand-in ``self``; only data is written:
``md_vae_sfl_tiny.npz`` and ``md_vae_sfl_yaml_keys.json`` (the key names of the reference's
model.yaml).

The sizes of md_vae_tiny (B=3, T=24, F=8, hidden sizes 16, Z=4, 3 components, both dropouts 0)
plus baseline_fc [H, H, H, 1]; the recogniser output's FC carries the reference's module name
phn_recog_out_fc.  pi_mcmc_num K = 3.  Two targets: VAE in train mode, TEST in eval mode (K = 1,
the argmax).  The loss weights are non-unit and mutually distinct, so a swapped weight, or the KL
weight's 2249 / batch_size scaling applied inside the reward, changes the numbers.

Randomness is recorded and replayed per draw in call order: K sets of ``randn_like`` /
``exponential_`` and K recorded ``Categorical.sample`` label tensors (drawn once by the real
sampler under a seed).  Forward hooks on the encoder and the decoder record each draw's row means
of vae_kld_loss and recon_loss, and baseline_fc's output is recorded, so that the score-function
terms can be recomputed from the fixture alone.

pi_fc's output layer is widened by PI_SCALE and its bias re-centred on the batch's mean logit
gap, enough that l1 - l0 spans a few units around 0 (a fresh pi_fc gives near-constant logits;
widening alone moves their common offset with the spread and saturates softmax, as md_vae_tiny's
x40 does, which makes the rif gradient vanish).  A seed is accepted only if
* the decode is robust to +-1e-4 (make_golden_md_recipe's check), for both targets;
* every draw contains both labels, and the K draws differ pairwise;
* the gradients of pi_fc's last layer and of baseline_fc's first layer both exceed 1e-3 in
  maximum magnitude.

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_md_sfl.py
"""
import json
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden_md_recipe as R  # noqa: E402  (shims, batch, modules; reference src on sys.path)

import speechbrain as sb  # noqa: E402  (the stand-in)
from models.MD_VAE.model import Target  # noqa: E402  (reference)
from models.MD_VAE_sfl.model import SBModel  # noqa: E402  (reference)
from modules.fc_block import FCBlock  # noqa: E402  (reference)
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats  # noqa: E402  (reference)
from utils.metric_stats.md_metric_stats import MDMetricStats  # noqa: E402  (reference)

B, T, H, L, Z, NC = R.B, R.T, R.H, R.L, R.Z, R.NC
K = 3
PI_SCALE = 400.0
WEIGHTS = dict(boundary_kld_weight=0.00001, recon_weight=0.7, vae_kld_weight=0.3, pi_nll_weight=0.5,
               rif_weight=0.9, entropy_weight=0.01, baseline_weight=0.4)
MODEL_NAME = "md_vae_sfl_tiny"
SFL_KEYS = ("pi_nll_loss", "rif_loss", "entropy_loss", "baseline_loss")


def _modules():
    """make_golden_md_recipe's modules in the reference yaml's order, under its names."""
    base = R._modules()
    mods = torch.nn.ModuleDict()
    for name, mod in base.items():
        mods["phn_recog_out_fc" if name == "phn_recog_fc" else name] = mod
    mods["baseline_fc"] = FCBlock(fc_sizes=[H, H, H, 1], end_activation=False)
    return mods


class _Inject(R._Inject):
    """As the base, with one recorded label tensor per Categorical.sample call."""

    def __enter__(self):
        super().__enter__()
        labels = list(self.labels)
        torch.distributions.Categorical.sample = lambda self_, *a, **k: labels.pop(0).clone()
        return self


def _model(modules):
    m = SBModel.__new__(SBModel)
    m.modules = modules
    m.device = "cpu"
    m.stats_loggers = {}
    m.hparams = types.SimpleNamespace(
        epoch_counter=types.SimpleNamespace(current=1),
        normalizer=lambda feats, lens, epoch=None: feats,
        batch_size=B, dataset_name="golden", model_name=MODEL_NAME, pi_mcmc_num=K, **WEIGHTS)
    return m


def run(seed):
    torch.manual_seed(seed)
    modules = _modules()
    with torch.no_grad():
        modules["phoneme_recognizer"].fc.blocks[-1].weight *= 40.0
        modules["pi_fc"].blocks[-1].weight *= PI_SCALE
    g = torch.Generator().manual_seed(seed + 1)
    batch = R._batch(g)
    us = [torch.rand(B, T, generator=g) for _ in range(10)]
    eps_v = torch.randn(K, B, T, Z, generator=g)
    eps_g = torch.randn(K, B, T, NC * Z, generator=g)
    expo = torch.empty(K, B, T, NC).exponential_(generator=g)
    eps_calls = [e for k in range(K) for e in (eps_v[k], eps_g[k])]
    m = _model(modules)
    rec = {"feat": batch["feat"][0].numpy(), "feat_lens": batch["feat"][1].numpy(),
           "gt_cnncl_seq": batch["gt_cnncl_seq"][0].numpy(), "seq_lens": batch["gt_cnncl_seq"][1].numpy(),
           "fa_boundary_seq": batch["fa_boundary_seq"][0].numpy(),
           "gt_boundary_seq": batch["gt_boundary_seq"][0].numpy(),
           "plvl_gt_md_lbl_seq": batch["plvl_gt_md_lbl_seq"][0].numpy(),
           "prior": batch["prior"][0].numpy(),
           "boundary_u": torch.stack(us).numpy(), "eps_v": eps_v.numpy(), "eps_g": eps_g.numpy(),
           "expo": expo.numpy()}

    # each draw's row means of the H-VAE's KL and the decoder's reconstruction loss, the baseline
    draws = {"kld": [], "recon": [], "baseline": []}
    hooks = [
        modules["encoder"].register_forward_hook(
            lambda mod, a, out: draws["kld"].append(out["losses"]["vae_kld_loss"].detach().mean(-1))),
        modules["decoder"].register_forward_hook(
            lambda mod, a, out: draws["recon"].append(out["losses"]["recon_loss"].detach().mean(-1))),
        modules["baseline_fc"].register_forward_hook(
            lambda mod, a, out: draws["baseline"].append(out.detach().squeeze(-1))),
    ]

    def probe():
        zeros = [torch.zeros(B, T, dtype=torch.int64)] * K
        with _Inject(us, eps_calls, list(expo), zeros), torch.no_grad():
            return m.compute_forward(batch, sb.Stage.TRAIN)["pi_logits"]

    modules.train(True)
    m.target = Target.VAE
    with torch.no_grad():  # centre the logit gap
        pl = probe()
        modules["pi_fc"].blocks[-1].bias[1] -= (pl[..., 1] - pl[..., 0]).mean()
    for n, p in modules.named_parameters():
        rec["param/" + n] = p.detach().numpy().copy()
    # the K label tensors Categorical.sample draws for these pi_logits under a seed of their own
    pi_logits = probe()
    torch.manual_seed(seed + 2)
    dist = torch.distributions.Categorical(logits=pi_logits)
    labels = [dist.sample() for _ in range(K)]
    for k in range(K):
        if len(torch.unique(labels[k])) != 2:
            return "a draw holds one label only"
        if any(torch.equal(labels[k], labels[j]) for j in range(k)):
            return "two draws are equal"
    rec["pi_labels"] = torch.stack(labels).numpy()
    span = (pi_logits[..., 1] - pi_logits[..., 0]).abs().max().item()
    none_grads = {}

    for target, stage, train in ((Target.VAE, sb.Stage.TRAIN, True), (Target.TEST, sb.Stage.TEST, False)):
        name = target.name
        m.target = target
        modules.train(train)
        for p in modules.parameters():
            p.grad = None
        for v in draws.values():
            v.clear()
        m.stats_loggers = {}
        if stage == sb.Stage.TEST:
            m.stats_loggers = {"plvl_md_stats": MDMetricStats(), "boundary_stats": BoundaryMetricStats()}
        captured = {}
        orig = m.compute_and_save_losses

        def capture(losses, _orig=orig, _c=captured):
            _c.update({k: v.detach().clone() for k, v in losses.items()})
            return _orig(losses)

        m.compute_and_save_losses = capture
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp, _Inject(us, eps_calls, list(expo), labels):
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
                    with open(os.path.join("datasets", "golden", "saved_md_results", MODEL_NAME + ".json")) as f:
                        rec[f"{name}/saved_md_result_json"] = np.array(f.read())
            finally:
                os.chdir(cwd)
                del m.compute_and_save_losses
        n_draws = K if train else 1
        assert all(len(v) == n_draws for v in draws.values())
        rec[f"{name}/total"] = loss.detach().numpy()
        for k, v in captured.items():
            rec[f"{name}/loss/{k}"] = v.numpy()
        for k in SFL_KEYS:  # per frame [B, T], before the length mask
            rec[f"{name}/frame/{k}"] = pred["losses"][k].detach().numpy()
        rec[f"{name}/draw_kld_mean"] = torch.stack(draws["kld"]).numpy()
        rec[f"{name}/draw_recon_mean"] = torch.stack(draws["recon"]).numpy()
        rec[f"{name}/baseline"] = draws["baseline"][0].numpy()
        if not R._decode_is_robust(pred, batch, g):
            return "the decode is within 1e-4 of a tie"
        rec[f"{name}/pi_logits"] = pred["pi_logits"].detach().numpy()
        rec[f"{name}/sampled_pi"] = pred["sampled_pi"].detach().numpy()
        bnd, flvl, plvl = R._decode(pred, batch)
        rec[f"{name}/decoded_boundary"] = R._pad(bnd, T)
        rec[f"{name}/decoded_flvl"] = R._pad(flvl, T)
        rec[f"{name}/decoded_plvl"] = R._pad(plvl, L)
        if train:
            assert torch.equal(pred["sampled_pi"], labels[-1].float())
            none_grads[name] = []
            for n, p in modules.named_parameters():
                if p.grad is None:
                    none_grads[name].append(n)
                else:
                    rec[f"{name}/grad/{n}"] = p.grad.numpy().copy()
            g_pi = modules["pi_fc"].blocks[-1].weight.grad.abs().max().item()
            g_bl = modules["baseline_fc"].blocks[0].weight.grad.abs().max().item()
            if min(g_pi, g_bl) <= 1e-3:
                return f"gradients too small: pi_fc {g_pi:.2e}, baseline_fc {g_bl:.2e}"
        else:
            assert torch.equal(pred["sampled_pi"], torch.argmax(pred["pi_logits"], -1).float())
            rec[f"{name}/md_summary_json"] = np.array(json.dumps(m.stats_loggers["plvl_md_stats"].summarize()))
            rec[f"{name}/boundary_summary_json"] = np.array(
                json.dumps(m.stats_loggers["boundary_stats"].summarize()))
    for h in hooks:
        h.remove()
    meta = dict(B=B, T=T, F=R.F, H=H, L=L, n_phonemes=R.NPH, Z=Z, NC=NC, K=K, seed=seed, weights=WEIGHTS,
                batch_size=B, pi_scale=PI_SCALE, max_logit_gap=span, grad_pi_fc_last=g_pi,
                grad_baseline_fc_first=g_bl, none_grads=none_grads,
                param_names=[n for n, _ in modules.named_parameters()])
    rec["meta_json"] = np.array(json.dumps(meta))
    return rec


def yaml_keys():
    R.REF_YAML = os.path.join(R.make_golden.REF_SRC, "models", "MD_VAE_sfl", "model.yaml")
    return R.yaml_keys()


if __name__ == "__main__":
    torch.set_num_threads(1)
    for seed in range(71, 111):
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
    with open(os.path.join(R.OUT_DIR, "md_vae_sfl_yaml_keys.json"), "w") as f:
        json.dump(yaml_keys(), f, indent=1)
