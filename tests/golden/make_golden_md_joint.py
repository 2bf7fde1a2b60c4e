"""Golden fixtures for the joint MD-VAE recipes (ml-vae_amd/models/MD_VAE_joint, MD_VAE_joint_ll).

TEST INFRASTRUCTURE ONLY.  Runs only where a checkout of the reference is available; no test needs
it.  It reuses ``make_golden.py``'s import shims and ``make_golden_md_recipe.py``'s modules, batch,
recorded-noise injection and seed-acceptance rule, and runs the reference's own
``compute_forward`` + ``compute_objectives`` of ``models.MD_VAE_joint.model.SBModel``
(ref:src/models/MD_VAE_joint/model.py:42-167) and ``models.MD_VAE_joint_ll.model.SBModel``
(ref:src/models/MD_VAE_joint_ll/model.py:40-177) on a stand-in ``self``; only data is written:
``md_vae_joint_tiny.npz``, ``md_vae_joint_ll_tiny.npz`` and the key names of the two model.yaml files
(``md_vae_joint_yaml_keys.json``, ``md_vae_joint_ll_yaml_keys.json``).

The same tiny shapes as md_vae_tiny (B=3, T=24, F=8, every hidden size 16, L=6, n_phonemes=5, Z=4,
NC=3; frame lengths 1.0 / 0.75 / 0.5; dropouts 0; widened output layers), one TRAIN pass in train
mode and one TEST pass in eval mode per recipe.  TRAIN: mean losses, total, pi_logits, sampled_pi,
gradients and the names of the parameters without one (and, for joint_ll, whose forward decodes,
the decoded sequences); TEST: losses, the three decoded sequences, the MD and boundary summaries
(and, for joint, the saved-results JSON).

The reference's MD_VAE_joint calls ``save_md_result`` in every stage, which raises KeyError outside
evaluated stages (no decoded sequences in the predictions): for its TRAIN pass the call is replaced
by a no-op, here in the generator only.

A seed is accepted only if every decode that enters the fixture is unchanged under +-1e-4
perturbations of its inputs (make_golden_md_recipe._decode_is_robust).

Usage (from an empty directory):  PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_md_joint.py
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

import make_golden  # noqa: E402,F401  (generator-only shims, reference src on sys.path)
import make_golden_md_recipe as R  # noqa: E402  (modules, batch, injection, acceptance rule)

import speechbrain as sb  # noqa: E402  (the stand-in)
from models.MD_VAE_joint.model import SBModel as Joint  # noqa: E402  (reference)
from models.MD_VAE_joint_ll.model import SBModel as JointLL  # noqa: E402  (reference)
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats  # noqa: E402  (reference)
from utils.metric_stats.md_metric_stats import MDMetricStats  # noqa: E402  (reference)

OUT_DIR = make_golden.OUT_DIR
B, T, L, Z, NC = R.B, R.T, R.L, R.Z, R.NC
RECIPES = {
    "md_vae_joint": dict(cls=Joint, ref_dir="MD_VAE_joint", saves=True, decodes_in_train=False,
                         weights=dict(boundary_kld_weight=0.00001, vae_kld_weight=0.00001,
                                      phn_recog_bce_weight=10, boundary_bce_weight=10)),
    "md_vae_joint_ll": dict(cls=JointLL, ref_dir="MD_VAE_joint_ll", saves=False, decodes_in_train=True,
                            weights=dict(boundary_kld_weight=0.00001, vae_kld_weight=0.00001,
                                         pi_nll_weight=0.001)),
}


def _model(cls, modules, weights, model_name):
    m = cls.__new__(cls)
    m.modules = modules
    m.device = "cpu"
    m.stats_loggers = {}
    m.hparams = types.SimpleNamespace(
        epoch_counter=types.SimpleNamespace(current=1),
        normalizer=lambda feats, lens, epoch=None: feats,
        batch_size=B, dataset_name="golden", model_name=model_name, **weights)
    return m


def run(recipe, seed):
    spec = RECIPES[recipe]
    model_name = recipe + "_tiny"
    torch.manual_seed(seed)
    modules = R._modules()
    with torch.no_grad():  # as make_golden_md_recipe: decoded labels and argmax a mix of 0s and 1s
        modules["phoneme_recognizer"].fc.blocks[-1].weight *= 40.0
        modules["pi_fc"].blocks[-1].weight *= 40.0
    g = torch.Generator().manual_seed(seed + 1)
    batch = R._batch(g)
    us = [torch.rand(B, T, generator=g) for _ in range(10)]
    eps_v = torch.randn(B, T, Z, generator=g)
    eps_g = torch.randn(B, T, NC * Z, generator=g)
    expo = torch.empty(B, T, NC).exponential_(generator=g)
    m = _model(spec["cls"], modules, spec["weights"], model_name)
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

    # the labels Categorical.sample draws for the TRAIN pass's pi_logits under a seed of their own
    modules.train(True)
    with R._Inject(us, [eps_v, eps_g], [expo], torch.zeros(B, T, dtype=torch.int64)), torch.no_grad():
        pi_logits = m.compute_forward(batch, sb.Stage.TRAIN)["pi_logits"]
    torch.manual_seed(seed + 2)
    labels = torch.distributions.Categorical(logits=pi_logits).sample()
    rec["pi_labels"] = labels.numpy()

    for name, stage, train in (("TRAIN", sb.Stage.TRAIN, True), ("TEST", sb.Stage.TEST, False)):
        modules.train(train)
        for p in modules.parameters():
            p.grad = None
        m.stats_loggers = {}
        if not train:
            m.stats_loggers = {"plvl_md_stats": MDMetricStats(), "boundary_stats": BoundaryMetricStats()}
        captured = {}
        orig = m.compute_and_save_losses

        def capture(losses, _orig=orig, _c=captured):
            _c.update({k: v.detach().clone() for k, v in losses.items()})
            return _orig(losses)

        m.compute_and_save_losses = capture
        if train and spec["saves"]:
            m.save_md_result = lambda batch_, predictions_: None  # see the module docstring
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp, R._Inject(us, [eps_v, eps_g], [expo], labels):
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
                    if spec["saves"]:
                        with open(os.path.join("datasets", "golden", "saved_md_results", model_name + ".json")) as f:
                            rec[f"{name}/saved_md_result_json"] = np.array(f.read())
            finally:
                os.chdir(cwd)
                del m.compute_and_save_losses
                if "save_md_result" in m.__dict__:
                    del m.save_md_result
        rec[f"{name}/total"] = loss.detach().numpy()
        for k, v in captured.items():
            rec[f"{name}/loss/{k}"] = v.numpy()
        rec[f"{name}/pi_logits"] = pred["pi_logits"].detach().numpy()
        rec[f"{name}/sampled_pi"] = pred["sampled_pi"].detach().numpy()
        if not train or spec["decodes_in_train"]:
            if not R._decode_is_robust(pred, batch, g):
                return None
            bnd, flvl, plvl = R._decode(pred, batch)
            rec[f"{name}/decoded_boundary"] = R._pad(bnd, T)
            rec[f"{name}/decoded_flvl"] = R._pad(flvl, T)
            rec[f"{name}/decoded_plvl"] = R._pad(plvl, L)
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
    meta = dict(B=B, T=T, F=R.F, H=R.H, L=L, n_phonemes=R.NPH, Z=Z, NC=NC, seed=seed,
                weights=spec["weights"], batch_size=B, none_grads=none_grads,
                param_names=[n for n, _ in modules.named_parameters()])
    rec["meta_json"] = np.array(json.dumps(meta))
    return rec


def yaml_keys(ref_dir):
    R.REF_YAML = os.path.join(make_golden.REF_SRC, "models", ref_dir, "model.yaml")
    return R.yaml_keys()


if __name__ == "__main__":
    torch.set_num_threads(1)
    for recipe, spec in RECIPES.items():
        for seed in range(51, 91):
            rec = run(recipe, seed)
            if rec is not None:
                break
            print(recipe, "seed", seed, "refused: a decode is within 1e-4 of a tie")
        else:
            raise SystemExit("no seed accepted")
        path = os.path.join(OUT_DIR, recipe + "_tiny.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes, seed", seed,
              "none_grads", json.loads(str(rec["meta_json"]))["none_grads"])
        with open(os.path.join(OUT_DIR, recipe + "_yaml_keys.json"), "w") as f:
            json.dump(yaml_keys(spec["ref_dir"]), f, indent=1)
