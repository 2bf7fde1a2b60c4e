"""Timings of the H-VAE's latent stretch, composed against fused, on the device at the recipes'
shape (B = 8, T = 500, the yamls' sizes: Z = 32, 3 components; DESIGN.md, "The fused H-VAE latent
kernel").

    python tools/hvae_latent_step.py [--runs 5] [--iters 20] [--steps 10] [--only stretch|h_vae|gmm_vae]

1. The encoder's latent stretch, forward + backward, on fixed head outputs ml [B, T, 2Z] and
   P [B, T, 4NZ + N] with library draws: ReparamKLFn + GmmLatentFn + the eight apply_weight and four
   torch.stack of HierarchicalVAE.forward against one ops.hvae_latent; and the GMM-only stretch of
   test_gmm_vae (GmmLatentFn + two apply_weight against one ops.gmm_collapsed).  The cotangents are
   the recipes': d_h and d_kl.
2. The test_h_vae training step (forward, objectives, backward, Adam) with ``fused_latent`` off and on.
3. The test_gmm_vae training step, the same way.

The forms run on the same build in alternating runs; the medians over the runs and the spread
(min .. max) are printed, one JSON line per measurement.  Times are host clocks around work that
ends in a device synchronise."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ml-vae_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools.lstm_pair_step import alternate, report  # noqa: E402

TAU = 0.1


# --------------------------------------------------------------------------- 1. the stretch
def stretch(a):
    from mlvae_hip import ops
    B, T, Z, N = a.B, a.T, a.Z, a.N
    NZ = N * Z
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    ml, Pm = (0.5 * r(B, T, 2 * Z)).requires_grad_(True), (0.5 * r(B, T, 4 * NZ + N)).requires_grad_(True)
    pi = torch.nn.functional.one_hot(torch.randint(0, 2, (B, T), generator=g), 2).float().cuda()
    ch, ck = r(B, T, Z), r(B, T, Z)

    def draws():
        return ops.randn((B, T, Z)), ops.randn((B, T, NZ)), int(torch.randint(0, 2 ** 62, (1,)).item())

    def finish(h, kl):
        ml.grad = Pm.grad = None
        torch.autograd.backward([h, kl], [ch, ck])
        return h, kl

    def h_composed():
        eps_v, eps_g, seed = draws()
        zv, klv = ops.ReparamKLFn.apply(ml, eps_v)
        z, kl, w = ops.GmmLatentFn.apply(Pm, eps_g, None, N, Z, TAU, seed)
        v = {"mean": ml[..., :Z], "log_var": ml[..., Z:], "sampled_h": zv, "loss": klv}
        gm = {"mean": Pm[..., 2 * NZ:3 * NZ], "log_var": Pm[..., 3 * NZ:4 * NZ], "sampled_h": z, "loss": kl}
        out = {k: ops.apply_weight(torch.stack([v[k], ops.apply_weight(gm[k], w)], dim=2), pi) for k in v}
        return finish(out["sampled_h"], out["loss"])

    def h_fused():
        eps_v, eps_g, seed = draws()
        _, _, h, kl, _ = ops.hvae_latent(ml, Pm, pi, eps_v, eps_g, None, N, Z, TAU, seed)
        return finish(h, kl)

    def g_composed():
        _, eps_g, seed = draws()
        z, kl, w = ops.GmmLatentFn.apply(Pm, eps_g, None, N, Z, TAU, seed)
        return finish(ops.apply_weight(z, w), ops.apply_weight(kl, w))

    def g_fused():
        _, eps_g, seed = draws()
        h, kl, _ = ops.gmm_collapsed(Pm, eps_g, None, N, Z, TAU, seed)
        return finish(h, kl)

    what = f"B={B} T={T} Z={Z} N={N}, fwd+bwd with the draws"
    report(f"H-VAE latent stretch, {what}",
           alternate({"composed": h_composed, "fused": h_fused}, a.runs, a.iters, warmup=3),
           {"iters_per_run": a.iters})
    report(f"GMM-only latent stretch, {what}",
           alternate({"composed": g_composed, "fused": g_fused}, a.runs, a.iters, warmup=3),
           {"iters_per_run": a.iters})


# --------------------------------------------------------------------------- 2, 3. the steps
def training_step(a, recipe):
    import importlib
    import warnings
    from brain import Stage
    from brain.dataio import PaddedBatch
    from hyperpyyaml import load_hyperpyyaml
    from utils.data_io import SyntheticSet
    SBModel = importlib.import_module(f"models.{recipe}.model").SBModel
    models = {}
    for name, on in (("fused_latent_off", False), ("fused_latent_on", True)):
        ov = (f"dataset: synthetic\nmodel_class: {recipe}\nmodel_name: hvae_latent_step\n"
              f"batch_size: {a.B}\nmodel: !include:../models/{recipe}/model.yaml\n")
        with open(os.path.join(PKG, "config", "run.yaml")) as f:
            hp = load_hyperpyyaml(f, [{"model": {"input_size": a.F, "fused_latent": on}}, ov])
        m = SBModel(modules=hp["model"]["modules"], hparams=dict(hp["model"]), run_opts={"device": "cuda:0"})
        m.init_optimizers()
        m.modules.train()
        m.on_stage_start(Stage.TRAIN, 1)
        models[name] = m
    batch = PaddedBatch(SyntheticSet(a.B, a.F, a.T, a.T, seed=1).items)
    losses = {}

    def step_of(name):
        m = models[name]

        def step():
            losses[name] = m.fit_batch(batch)
        return step

    warnings.filterwarnings("ignore", message="loss stats logger")
    ms = alternate({name: step_of(name) for name in models}, a.runs, a.steps, warmup=3)
    report(f"{recipe} training step, B={a.B} T={a.T} F={a.F}, fp32 module mode", ms,
           {"steps_per_run": a.steps, "last_loss": {k: float(v) for k, v in losses.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--F", type=int, default=120)
    ap.add_argument("--Z", type=int, default=32)
    ap.add_argument("--N", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20, help="fwd+bwd calls of the stretch per run")
    ap.add_argument("--steps", type=int, default=10, help="training steps per run")
    ap.add_argument("--only", choices=["stretch", "h_vae", "gmm_vae"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/hvae_latent_step.py measures on the device: no HIP device found")
    if a.only in (None, "stretch"):
        stretch(a)
    if a.only in (None, "h_vae"):
        training_step(a, "test_h_vae")
    if a.only in (None, "gmm_vae"):
        training_step(a, "test_gmm_vae")


if __name__ == "__main__":
    main()
