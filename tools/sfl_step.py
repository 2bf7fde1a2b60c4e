"""Timings of the MD_VAE_sfl recipe's hot path on the device, at the recipe's shape
(B = 8, T = 500, F = 80, Z = 32, K = pi_mcmc_num = 5; DESIGN.md, the MD-VAE pi path).

    python tools/sfl_step.py [--runs 5] [--iters 200] [--steps 10]

1. The score-function terms: ops.sfl_losses forward + backward (two fused kernels) against the
   same math written with torch ops on the device (the reference's expression: Categorical, the
   one-hot bmm log-likelihood, .entropy(), F.mse_loss, .mean(-1), one pass per draw).
2. The VAE-target training step (forward, objectives, backward, Adam) of models/MD_VAE_sfl: the
   shipped form, the K draws through the encoder and the decoder once as a batch of K B, against
   a K-loop of B-sized passes.  The loop form exists in this tool only.

Both pairs run on the same build in alternating runs; the medians over the runs and the spread
(min .. max) are printed, one JSON line per measurement.  Times are host clocks around work that
ends in a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ml-vae_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F_  # noqa: E402
from torch.distributions import Categorical  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(forms, runs, iters, warmup):
    """{name: [ms per call, one per run]}: the forms take turns, run after run."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    out = {name: [] for name in forms}
    for _ in range(runs):
        for name, fn in forms.items():
            out[name].append(timed(fn, iters))
    return out


def report(what, ms, extra=None):
    rec = {"measurement": what}
    for name, v in ms.items():
        rec[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                     "max_ms": round(max(v), 4), "runs": len(v)}
    rec.update(extra or {})
    print(json.dumps(rec), flush=True)


# --------------------------------------------------------------------------- 1. the SFL terms
def sfl_terms(a):
    from mlvae_hip import ops
    B, T, F, Z, K = a.B, a.T, a.F, a.Z, a.K
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    logits = r(B, T, 2).requires_grad_(True)
    baseline = r(B, T).requires_grad_(True)
    lab = torch.randint(0, 2, (K, B, T), generator=g).float().cuda()
    draws = torch.stack([1 - lab, lab], dim=-1)
    recon, kld, nll = r(K, B, T, F) ** 2, r(K, B, T, Z) ** 2, r(B, T).abs()
    w = (0.7, 0.3, 0.5)
    d = [r(B, T) for _ in range(3)]

    def finish(out):
        logits.grad = baseline.grad = None
        torch.autograd.backward(out, d)
        return out, (logits.grad, baseline.grad)

    def hip():
        return finish(ops.sfl_losses(logits, draws, recon, kld, nll, baseline, *w))

    def torch_ops():
        dist = Categorical(logits=logits)
        rif = ent = bl = 0
        for k in range(K):
            ll = torch.bmm(dist.logits.reshape(B * T, 1, 2), draws[k].reshape(B * T, 2, 1)).reshape(B, T)
            reward = -(w[0] * recon[k].mean(-1) + w[1] * kld[k].mean(-1) + w[2] * nll)
            rif = rif + (reward - baseline.detach()) * -ll
            ent = ent + -dist.entropy()
            bl = bl + F_.mse_loss(baseline, reward, reduction="none")
        return finish((rif / K, ent / K, bl / K))

    (ho, hg), (to, tg) = hip(), torch_ops()
    err = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip((*ho, *hg), (*to, *tg)))
    ms = alternate({"hip_fused": hip, "torch_ops": torch_ops}, a.runs, a.iters, warmup=20)
    report(f"SFL terms fwd+bwd, B={B} T={T} F={F} Z={Z} K={K}", ms,
           {"max_rel_diff_hip_vs_torch": err, "iters_per_run": a.iters})


# --------------------------------------------------------------------------- 2. the training step
def training_step(a):
    from brain import Stage
    from brain.dataio import PaddedBatch
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import ops
    from models.MD_VAE.model import Target
    from models.MD_VAE_sfl.model import SBModel
    from utils.data_io import SyntheticSet

    ov = ("dataset: synthetic\nmodel_class: MD_VAE_sfl\nmodel_name: sfl_step\n"
          f"batch_size: {a.B}\nmodel: !include:../models/MD_VAE_sfl/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{"model": {"input_size": a.F, "latent_size": a.Z, "pi_mcmc_num": a.K}}, ov])

    class LoopModel(SBModel):
        """The reference's form: K passes of B utterances through the encoder and the decoder."""

        def compute_forward(self, batch, stage):
            predictions, batch, feats, feat_lens, noise = self._upstream(batch)
            rnn_out, pi_logits = self._pi_logits(predictions, feats, "phn_recog_out_fc")
            self._decode_and_nll(predictions, batch, feat_lens, stage)
            losses = predictions["losses"]
            K = self.hparams.pi_mcmc_num
            draws = ops.pi_sample_k(pi_logits, K, True)
            recon, kld = [], []
            for k in range(K):
                enc = self.modules["encoder"](rnn_out, draws[k])
                dec = self.modules["decoder"](enc["sampled_h"], feats)
                recon.append(dec["losses"]["recon_loss"])
                kld.append(enc["losses"]["vae_kld_loss"])
            recon, kld = torch.stack(recon), torch.stack(kld)
            losses["recon_loss"], losses["vae_kld_loss"] = recon.mean(0), kld.mean(0)
            baseline = self.modules["baseline_fc"](rnn_out).squeeze(-1)
            losses["rif_loss"], losses["entropy_loss"], losses["baseline_loss"] = ops.sfl_losses(
                pi_logits, draws, recon, kld, losses["pi_nll_loss"], baseline,
                self.hparams.recon_weight, self.hparams.vae_kld_weight, self.hparams.pi_nll_weight)
            return predictions

    items = SyntheticSet(a.B, a.F, a.T, a.T, seed=1, md_labels=True, n_phonemes=hp["n_phonemes"]).items
    batch = PaddedBatch(items)
    models = {}
    for name, cls in (("batched_KB", SBModel), ("loop_K_x_B", LoopModel)):
        m = cls(modules=hp["model"]["modules"], hparams=hp["model"], run_opts={"device": "cuda:0"})
        m.init_optimizers()
        m.modules.train()
        m.target = Target.VAE
        m.stats_loggers = {}
        models[name] = m
    losses = {}

    def step_of(name):
        m = models[name]

        def step():
            losses[name] = m.fit_batch(batch)
        return step

    import warnings
    warnings.filterwarnings("ignore", message="loss stats logger")
    ms = alternate({name: step_of(name) for name in models}, a.runs, a.steps, warmup=3)
    for m in models.values():
        m.on_stage_end(Stage.TRAIN, 0.0, 1)  # the deferred decode / label error words
    report(f"MD_VAE_sfl VAE-target training step, B={a.B} T={a.T} F={a.F} Z={a.Z} K={a.K}, fp32 module mode",
           ms, {"steps_per_run": a.steps, "last_loss": {k: float(v) for k, v in losses.items()}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--F", type=int, default=80)
    ap.add_argument("--Z", type=int, default=32)
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200, help="SFL-term calls per run")
    ap.add_argument("--steps", type=int, default=10, help="training steps per run")
    ap.add_argument("--only", choices=["terms", "step"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sfl_step.py measures on the device: no HIP device found")
    if a.only != "step":
        sfl_terms(a)
    if a.only != "terms":
        training_step(a)


if __name__ == "__main__":
    main()
