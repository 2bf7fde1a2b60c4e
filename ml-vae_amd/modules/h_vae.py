"""HierarchicalVAE on libmlvae (replaces ref:src/modules/h_vae.py:12-72).

A VanillaVAE (correct pronunciation) and a GMMVAE (mispronunciation) read the same frames; the
GMM outputs are collapsed over components with their hard mixture weights, both branches are
stacked on a new axis and mixed by pi (B, T, 2).  Every weighting is the apply_weight kernel.

fused=True: the two FC stacks and head GEMMs run as they do, and one ops.hvae_latent call
(csrc/hvae.hip) does the rest -- both reparameterisations and KLs, the Gumbel-softmax, the
collapse and the mix -- forward and backward.  torch's RNG is read in the composed path's order
(eps_v, eps_g, the Gumbel seed), so the same torch.manual_seed gives the same draws either way.
"""
import torch
from torch import nn

from mlvae_hip import ops
from modules.gmm_vae import GMMVAE, TAU
from modules.vanilla_vae import VanillaVAE
from utils.data_utils import apply_weight


class HierarchicalVAE(nn.Module):
    def __init__(self, fc_sizes, latent_size, num_components, fused=False):
        super().__init__()
        self.vanilla_vae = VanillaVAE(fc_sizes, latent_size)
        self.gmm_vae = GMMVAE(fc_sizes, latent_size, num_components)
        self.fused = bool(fused)

    def forward(self, feats, pi, eps_v=None, eps_g=None, expo=None):
        if self.fused:
            return self._forward_fused(feats, pi, eps_v, eps_g, expo)
        v = self.vanilla_vae(feats, eps=eps_v)
        g = self.gmm_vae(feats, eps=eps_g, expo=expo)
        w = g["gmm_weight"]  # (B, T, N)
        out = {}
        for key in ("mean", "log_var", "sampled_h", "loss"):
            pair = torch.stack([v[key], apply_weight(g[key], w)], dim=2)  # (B, T, 2, C)
            out[key] = apply_weight(pair, pi)  # (B, T, C)
        return {
            "gmm_weight": w,
            "mean": out["mean"],
            "log_var": out["log_var"],
            "sampled_h": out["sampled_h"],
            "losses": {"vae_kld_loss": out["loss"]},
        }

    def _forward_fused(self, feats, pi, eps_v, eps_g, expo):
        vae, gmm = self.vanilla_vae, self.gmm_vae
        ml = vae.mean_logvar(feats)
        if eps_v is None:
            eps_v = ops.randn(ml.shape[:-1] + (vae.latent_size,))
        P = gmm.stacked_heads(feats)
        eps_g, seed = gmm.draws(P, eps_g, expo)
        mean, log_var, h, kl, w = ops.hvae_latent(ml, P, pi, eps_v, eps_g, expo, gmm.num_components,
                                                  gmm.latent_size, TAU, seed)
        return {
            "gmm_weight": w,
            "mean": mean,
            "log_var": log_var,
            "sampled_h": h,
            "losses": {"vae_kld_loss": kl},
        }
