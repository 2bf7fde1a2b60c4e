"""The test_gmm_vae recipe (semantics of ref:src/models/test_gmm_vae/model.py:17-65): the GMM-VAE
encoder trained and inspected alone.  The normaliser, then modules['encoder'] (GMMVAE), its
per-component sampled_h collapsed by the hard mixture weights (apply_weight) into the decoder's
input; kld_loss is the masked mean of the per-component KL collapsed the same way, recon_loss the
decoder's.  kld_weight has no '_kld' substring: it is not rescaled by the corpus size.

``fused_latent`` (hparams): the collapsed sampled_h and KL come from GMMVAE.collapsed -- one
kernel each way (csrc/hvae.hip's GMM-only mode) instead of gmm_latent + two apply_weight -- with
the same draws under the same torch seed.  Off: the composed path, as the reference writes it.

``self.noise`` (tests): None, or {"eps": [B, T, N Z], "expo": [B, T, N]}, the draws injected into
the encoder instead of the library's Philox streams.
Module mode; data parallel through models/md_model.py's shard-exact step."""
from models.md_model import MDModel
from utils.data_utils import apply_lens_to_loss, apply_weight
from utils.metric_stats.loss_metric_stats import LossMetricStats


class SBModel(MDModel):
    dp_exact = True
    noise = None

    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        self.stats_loggers["kld_loss_stats"] = LossMetricStats("kld_loss")
        self.stats_loggers["recon_loss_stats"] = LossMetricStats("recon_loss")

    def compute_forward(self, batch, stage):
        batch = batch.to(self.device)
        feats, feat_lens = batch["feat"]
        feats = self.hparams.normalizer(feats, feat_lens, epoch=self.hparams.epoch_counter.current)
        feats = feats.contiguous()
        noise = self.noise or {}
        encoder = self.modules["encoder"]
        if getattr(self.hparams, "fused_latent", False):
            encoder_out = encoder.collapsed(feats, eps=noise.get("eps"), expo=noise.get("expo"))
            weighted_h = encoder_out["weighted_h"]
        else:
            encoder_out = encoder(feats, eps=noise.get("eps"), expo=noise.get("expo"))
            weighted_h = apply_weight(encoder_out["sampled_h"], encoder_out["gmm_weight"])
        decoder_out = self.modules["decoder"](weighted_h, feats)
        return {"encoder_out": encoder_out, "decoder_out": decoder_out}

    def compute_objectives(self, predictions, batch, stage):
        encoder_out = predictions["encoder_out"]
        feat_lens = batch["feat"][1]
        if "weighted_loss" in encoder_out:
            kld_loss = encoder_out["weighted_loss"]
        else:
            kld_loss = apply_weight(encoder_out["loss"], encoder_out["gmm_weight"])
        losses = {
            "kld_loss": apply_lens_to_loss(kld_loss, feat_lens),
            "recon_loss": apply_lens_to_loss(predictions["decoder_out"]["losses"]["recon_loss"], feat_lens),
        }
        return self.compute_and_save_losses(losses)
