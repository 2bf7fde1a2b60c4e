"""The test_h_vae recipe (semantics of ref:src/models/test_h_vae/model.py:13-66): the Hierarchical
VAE trained and inspected alone.  The normaliser; modules['rnn'] (the reference yaml's
unidirectional torch.nn.LSTM 2x512, here modules.lstm.LSTM on the HIP recurrence);
modules['pi_fc'] -> pi_logits; sampled_pi = ops.pi_sample (a Categorical draw in TRAIN, the argmax
otherwise); modules['encoder'] (HierarchicalVAE) on (rnn_out, sampled_pi); the decoder.  Losses: the
masked means of vae_kld_loss and recon_loss; vae_kld_weight gets the '_kld' rule of
models/md_model.py (divided by 2249 / batch_size).

Two things of the reference, decided:
* pi_fc receives no gradient: the sample is not differentiable and nothing else reads the logits.
  Its parameters keep ``grad is None`` and come through fit_batch bit-unchanged (the optimizer and
  the clip skip parameters without gradient).
* The reference's checkpointer lists encoder, decoder and epoch_counter only, so its test.py
  evaluates with a freshly initialised rnn.  Our model.yaml lists rnn and pi_fc as well, after the
  reference's three: a recovered model is the trained one.

``fused_latent`` (the yaml passes it to the encoder as ``fused``): the encoder's latent stretch is
one kernel each way (csrc/hvae.hip), with the same draws under the same torch seed.

``self.noise`` (tests): None, or a dict with any of pi_u [B, T], eps_v, eps_g, expo -- the draws
injected instead of the library's Philox streams.
Module mode; data parallel through models/md_model.py's shard-exact step."""
from mlvae_hip import ops
from models.md_model import MDModel
from utils.data_utils import apply_lens_to_loss


class SBModel(MDModel):
    dp_exact = True
    noise = None

    def compute_forward(self, batch, stage):
        batch = batch.to(self.device)
        feats, feat_lens = batch["feat"]
        feats = self.hparams.normalizer(feats, feat_lens, epoch=self.hparams.epoch_counter.current)
        feats = feats.contiguous()
        noise = self.noise or {}
        rnn_out = self.modules["rnn"](feats)[0]           # (B, T, C)
        pi_logits = self.modules["pi_fc"](rnn_out)        # (B, T, 2)
        sampled_pi = ops.pi_sample(pi_logits, self.modules.training, u=noise.get("pi_u"))
        encoder_out = self.modules["encoder"](rnn_out, sampled_pi, eps_v=noise.get("eps_v"),
                                              eps_g=noise.get("eps_g"), expo=noise.get("expo"))
        decoder_out = self.modules["decoder"](encoder_out["sampled_h"], feats)
        return {"pi_logits": pi_logits, "sampled_pi": sampled_pi, "encoder_out": encoder_out,
                "decoder_out": decoder_out}

    def compute_objectives(self, predictions, batch, stage):
        feat_lens = batch["feat"][1]
        original_losses = dict(predictions["encoder_out"]["losses"])
        original_losses["recon_loss"] = predictions["decoder_out"]["losses"]["recon_loss"]
        losses = {key: apply_lens_to_loss(value, feat_lens) for key, value in original_losses.items()}
        return self.compute_and_save_losses(losses)
