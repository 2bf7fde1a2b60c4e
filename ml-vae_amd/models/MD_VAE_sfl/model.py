"""The MD_VAE_sfl recipe (semantics of ref:src/models/MD_VAE_sfl/model.py:24-189): MD-VAE whose
pi network also learns from the reconstruction and the KL, through a score-function (REINFORCE)
estimator.  The draw that picks the H-VAE branch is not differentiable, so per frame

    reward        = -(recon_weight mean_F(recon) + vae_kld_weight mean_Z(kld) + pi_nll_weight pi_nll)
    rif_loss      = (reward - baseline) * -log_prob(draw)       (reward and baseline detached)
    entropy_loss  = -entropy(Categorical(pi_logits))
    baseline_loss = (baseline_fc(rnn_out) - reward)^2            (gradient into rnn_out too)

averaged over K = pi_mcmc_num draws in train (Categorical draws) and K = 1 in eval (the argmax);
recon_loss and vae_kld_loss are the means over the draws.  The reward's weights are the raw
hparams (no 2249 / batch_size scaling of the KL weight: that applies to the total only).
Targets, the no_grad treatment of the untrained upstream modules, the device decode, pi_nll_loss
(once per step, from the decode's labels) and the deferred error word are MD_VAE's.

The K draws share rnn_out, so they go through the encoder and the decoder once as a batch of
K B utterances (the reference loops K times over B): the recurrences are latency-bound at small
B.  Dropout and the eps streams are keyed by global element index, so every one of the K B rows
has its own noise, as K independent passes have in distribution.  The score-function terms are
one fused kernel each way (ops.sfl_losses).

``self.noise`` (tests): as MD_VAE's, with pi_u [K,B,T] and eps_v, eps_g, expo with a leading K.
``use_kaldi_feat: true`` (the reference's MD_VAE_sfl default; here an override, as the yaml's key
set is the recipe's without it): the input is batch['kaldi_feat'] and the normaliser is not run.

Data parallel (models/md_model.py's shard-exact step): the K B fold runs under the shard context's
folded(K) variant, so row k B_l + b draws what the single process draws at row k B_g + b_g.
"""
import contextlib

from mlvae_hip import ops
from models.MD_VAE.model import SBModel as MD_VAE
from models.MD_VAE.model import Target


class SBModel(MD_VAE):
    def _use_kaldi_feat(self):
        return getattr(self.hparams, "use_kaldi_feat", False) is True

    def _feat_field(self):
        return "kaldi_feat" if self._use_kaldi_feat() else "feat"

    def _input_feats(self, batch):
        """use_kaldi_feat (ref:src/models/MD_VAE_sfl/model.py:59-63): the corpus's already
        normalised `kaldi_feat`, the normaliser not called; else `feat` through the normaliser."""
        if not self._use_kaldi_feat():
            return super()._input_feats(batch)
        if "kaldi_feat" not in batch:
            raise ValueError("use_kaldi_feat: the batch has no kaldi_feat field; build the corpus with "
                             "synthetic: {kaldi_feats: true} (with waveforms: true), or point "
                             "prepare.dataset_dir at a computed dataset that holds it")
        return batch["kaldi_feat"]

    def compute_forward(self, batch, stage):
        predictions, batch, feats, feat_lens, noise = self._upstream(batch)
        if self.target in (Target.VAE, Target.TEST):
            hp = self.hparams
            train = self.modules.training
            rnn_out, pi_logits = self._pi_logits(predictions, feats, "phn_recog_out_fc")
            self._decode_and_nll(predictions, batch, feat_lens, stage)
            losses = predictions["losses"]

            K = hp.pi_mcmc_num if train else 1
            draws = ops.pi_sample_k(pi_logits, K, train, u=noise.get("pi_u"))  # (K, B, T, 2)
            predictions["sampled_pi_draws"] = draws
            predictions["sampled_pi"] = draws[-1, ..., 1]  # the last draw's labels (B, T)

            # the K draws as one batch of K B utterances
            B, T = pi_logits.shape[:2]
            fold = lambda t: None if t is None else t.reshape(K * B, T, t.shape[-1])
            sh = ops.current_shard()
            with (sh.folded(K) if sh is not None else contextlib.nullcontext()):
                enc = self.modules["encoder"](rnn_out.repeat(K, 1, 1), fold(draws),
                                              eps_v=fold(noise.get("eps_v")), eps_g=fold(noise.get("eps_g")),
                                              expo=fold(noise.get("expo")))
                dec = self.modules["decoder"](enc["sampled_h"], feats.repeat(K, 1, 1))
            recon = dec["losses"]["recon_loss"].view(K, B, T, -1)
            kld = enc["losses"]["vae_kld_loss"].view(K, B, T, -1)
            losses["recon_loss"] = recon.mean(0)
            losses["vae_kld_loss"] = kld.mean(0)

            baseline = self.modules["baseline_fc"](rnn_out).squeeze(-1)  # (B, T)
            predictions["baseline"] = baseline
            losses["rif_loss"], losses["entropy_loss"], losses["baseline_loss"] = ops.sfl_losses(
                pi_logits, draws, recon, kld, losses["pi_nll_loss"], baseline,
                hp.recon_weight, hp.vae_kld_weight, hp.pi_nll_weight)
        return predictions
