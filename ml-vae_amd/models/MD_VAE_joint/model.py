"""The MD_VAE_joint recipe (semantics of ref:src/models/MD_VAE_joint/model.py:23-182): the MD-VAE's
modules trained jointly.  There is no target cycle: every training step runs the phoneme
recogniser and the boundary detector with autograd and their losses attached, then
phn_recog_out.detach() -> phn_recog_fc, concat_fc, rnn, pi_fc, ops.pi_sample, the H-VAE encoder
and the decoder, and sums phn_recog_bce_loss, boundary_bce_loss, boundary_kld_loss, vae_kld_loss
and recon_loss through compute_and_save_losses.  The forward holds no decode and no pi_nll_loss
(pi_fc gets no gradient); the Viterbi MD decode runs in compute_objectives of evaluated stages only.

Evaluated stages: TEST, and VALID of every tenth epoch.  Loss stats, the MD and boundary metrics,
on_stage_end, the train_log lines and the checkpoint (max_key plvl_md.F1) exist only there, so a
checkpoint is written at VALID of epochs 10, 20, ...

Deviation from the reference: it calls save_md_result in every stage, which raises KeyError
outside evaluated stages (no decoded sequences there), i.e. on the first training batch.  Here the
results are saved in TEST only, as the MD_VAE recipe does.

``pair_upstream`` (hparams): the recogniser's and the detector's LSTMs have the same shape, read
the same feats and do not depend on each other; when set, and ops.lstm_pair_ok holds, both run as
one paired recurrence launch per layer (ops.lstm_pair) and the modules receive the outputs as
rnn_out.  Otherwise each module runs its own.  The pair draws nothing, so the data-parallel shard
contract (models/md_model.py) holds without change.

``self.noise`` (tests): as MD_VAE's.
"""
import contextlib

import torch

from brain import Stage
from mlvae_hip import ops
from models.MD_VAE.model import SBModel as MD_VAE
from models.md_model import MDModel
from utils.data_utils import apply_lens_to_loss, undo_padding
from utils.decode_utils import decode_md_device
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
from utils.metric_stats.md_metric_stats import MDMetricStats


class SBModel(MD_VAE):
    upstream_grad = True    # the recogniser and the detector train in this step
    saves_md_result = True  # TEST writes datasets/<dataset_name>/saved_md_results/<model_name>.json

    # ------------------------------------------------------------------ stages
    def on_stage_start(self, stage, epoch=None):
        MDModel.on_stage_start(self, stage, epoch)  # the loss stats
        if stage not in (Stage.TRAIN, Stage.VALID, Stage.TEST):
            raise ValueError(f"invalid stage {stage}")
        self._decode_err = None
        self._md_results = []
        if self._evaluated(stage, epoch):
            self.stats_loggers["plvl_md_stats"] = MDMetricStats()
            self.stats_loggers["boundary_stats"] = BoundaryMetricStats()
        else:
            self.stats_loggers = {}

    def to_run_evaluation(self, stage, epoch):
        if stage == Stage.TRAIN:
            return False
        if stage == Stage.TEST:
            return True
        if epoch is None:
            raise ValueError("epoch cannot be None")
        return epoch % 10 == 0

    def _evaluated(self, stage, epoch=None):
        """to_run_evaluation at the running epoch (the hooks that receive none)."""
        if epoch is None and stage == Stage.VALID:
            epoch = self.hparams.epoch_counter.current
        return self.to_run_evaluation(stage, epoch)

    def on_stage_end(self, stage, stage_loss, epoch=None):
        self._raise_device_errors()
        if stage == Stage.TEST and self._dp():
            self._gather_md_results()
        if self._evaluated(stage, epoch):
            MDModel.on_stage_end(self, stage, stage_loss, epoch)

    def _gather_md_results(self):
        import torch.distributed as tdist
        parts = [None] * self.world_size
        tdist.all_gather_object(parts, self._md_results)
        if self.rank == 0:  # one writer, in the single-process order (batch, rank)
            results = {}
            for _, _, res in sorted(((b, r, res) for r, part in enumerate(parts) for b, res in part),
                                    key=lambda x: x[:2]):
                results.update(res)
            self._write_md_results(results)

    # ------------------------------------------------------------------ forward
    def _upstream(self, batch):
        """Normaliser, phoneme recogniser and boundary detector, both in every step:
        (predictions, batch on the device, feats, feat_lens, the injected noise)."""
        noise = self.noise or {}
        batch = batch.to(self.device)
        feats, feat_lens = batch["feat"]
        predictions = {"losses": {}}
        feats = self.hparams.normalizer(feats, feat_lens, epoch=self.hparams.epoch_counter.current)
        feats = feats.contiguous()
        recog, detector = self.modules["phoneme_recognizer"], self.modules["boundary_detector"]
        seqs, seq_lens = batch["gt_cnncl_seq"]
        fa_boundary_seqs = batch["fa_boundary_seq"][0]
        # modules whose losses the reference detaches run without autograd (as MD_VAE's do)
        with (contextlib.nullcontext() if self.upstream_grad else torch.no_grad()):
            out_a = out_b = None
            if getattr(self.hparams, "pair_upstream", False) and \
                    ops.lstm_pair_ok(recog.rnn, detector.rnn, self.modules.training):
                out_a, out_b = ops.lstm_pair(feats, recog.rnn, detector.rnn, self.modules.training)
            phn = recog(feats, feat_lens, seqs, seq_lens, fa_boundary_seqs, rnn_out=out_a)
            bnd = detector(feats, feat_lens, fa_boundary_seqs, uniform_u=noise.get("boundary_u"),
                           rnn_out=out_b)
        predictions["phn_recog_out"] = phn["out"]
        predictions["losses"].update(phn["losses"])
        predictions["boundary_v"] = bnd["boundary_v"]
        predictions["losses"].update(bnd["losses"])
        return predictions, batch, feats, feat_lens, noise

    def compute_forward(self, batch, stage):
        predictions, batch, feats, feat_lens, noise = self._upstream(batch)
        rnn_out, pi_logits = self._pi_logits(predictions, feats, "phn_recog_fc")
        sampled_pi = ops.pi_sample(pi_logits, self.modules.training, u=noise.get("pi_u"))
        predictions["sampled_pi"] = sampled_pi
        self._forward_decode(predictions, batch, feat_lens, stage)
        enc = self.modules["encoder"](rnn_out, sampled_pi, eps_v=noise.get("eps_v"),
                                      eps_g=noise.get("eps_g"), expo=noise.get("expo"))
        predictions["losses"].update(enc["losses"])
        dec = self.modules["decoder"](enc["sampled_h"], feats)
        predictions["losses"].update(dec["losses"])
        return predictions

    def _forward_decode(self, predictions, batch, feat_lens, stage):
        """The joint recipe's forward holds no decode (MD_VAE_joint_ll's does)."""

    def _decode(self, predictions, batch, feat_lens):
        """The Viterbi MD decode of an evaluated batch, as the reference's host lists."""
        seqs, seq_lens = batch["gt_cnncl_seq"]
        decoded = decode_md_device(predictions, feat_lens, seqs, seq_lens, prior=batch["prior"][0][0],
                                   weight=getattr(self.hparams, "dec_weight", 1.0),
                                   skip_empty=self._dp())  # a short rank slice's fillers
        predictions["decoded_device"] = decoded
        err = decoded[4]
        self._decode_err = err if self._decode_err is None else self._decode_err | err
        return self._decoded_lists(predictions)

    # ------------------------------------------------------------------ objectives
    def compute_objectives(self, predictions, batch, stage):
        feats, feat_lens = batch["feat"]
        losses = {key: apply_lens_to_loss(value, feat_lens)
                  for key, value in predictions["losses"].items()}
        loss = self.compute_and_save_losses(losses)

        if self._evaluated(stage):
            if "decoded_device" in predictions:  # the forward's decode, not run again
                boundary_seqs, _, plvl_md_lbl_seqs = self._decoded_lists(predictions)
            else:
                boundary_seqs, _, plvl_md_lbl_seqs = self._decode(predictions, batch, feat_lens)
            gt_md_lbl_seqs = undo_padding(*batch["plvl_gt_md_lbl_seq"])
            gt_boundary_seqs = undo_padding(*batch["gt_boundary_seq"])
            bi = getattr(batch, "global_index", None)
            self.stats_loggers["plvl_md_stats"].append(
                ids=batch["id"], batch_index=bi, pred_md_lbl_seqs=plvl_md_lbl_seqs, gt_md_lbl_seqs=gt_md_lbl_seqs,
                pred_boundary_seqs=boundary_seqs, gt_boundary_seqs=gt_boundary_seqs)
            self.stats_loggers["boundary_stats"].append(
                ids=batch["id"], batch_index=bi, predictions=boundary_seqs, targets=gt_boundary_seqs)

        if stage == Stage.TEST and self.saves_md_result:
            self.save_md_result(batch, predictions)
        return loss
