"""The test_phn_classifier recipe (semantics of ref:src/models/test_phn_classifier/model.py:17-64):
the MD-VAE's phoneme recogniser trained and inspected alone.  The normaliser, then
modules['phoneme_recognizer'] on the canonical phonemes expanded by fa_boundary_seq; the loss is
the length-masked mean of its BCE (no weights, no loss stats, as the reference); the scores are
the frame- and phoneme-level accuracy of the output against flvl_gt_cnncl_seq and gt_cnncl_seq
over the gt_boundary_seq segments (phn_acc.flvl_acc / phn_acc.plvl_acc), on every stage.

The reference unpads the batch into 4 B host tensors per batch and scores them in Python, TRAIN
included.  Here one kernel (ops.phn_acc_counts) leaves four integers per utterance on the device
and the stats object reads them once per stage; the reference's asserts on the boundary flags
become a bit of the device error word, read in on_stage_end.  ops.phn_bce keeps its own per-batch
read of its two error bits (the module's asserts): that is unchanged here.
Module mode; data parallel through models/md_model.py's shard-exact step."""
from mlvae_hip import ops
from models.md_model import MDModel
from utils.data_utils import apply_lens_to_loss
from utils.metric_stats.phn_acc_metric_stats import PhnAccMetricStats


class SBModel(MDModel):
    dp_exact = True
    _scored = False

    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        self.stats_loggers["phn_acc_stats"] = PhnAccMetricStats()
        self._scored = False

    def on_stage_end(self, stage, stage_loss, epoch=None):
        if self._scored:  # the stage's segment error bit, read where the counts are
            self._scored = False
            ops.raise_score_err()
        super().on_stage_end(stage, stage_loss, epoch)

    def compute_forward(self, batch, stage):
        batch = batch.to(self.device)
        feats, feat_lens = batch["feat"]
        seqs, seq_lens = batch["gt_cnncl_seq"]
        boundary_seqs = batch["fa_boundary_seq"][0]
        feats = self.hparams.normalizer(feats, feat_lens, epoch=self.hparams.epoch_counter.current)
        return self.modules["phoneme_recognizer"](feats.contiguous(), feat_lens, seqs, seq_lens,
                                                  boundary_seqs)

    def compute_objectives(self, predictions, batch, stage):
        feat_lens = batch["feat"][1]
        loss = apply_lens_to_loss(predictions["losses"]["phn_recog_bce_loss"], feat_lens)
        seqs, seq_lens = batch["gt_cnncl_seq"]
        counts = ops.phn_acc_counts(predictions["out"], feat_lens, batch["flvl_gt_cnncl_seq"][0],
                                    seqs, seq_lens, batch["gt_boundary_seq"][0])
        self._scored = True
        self.stats_loggers["phn_acc_stats"].append_counts(
            batch["id"], counts, batch_index=getattr(batch, "global_index", None))
        return loss
