"""The test_b_ind_classifier recipe (semantics of ref:src/models/test_b_ind_classifier/
model.py:17-74): the MD-VAE's boundary detector trained and inspected alone.  The normaliser, then
modules['boundary_detector'] against fa_boundary_seq; the predicted boundaries of an utterance are
the k frames with the largest boundary_v, k = the boundaries of its fa_boundary_seq; they are
scored against gt_boundary_seq (boundary.f1 / boundary.r_value), on every stage.

The reference unpads boundary_v, runs torch.topk per utterance and walks two Python lists per
utterance, on every batch, TRAIN included.  Here ops.boundary_topk and ops.boundary_counts leave
three integers per utterance on the device and the stats object reads them once per stage: no
host sync per batch at all.  torch.topk's error for k > T_i becomes a bit of the device error
word, read in on_stage_end.

One thing not kept from the reference: its compute_objectives sums the module's *unreduced* [B, T]
losses (the module's masked means were commented out later), and backward() on that raises.  The
meaning built is its siblings': loss = sum_k weight_k * apply_lens_to_loss(loss_k, feat_lens) over
the module's keys in order (bce, then kld), weight_k = hparams.<key>_weight, 1 when absent -- this
recipe's own rule: no warning, no '_kld' division, no loss stats.
Module mode; data parallel through models/md_model.py's shard-exact step."""
from mlvae_hip import ops
from models.md_model import MDModel
from utils.data_utils import apply_lens_to_loss
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats


class SBModel(MDModel):
    dp_exact = True
    noise = None       # {"boundary_u": [10, B, T]} injects the detector's uniform draws (parity tests)
    _scored = False

    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        self.stats_loggers["boundary_stats"] = BoundaryMetricStats()
        self._scored = False

    def on_stage_end(self, stage, stage_loss, epoch=None):
        if self._scored:  # the stage's top-k error bit, read where the counts are
            self._scored = False
            ops.raise_score_err()
        super().on_stage_end(stage, stage_loss, epoch)

    def compute_forward(self, batch, stage):
        batch = batch.to(self.device)
        feats, feat_lens = batch["feat"]
        fa_boundary_seqs = batch["fa_boundary_seq"][0]
        feats = self.hparams.normalizer(feats, feat_lens, epoch=self.hparams.epoch_counter.current)
        return self.modules["boundary_detector"](feats.contiguous(), feat_lens, fa_boundary_seqs,
                                                 uniform_u=(self.noise or {}).get("boundary_u"))

    def compute_objectives(self, predictions, batch, stage):
        feat_lens = batch["feat"][1]
        loss = 0
        for key, value in predictions["losses"].items():
            weight = getattr(self.hparams, key.replace("_loss", "_weight"), 1)
            loss = loss + weight * apply_lens_to_loss(value, feat_lens)
        pred = ops.boundary_topk(predictions["boundary_v"], feat_lens, batch["fa_boundary_seq"][0])
        counts = ops.boundary_counts(pred, batch["gt_boundary_seq"][0], feat_lens)
        self._scored = True
        predictions["pred_boundary_seq"] = pred
        self.stats_loggers["boundary_stats"].append_counts(
            batch["id"], counts, batch_index=getattr(batch, "global_index", None))
        return loss
