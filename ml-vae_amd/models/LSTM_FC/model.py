"""The LSTM_FC recipe (semantics of ref:src/models/LSTM_FC/model.py:16-69): the supervised MD
baseline.  A unidirectional LSTM over the frames, an FCBlock down to two classes, a class-weighted
BCE-with-logits on the frame-level MD labels (pos_weight = [1, misp_weight] against the targets
[1 - label, label]) under SpeechBrain's compute_masked_loss, and ACC / PRE / REC / F1 of the
argmax against the labels, per utterance at frame level (flvl_md.*), on every stage.

The FCBlock's layers but the last run through ops.linear; the last layer, the loss per frame and
class, the argmax and the per-utterance MD counts are one kernel (ops.flvl_md_head), and the
counts stay on the device until the stage's scores are summarised: no host lists and no sync per
batch (the reference makes 2 B Python lists per batch, TRAIN included).

Two things kept from the reference: compute_forward does not apply the normaliser (the yaml
carries and checkpoints one), and in TRAIN the batch is read under its aug_ names -- when the
batch has them; the synthetic corpus has no augmentation, as the reference's pipeline yields the
plain fields under the aug_ names when none is configured (ref:src/utils/data_io.py:204-207).
The reference's append(...) passes argument names its scoring function does not take and raises
at the first batch; the meaning implemented is its sibling w2v_LSTM_FC's (pred_md_lbl_seqs /
gt_md_lbl_seqs).  The counts follow the loss's length mask (frame t valid iff t < len T in fp32).
Module mode; data parallel through models/md_model.py's shard-exact step."""
from torch import nn

from brain import Stage
from mlvae_hip import ops
from models.md_model import MDModel
from utils.metric_stats.md_metric_stats import MDMetricStats


class SBModel(MDModel):
    dp_exact = True
    _head_ran = False

    def _dp_lens_field(self, batch, stage):
        return self._fields(batch, stage)[0]

    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        self.stats_loggers["flvl_md_stats"] = MDMetricStats()
        self._head_ran = False

    def on_stage_end(self, stage, stage_loss, epoch=None):
        if self._head_ran:  # the stage's label error bit, read where the counts are
            self._head_ran = False
            ops.raise_flvl_err()
        super().on_stage_end(stage, stage_loss, epoch)

    @staticmethod
    def _fields(batch, stage):
        """(feat, labels) field names: TRAIN reads the augmented ones when the batch has them."""
        if stage == Stage.TRAIN and "aug_feat" in batch and "aug_flvl_gt_md_lbl_seq" in batch:
            return "aug_feat", "aug_flvl_gt_md_lbl_seq"
        return "feat", "flvl_gt_md_lbl_seq"

    def compute_forward(self, batch, stage):
        batch = batch.to(self.device)
        feat_key, lbl_key = self._fields(batch, stage)
        feats, feat_lens = batch[feat_key]
        labels = batch[lbl_key][0]

        out = self.modules["lstm"](feats.contiguous())[0]
        plan = self.modules["fc"].linear_plan()
        for lin, act in plan[:-1]:
            out = ops.linear(out, lin.weight, lin.bias, act)
        last, act = plan[-1]
        if act or not isinstance(last, nn.Linear) or last.out_features != 2 or last.bias is None:
            raise ValueError("LSTM_FC: fc must end in a Linear to 2 classes with a bias and no activation")
        logits, loss_e, pred, counts = ops.flvl_md_head(
            out, last.weight, last.bias, labels, feat_lens, (1.0, self.hparams.misp_weight))
        self._head_ran = True
        return {"out": logits, "loss_e": loss_e, "flvl_pred_md_lbl_seq": pred, "flvl_md_counts": counts}

    def compute_objectives(self, predictions, batch, stage):
        feat_key, _ = self._fields(batch, stage)
        feat_lens = batch[feat_key][1]
        # compute_masked_loss: sum(loss * mask) / sum(mask), the length mask over both classes
        loss = ops.masked_mean(predictions["loss_e"], feat_lens)
        self.stats_loggers["flvl_md_stats"].append_counts(
            batch["id"], predictions["flvl_md_counts"], batch_index=getattr(batch, "global_index", None))
        return loss
