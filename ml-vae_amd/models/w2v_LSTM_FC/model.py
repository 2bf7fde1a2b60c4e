"""The w2v_LSTM_FC recipe (semantics of ref:src/models/w2v_LSTM_FC/model.py:16-78): wav2vec2
fine-tuned for frame-level mispronunciation detection.  ``wav2vec2(wavs)`` -> ``classifier`` (an
FCBlock 1024 -> 1) -> one logit per frame; BCE-with-logits (no pos_weight) on the frame-level MD
labels under SpeechBrain's compute_masked_loss; ACC / PRE / REC / F1 of round(sigmoid(logits))
against the labels, per utterance at frame level (flvl_md.*), on every stage.

The encoder is modules.wav2vec2.Wav2Vec2 with ``freeze: False, freeze_feature_extractor: True``: the
conv stack stays frozen, everything above it trains through the HIP backward (csrc/w2v.hip), in the
reference's second optimizer group (``wav2vec_opt`` at ``lr_wav2vec``).  The head and the loss are
not the hot path: the classifier is ops.linear, the loss and the scoring are module-mode torch.

Kept from the reference: logits and labels are cut to their common length; logits longer than the
labels raise, in compute_forward (by more than 0 frames) and in compute_objectives (by more than
1); the loss's mask is length_to_mask(feat_lens * min_len) over the cut length while the scored
sequences are cut by undo_padding (round(len * min_len)); torch.round is half-to-even, so a logit of
exactly 0 predicts 0.

Single process: the encoder's two whole-tensor norms couple the utterances of a batch, so
``--distributed_launch`` raises, as in the other w2v recipes.  Needs the spoken corpus
(synthetic: {md_labels: true, waveforms: true}) for ``batch['wav']``."""
import torch
import torch.nn.functional as F

from models.md_model import MDModel
from utils.data_utils import length_to_mask, undo_padding
from utils.metric_stats.md_metric_stats import MDMetricStats


class SBModel(MDModel):
    dp_exact = False

    def on_stage_start(self, stage, epoch=None):
        if self.world_size > 1:
            raise RuntimeError("the w2v_LSTM_FC recipe is single-process: the wav2vec2 encoder's whole-batch "
                               "norms couple the utterances of a batch (run without --distributed_launch)")
        super().on_stage_start(stage, epoch)
        self.stats_loggers["flvl_md_stats"] = MDMetricStats()

    def compute_forward(self, batch, stage):
        batch = batch.to(self.device)
        if "wav" not in batch:
            raise ValueError("w2v_LSTM_FC: the batch has no wav field: the recipe needs the spoken corpus "
                             "(synthetic: {md_labels: true, waveforms: true})")
        wavs = batch["wav"][0]
        feats = self.modules["wav2vec2"](wavs)  # (B, T, 1024)
        logits = self.modules["classifier"](feats.contiguous()).squeeze(dim=-1)  # (B, T)
        labels = batch["flvl_gt_md_lbl_seq"][0]
        if logits.shape[1] - labels.shape[1] > 0:
            raise ValueError(f"Inconsistent sequence lengths: {logits.shape[1]} != {labels.shape[1]}")
        return {"logits": logits}

    def compute_objectives(self, predictions, batch, stage):
        logits = predictions["logits"]
        feat_lens = batch["feat"][1]
        labels = batch["flvl_gt_md_lbl_seq"][0]
        if logits.shape[1] - labels.shape[1] > 1:
            raise ValueError(f"Inconsistent sequence lengths: {logits.shape[1]} != {labels.shape[1]}")
        min_len = min(logits.shape[1], labels.shape[1])
        logits, labels = logits[:, :min_len], labels[:, :min_len]

        # compute_masked_loss: sum(loss * mask) / sum(mask), mask = arange(min_len) < feat_lens * min_len
        targets = labels.to(logits.dtype)
        mask = length_to_mask(feat_lens * min_len, max_len=min_len).to(logits.dtype)
        loss = (F.binary_cross_entropy_with_logits(logits, targets, reduction="none") * mask).sum() / mask.sum()

        pred = torch.round(torch.sigmoid(logits.detach()))
        self.stats_loggers["flvl_md_stats"].append(
            batch["id"], pred_md_lbl_seqs=undo_padding(pred, feat_lens), gt_md_lbl_seqs=undo_padding(labels, feat_lens))
        return loss
