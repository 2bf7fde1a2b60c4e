"""The CRDNN_CTC recipe (semantics of ref:src/models/CRDNN_CTC/model.py:22-176): the supervised
recogniser baseline.  A CRDNN (modules/crdnn.py: a bidirectional LSTM stack and a DNN; with
model_cnn.yaml the lobe's CNN front end and time pooling before them, ConvCRDNN) and a
Linear to ``output_neurons`` classes under a log-softmax, trained by CTC on the pronounced
phonemes (gt_phn_seq); on every batch of every stage the greedy decode is aligned by edit
distance to the pronounced and to the canonical sequence (phn_per / cnncl_per), every position
where the aligned prediction differs from the canonical phoneme is called a mispronunciation
(plvl_md.*, with correct_per / misp_per), and a Viterbi pass of the CTC chain over the canonical
sequence gives the phoneme boundaries (boundary.*, and the soft plvl_md scores).  With time pooling
the log-posteriors have T // 2 frames: the relative lengths carry over (the kernels take them
against pout's own frames), and for the Viterbi pass pout is first resampled to the features'
frames as the reference's resample_tensor does (resample_frames below).

Kept from the reference: the normaliser is applied; the loss is F.ctc_loss(reduction='mean',
zero_infinity=True) on the log-posteriors (the mean over the batch of nll_i / U_i), blank =
``blank_index``; the stats keys; TEST writes test_output/md_result_seqs.txt.

What differs: log-softmax, CTC loss with its gradient, greedy decode, both alignments, the MD /
PER counts, Viterbi and the boundary counts are HIP kernels (ops.log_softmax, ctc_nll,
ctc_greedy_decode, edit_align, ctc_md_counts, ctc_viterbi, boundary_counts); their outputs stay
on the device until the stage's scores are summarised -- no host read per batch (the reference
runs SpeechBrain's decoder, its edit distance and the ctc_segmentation package per utterance on
the host on every batch, TRAIN included).  The boundaries are the Viterbi path's, not the
ctc_segmentation package's (which is not available here): a stated departure.  An utterance
whose frames cannot hold its chain is counted (``infeasible``), not raised -- until the soft MD
scores need its boundaries at the stage's end.  Adam replaces Adadelta + NewBob, as in LSTM_FC.
The recipe needs gt_phn_seq: the spoken synthetic corpus (synthetic: {md_labels: true, waveforms:
true}).  Module mode, single process (dp_exact stays False)."""
import logging
from pathlib import Path

import torch

from brain import Stage
from mlvae_hip import ops
from models.md_model import MDModel
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
from utils.metric_stats.error_rate_stats import ErrorRateStats
from utils.metric_stats.md_metric_stats import MDMetricStats

logger = logging.getLogger(__name__)


def resample_frames(pout, T):
    """pout [B, T', C] on T frames, as the reference's resample_tensor (ref:src/utils/data_utils.py:107-156):
    every frame repeated T // T' times, then cut or zero-padded to T (a difference of more than 3
    frames raises).  T' == T: pout itself."""
    Tp = pout.shape[1]
    if Tp == T:
        return pout
    factor = T // Tp
    if factor < 1:
        raise ValueError(f"resample_frames: non-positive factor for lengths {Tp} and {T}")
    out = torch.repeat_interleave(pout, factor, dim=1)
    diff = out.shape[1] - T
    if abs(diff) > 3:
        raise ValueError(f"resample_frames: {Tp} frames x {factor} differ from {T} by {diff} (> 3)")
    if diff > 0:
        out = out[:, :T]
    elif diff < 0:
        out = torch.cat([out, out.new_zeros(out.shape[0], -diff, out.shape[2])], dim=1)
    return out.contiguous()


class SBModel(MDModel):
    _eval_ran = False
    infeasible = None  # device int32 scalar: the stage's utterances without a Viterbi path

    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        self.stats_loggers["phn_per_stats"] = ErrorRateStats()
        self.stats_loggers["cnncl_per_stats"] = ErrorRateStats()
        self.stats_loggers["plvl_md_stats"] = MDMetricStats()
        self.stats_loggers["boundary_stats"] = BoundaryMetricStats()
        self._eval_ran = False
        self.infeasible = None

    def on_stage_end(self, stage, stage_loss, epoch=None):
        if self._eval_ran:  # the stage's data-error bits, read where the counts are
            self._eval_ran = False
            ops.raise_ctc_eval_err()
            n_inf = int(self.infeasible)  # read with the stage's counts
            if n_inf:
                logger.warning("%s stage, epoch %s: %d utterance(s) too short for the CTC chain of their "
                               "canonical sequence", stage.name, epoch, n_inf)
        super().on_stage_end(stage, stage_loss, epoch)
        if stage == Stage.TEST and self.rank == 0:
            out = Path(self.hparams.output_dir) / "test_output"
            self.stats_loggers["plvl_md_stats"].write_seqs_to_file(out / "md_result_seqs.txt")

    def _blank(self):
        return int(self.hparams.blank_index)

    def compute_forward(self, batch, stage):
        for key in ("gt_phn_seq", "gt_cnncl_seq", "gt_boundary_seq"):
            if key not in batch:
                raise ValueError(f"CRDNN_CTC: the batch has no {key}: the recipe needs the spoken corpus "
                                 "(synthetic: {md_labels: true, waveforms: true})")
        feats, feat_lens = self._normalised_feats(batch, stage)
        out = self.modules["crdnn"](feats)
        out = self.modules["output"](out)
        return {"pout": ops.log_softmax(out), "pout_lens": feat_lens, "feat_frames": feats.shape[1]}

    def _targets(self, batch, key):
        seqs, lens = batch[key]
        return seqs.to(self.device), lens.to(self.device)

    def compute_loss(self, predictions, batch):
        return self._ctc_loss(predictions, batch, "gt_phn_seq")

    def _ctc_loss(self, predictions, batch, key):
        """F.ctc_loss(reduction='mean', zero_infinity=True) against the sequences batch[key]."""
        phns, phn_lens = self._targets(batch, key)
        nll = ops.ctc_nll(predictions["pout"], predictions["pout_lens"], phns, phn_lens, 1, self._blank())
        n_tgt = torch.round(phns.shape[1] * phn_lens.to(torch.float32)).clamp(min=1.0)
        return (nll / n_tgt).mean()

    def compute_objectives(self, predictions, batch, stage):
        loss = self.compute_loss(predictions, batch)
        with torch.no_grad():
            pout, lens = predictions["pout"].detach(), predictions["pout_lens"]
            ids = batch["id"]
            bi = getattr(batch, "global_index", None)
            phns, phn_lens = self._targets(batch, "gt_phn_seq")
            cnncls, cnncl_lens = self._targets(batch, "gt_cnncl_seq")
            gt_boundary = batch["gt_boundary_seq"][0].to(self.device)

            pred, pred_len = ops.ctc_greedy_decode(pout, lens, self._blank())
            ali, edits = ops.edit_align(pred, pred_len, phns, phn_lens, cnncls, cnncl_lens)
            counts = ops.ctc_md_counts(ali, phns, phn_lens, cnncls, cnncl_lens)
            # the boundaries are scored on the features' frames: a time-pooled pout is resampled first
            pout_t = resample_frames(pout, predictions.get("feat_frames", pout.shape[1]))
            _, boundary, infeasible = ops.ctc_viterbi(pout_t, lens, cnncls, cnncl_lens, self._blank())
            self._eval_ran = True
            n_inf = infeasible.sum()
            self.infeasible = n_inf if self.infeasible is None else self.infeasible + n_inf

            self.stats_loggers["phn_per_stats"].append_counts(ids, edits[:, 0], batch_index=bi)
            self.stats_loggers["cnncl_per_stats"].append_counts(ids, edits[:, 1], batch_index=bi)
            self.stats_loggers["plvl_md_stats"].append_aligned(
                ids, counts, ali[:, 0], phns, cnncls, pred_boundary=boundary, gt_boundary=gt_boundary,
                batch_index=bi)
            self.stats_loggers["boundary_stats"].append_counts(
                ids, ops.boundary_counts(boundary, gt_boundary, lens), batch_index=bi)
        return loss
