"""The HMM_DNN_ALI recipe (semantics of ref:src/models/HMM_DNN_ALI/model.py:16-91): the forced
aligner.  A frame DNN (VanillaNN, Linear) whose centred log-posteriors drive a left-to-right HMM
with ``states_per_phoneme`` states per phoneme; trained on the forward score (or CTC), aligned
with Viterbi on every batch of every stage, scored by frame accuracy against gt_phn_end_seq
(accuracy.average).

Kept from the reference: the forward VanillaNN -> Linear -> (out - out.mean(1)) -> log-softmax,
the mean over all frames of the padded batch; the normaliser is carried by the yaml and NOT
applied (the reference tests ``hasattr(hparams, 'normalize')``, which its yaml never satisfies);
the training type is reset to ``init_training_type`` at every stage start
(``switch_training_type`` is carried and unused, as there); the alignments are stored in the
aligner when training on 'forward'.

What differs: the centring and log-softmax, the forward score with its occupancy gradient, the
CTC loss, Viterbi and the accuracy counts are HIP kernels (ops.center_log_softmax, hmm_forward,
ctc_nll, hmm_viterbi, align_counts); the counts and the data-error word stay on the device until
the stage's scores are summarised -- no host read per batch (the reference scores per utterance
on the host on every batch).  'ctc' is F.ctc_loss(reduction='mean', zero_infinity=True) with
blank = blank_index: the mean over the batch of nll_i / U_i.  'viterbi' training raises
NotImplementedError.  TEST also writes test_output/alignments.json: per utterance id the start
frame of every phoneme of the Viterbi alignment -- the aligner's product, what another recipe
reads as fa_boundary_seq.  Module mode, single process (dp_exact stays False)."""
import json
from pathlib import Path

import torch

from brain import Stage
from mlvae_hip import ops
from models.md_model import MDModel
from utils.metric_stats.align_acc_metric_stats import AlignAccMetricStats


class SBModel(MDModel):
    _lattice_ran = False
    _starts = ()

    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        self.training_type = self.hparams.init_training_type
        self.stats_loggers["accuracy_stats"] = AlignAccMetricStats()
        self._lattice_ran = False
        self._starts = []  # TEST: (ids, [B, 1 + L] device rows: L_i, then the phoneme start frames)

    def on_stage_end(self, stage, stage_loss, epoch=None):
        if self._lattice_ran:  # the stage's data-error bits, read where the counts are
            self._lattice_ran = False
            ops.raise_align_err()
        if stage == Stage.TEST and self.rank == 0 and self._starts:
            self._write_alignments()
        super().on_stage_end(stage, stage_loss, epoch)

    def compute_forward(self, batch, stage):
        batch = batch.to(self.device)
        feats, feat_lens = batch["feat"]
        # the yaml's normalizer is carried, not applied (see the module docstring)
        out = self.modules["model"](feats.contiguous())
        out = self.modules["output"](out)
        return ops.center_log_softmax(out), feat_lens

    def compute_objectives(self, predictions, batch, stage):
        pout, pout_lens = predictions
        ids = batch["id"]
        phns_orig, phn_lens = batch["gt_cnncl_seq"]
        phn_ends = batch["gt_phn_end_seq"][0]
        aligner = self.hparams.aligner
        spp = aligner.states_per_phoneme
        phns_orig, phn_lens = phns_orig.to(self.device), phn_lens.to(self.device)
        phns = aligner.expand_phns_by_states_per_phoneme(phns_orig, phn_lens)

        if self.training_type == "forward":
            loss = -aligner(pout, pout_lens, phns, phn_lens, "forward")
        elif self.training_type == "ctc":
            nll = ops.ctc_nll(pout, pout_lens, phns, phn_lens, 1, self.hparams.blank_index)
            n_tgt = torch.round(phns.shape[1] * phn_lens.to(torch.float32)).clamp(min=1.0)
            loss = (nll / n_tgt).mean()
        elif self.training_type == "viterbi":
            raise NotImplementedError("HMM_DNN_ALI: 'viterbi' training needs SpeechBrain's flat-start "
                                      "alignments and nll_loss over padding, which are not pinned here")
        else:
            raise ValueError(f"HMM_DNN_ALI: training type {self.training_type!r}")

        with torch.no_grad():
            _, alignments = aligner(pout.detach(), pout_lens, phns, phn_lens, "viterbi")
            self._lattice_ran = True
            if self.training_type in ("viterbi", "forward"):
                aligner.store_alignments(ids, alignments)
            counts = ops.align_counts(alignments, pout_lens, phns_orig, phn_lens, spp, phn_ends,
                                      self.hparams.samples_per_frame)
            self.stats_loggers["accuracy_stats"].append_counts(
                ids, counts, batch_index=getattr(batch, "global_index", None))
            if stage == Stage.TEST:
                self._starts.append((list(ids), self._phoneme_starts(alignments, phns_orig, phn_lens, spp)))
        return loss

    @staticmethod
    def _phoneme_starts(alignments, phns_orig, phn_lens, spp):
        """int32 [B, 1 + L] on the device: L_i, then the first frame of every phoneme (-1: none)."""
        L = phns_orig.shape[1]
        phone = torch.div(alignments, spp, rounding_mode="floor")  # -1 stays -1
        hit = phone.unsqueeze(-1) == torch.arange(L, device=phone.device, dtype=phone.dtype)
        first = torch.where(hit.any(1), hit.to(torch.int32).argmax(1), -1).to(torch.int32)
        n = torch.round(L * phn_lens.to(torch.float32)).to(torch.int32)
        return torch.cat([n.unsqueeze(1), first], dim=1)

    def _write_alignments(self):
        width = max(rows.shape[1] for _, rows in self._starts)
        rows = torch.cat([torch.nn.functional.pad(r, (0, width - r.shape[1]), value=-1)
                          for _, r in self._starts]).cpu().tolist()  # the stage's one read
        utts = [u for ids, _ in self._starts for u in ids]
        out = Path(self.hparams.output_dir) / "test_output"
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "alignments.json", "w") as f:
            json.dump({u: r[1:1 + r[0]] for u, r in zip(utts, rows)}, f)
        self._starts = []
