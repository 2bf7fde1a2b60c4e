"""The w2v_CRDNN_CTC_cnncl recipe (semantics of ref:src/models/w2v_CRDNN_CTC_cnncl/model.py:15-68):
CRDNN_CTC_cnncl -- the CTC loss against the canonical phonemes -- on the features of a wav2vec2 encoder
that trains with it (models/w2v_CRDNN_CTC/model.py has the forward and the encoder's settings).

Kept from the reference: at TEST the log-posteriors of every utterance, cut to the utterance's frames
and resampled to its feature frames (the reference's resample_tensor: each frame repeated, then cut
or zero-padded; resample_frames), are collected and written to ``<output_dir>/saved_phn_recog_outs.pt``
as {utterance id: tensor [feature frames, classes]} on the CPU; an existing file is merged, with a
warning for every id it already holds.  What reads that file in the reference (MD_VAE_sfl_saved_phn_recog)
is not built here."""
import warnings
from pathlib import Path

import torch

from brain import Stage
from models.CRDNN_CTC.model import resample_frames
from models.CRDNN_CTC_cnncl.model import SBModel as CRDNN_CTC_cnncl
from models.w2v_CRDNN_CTC.model import single_process, w2v_forward


def frames_of(rel, T):
    """undo_padding's length of a relative length at T padded frames."""
    return int(torch.round(rel * T))


class SBModel(CRDNN_CTC_cnncl):
    def on_stage_start(self, stage, epoch=None):
        single_process(self)
        super().on_stage_start(stage, epoch)
        if stage == Stage.TEST:
            self.saved_pouts = {}

    def compute_forward(self, batch, stage):
        predictions = w2v_forward(self, batch, stage)
        if stage == Stage.TEST:
            pout = predictions["pout"].detach()
            rel = batch["feat"][1].cpu()
            for i, utt in enumerate(batch["id"]):
                own = pout[i:i + 1, :frames_of(rel[i], pout.shape[1])]
                self.saved_pouts[utt] = resample_frames(own, frames_of(rel[i], predictions["feat_frames"]))[0].cpu()
        return predictions

    def on_stage_end(self, stage, stage_loss, epoch=None):
        super().on_stage_end(stage, stage_loss, epoch)
        if stage == Stage.TEST and self.rank == 0:
            path = Path(self.hparams.output_dir) / "saved_phn_recog_outs.pt"
            saved = torch.load(path) if path.exists() else {}
            for key in self.saved_pouts:
                if key in saved:
                    warnings.warn(f"duplicate key {key}")
            saved.update(self.saved_pouts)
            torch.save(saved, path)
