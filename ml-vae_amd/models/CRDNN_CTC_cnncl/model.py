"""The CRDNN_CTC_cnncl recipe (semantics of ref:src/models/CRDNN_CTC_cnncl/model.py:16-44):
CRDNN_CTC whose CTC loss is taken against the canonical phonemes (gt_cnncl_seq) instead of the
pronounced ones -- the recogniser never sees a mispronunciation labelled.  Forward, decode,
alignments, Viterbi boundaries and every score are CRDNN_CTC's (models/CRDNN_CTC/model.py); the
yaml logs plvl_md.{ACC,PRE,REC,F1} only, as the reference's."""
from models.CRDNN_CTC.model import SBModel as CRDNN_CTC


class SBModel(CRDNN_CTC):
    def compute_loss(self, predictions, batch):
        return self._ctc_loss(predictions, batch, "gt_cnncl_seq")
