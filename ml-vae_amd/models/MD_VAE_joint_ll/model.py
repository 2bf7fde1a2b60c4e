"""The MD_VAE_joint_ll recipe (semantics of ref:src/models/MD_VAE_joint_ll/model.py:22-185):
MD_VAE_joint's forward with the upstream losses detached, plus pi_nll_loss in every forward.

The phoneme recogniser and the boundary detector run under torch.no_grad(): their losses are
logged and weighted into the total as the reference's detached values, and their parameters get
no gradient (.grad stays None; the optimizer and the clip skip them).  The Viterbi MD decode runs
inside every forward, TRAIN included, and pi_nll_loss (weight 0.001) is ops.pi_nll on the frame
labels the decode left on the device; its error word is read at the stage's end, or where the host
lists are materialised (evaluation).  Evaluation runs in every VALID and in TEST; there is no
save_md_result.

``pair_upstream`` and ``self.noise``: as MD_VAE_joint's.
"""
from brain import Stage
from models.MD_VAE_joint.model import SBModel as MD_VAE_joint


class SBModel(MD_VAE_joint):
    upstream_grad = False
    saves_md_result = False

    def to_run_evaluation(self, stage):
        return stage == Stage.VALID or stage == Stage.TEST

    def _evaluated(self, stage, epoch=None):
        return self.to_run_evaluation(stage)

    def _forward_decode(self, predictions, batch, feat_lens, stage):
        self._decode_and_nll(predictions, batch, feat_lens, stage)
