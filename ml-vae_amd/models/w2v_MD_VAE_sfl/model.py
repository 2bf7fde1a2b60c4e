"""The w2v_MD_VAE_sfl recipe (semantics of ref:src/models/w2v_MD_VAE_sfl/model.py:16-158):
MD_VAE_sfl -- the score-function training of the pi network over pi_mcmc_num draws -- on the
features of a frozen wav2vec2 encoder.  The wiring (one encoder pass per batch shared by
phn_recog_in_fc, b_detector_in_fc and w2v_feat_fc, the 1-or-2-frame zero padding, the
un-normalised decoder target, single process) is models/w2v_MD_VAE's; everything after it is
MD_VAE_sfl's forward.  The input is always batch['feat'] + batch['wav']: the reference's w2v
forward has no use_kaldi_feat branch.
"""
from models.MD_VAE.model import Target  # noqa: F401
from models.MD_VAE_sfl.model import SBModel as MD_VAE_sfl
from models.w2v_MD_VAE.model import W2VInputs


class SBModel(W2VInputs, MD_VAE_sfl):
    def _feat_field(self):
        return "feat"
