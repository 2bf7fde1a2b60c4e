"""The w2v_CRDNN_CTC recipe (semantics of ref:src/models/w2v_CRDNN_CTC/model.py:7-24): CRDNN_CTC on
the features of a wav2vec2 encoder that trains with it, conv feature extractor included.
``wav2vec2(wavs)`` [B, T_w, 1024] goes to ``crdnn`` and ``output`` under the log-softmax; there is no
normaliser.  Everything else is CRDNN_CTC's (models/CRDNN_CTC/model.py): the CTC loss on the
pronounced phonemes, the device evaluation path on every stage, and the Viterbi boundaries on the
log-posteriors resampled from their own frames (T_w, or T_w // 2 after time pooling) to the features'
frames by resample_frames; the relative lengths are the features'.

``crdnn`` is modules.crdnn.CRDNN in the yaml (the LSTM stack and the DNN).  The reference's CNN block(s)
and time pooling (modules.crdnn.ConvCRDNN) cannot sit on a trained encoder yet: the Conv2d family's
Cin = 1 first layer (csrc/conv2d.hip) has no input gradient, and raises on an input that requires one.

The encoder is modules.wav2vec2.Wav2Vec2 with ``freeze: False, train_feature_extractor: True`` -- what
SpeechBrain 0.5.x trains under the reference's ``freeze: False`` -- in the reference's second optimizer
group (``wav2vec_opt`` over ``wav2vec2`` at ``lr_wav2vec``; ``adam_opt`` over ``crdnn`` and ``output``).

Single process: the encoder's two whole-tensor norms couple the utterances of a batch, so
``--distributed_launch`` raises, as in the other w2v recipes.  Needs the spoken corpus (synthetic:
{md_labels: true, waveforms: true}) for ``batch['wav']`` and the phoneme sequences."""
from mlvae_hip import ops
from models.CRDNN_CTC.model import SBModel as CRDNN_CTC


def w2v_forward(self, batch, stage):
    """compute_forward of both w2v_CRDNN_CTC recipes."""
    name = type(self).__module__.split(".")[1]
    batch = batch.to(self.device)
    for key in ("wav", "gt_phn_seq", "gt_cnncl_seq", "gt_boundary_seq"):
        if key not in batch:
            raise ValueError(f"{name}: the batch has no {key}: the recipe needs the spoken corpus "
                             "(synthetic: {md_labels: true, waveforms: true})")
    wavs = batch["wav"][0]
    feats = self.modules["wav2vec2"](wavs)  # (B, T_w, 1024)
    out = self.modules["crdnn"](feats.contiguous())
    out = self.modules["output"](out)
    frames, lens = batch["feat"]
    return {"pout": ops.log_softmax(out), "pout_lens": lens, "feat_frames": frames.shape[1]}


def single_process(self):
    if self.world_size > 1:
        name = type(self).__module__.split(".")[1]
        raise RuntimeError(f"the {name} recipe is single-process: the wav2vec2 encoder's whole-batch norms couple "
                           "the utterances of a batch (run without --distributed_launch)")


class SBModel(CRDNN_CTC):
    def on_stage_start(self, stage, epoch=None):
        single_process(self)
        super().on_stage_start(stage, epoch)

    def compute_forward(self, batch, stage):
        return w2v_forward(self, batch, stage)
