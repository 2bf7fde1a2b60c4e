"""The w2v_MD_VAE recipe (semantics of ref:src/models/w2v_MD_VAE/model.py:16-129): MD_VAE on the
features of a frozen wav2vec2 encoder (modules/wav2vec2.py) instead of the Fbank frames.

What changes against MD_VAE, as the reference wires it:

* ``w2v_feats = wav2vec2(batch['wav'])`` [B, T_w, wav2vec2_size], once per batch and shared by
  the three consumers; T_w is 1 or 2 frames short of ``feat``'s T (the encoder's receptive field
  is 400 samples at a hop of 320) and is zero-padded up to it -- any other difference raises;
* ``phn_recog_in_fc(w2v_feats)`` feeds the phoneme recogniser, ``b_detector_in_fc(w2v_feats)`` the
  boundary detector, ``w2v_feat_fc(w2v_feats)`` replaces ``feat_fc`` in the pi path;
* the decoder's target stays ``batch['feat']`` as it is: the reference's w2v forward never calls
  the normaliser, so it is not applied here either.

The encoder is frozen (forward only, no_grad): the reference's ``wav2vec_opt`` optimizer group has
no trainable parameter and is dropped.  Single process: the encoder's two whole-tensor norms
(normalize_wav, output_norm) couple the utterances of a batch, so a rank's shard would not see
what the single process sees; ``--distributed_launch`` raises.  The recipe needs the spoken corpus
(synthetic: {md_labels: true, waveforms: true}) for ``batch['wav']``.
"""
import torch

from models.MD_VAE.model import SBModel as MD_VAE
from models.MD_VAE.model import Target  # noqa: F401  (the recipe surface of MD_VAE)


def pad_to_frames(w2v_feats, T):
    """w2v_feats [B, T_w, C] zero-padded along time to T frames; T - T_w must be 0, 1 or 2
    (ref:src/models/w2v_MD_VAE/model.py:26-32)."""
    diff = T - w2v_feats.shape[1]
    if not 0 <= diff <= 2:
        raise ValueError(f"w2v_MD_VAE: the encoder gave {w2v_feats.shape[1]} frames for {T} feature frames "
                         f"(shape_diff = {-diff}; it may be 1 or 2 frames short, nothing else)")
    if diff:
        w2v_feats = torch.nn.functional.pad(w2v_feats, (0, 0, 0, diff))
    return w2v_feats


class W2VInputs:
    """The wav2vec2 wiring over MD_VAE's input hooks (mixed in before MD_VAE / MD_VAE_sfl)."""
    dp_exact = False
    _w2v_feats = None

    def on_stage_start(self, stage, epoch=None):
        if self.world_size > 1:
            raise RuntimeError("the w2v_MD_VAE recipes are single-process: the wav2vec2 encoder's whole-batch "
                               "norms couple the utterances of a batch (run without --distributed_launch)")
        super().on_stage_start(stage, epoch)

    def _input_feats(self, batch):
        """(batch['feat'] as it is -- the decoder's target, no normaliser --, its lengths); runs the
        encoder once and keeps its padded features for the three consumers."""
        if "wav" not in batch:
            raise ValueError("w2v_MD_VAE: the batch has no wav field: the recipe needs the spoken corpus "
                             "(synthetic: {md_labels: true, waveforms: true})")
        feats, feat_lens = batch["feat"]
        wavs = batch["wav"][0]
        self._w2v_feats = pad_to_frames(self.modules["wav2vec2"](wavs), feats.shape[1])  # (B, T, C)
        return feats, feat_lens

    def _recog_input(self, feats):
        return self.modules["phn_recog_in_fc"](self._w2v_feats)

    def _detector_input(self, feats):
        return self.modules["b_detector_in_fc"](self._w2v_feats)

    def _pi_feats(self, feats):
        return self.modules["w2v_feat_fc"](self._w2v_feats)


class SBModel(W2VInputs, MD_VAE):
    _phn_out_fc = "phn_recog_out_fc"
