"""HMMAligner on the HIP lattice kernels (csrc/align.hip): the call surface of
speechbrain.alignment.aligner.HMMAligner that the HMM_DNN_ALI recipe uses
(ref:src/models/HMM_DNN_ALI/model.py:58-89, model.yaml:53-57).

A left-to-right HMM with ``states_per_phoneme`` states per phoneme, every allowed transition
(stay, next) at log-weight 0; the emission class of state j of phoneme p is p * spp + j.

``__call__`` takes the EXPANDED ids, as the recipe passes them: phns [B, L * spp] from
``expand_phns_by_states_per_phoneme``, each id one state class, with the phonemes' relative
lengths (U_i = round(L * spp * phn_lens_i)).  The reductions: score_i / T_i with
``input_len_norm``, / U_i with ``target_len_norm``, then ``batch_reduction`` (mean, sum, none) --
applied to the forward and the Viterbi scores alike.  SpeechBrain is not vendored: these
semantics are restated from its documented interface, not pinned against it.
Its lexicon, pronunciation-variant and silence-insertion paths are not part of this build.
"""
import torch
from torch import nn

from mlvae_hip import ops


class HMMAligner(nn.Module):
    def __init__(self, states_per_phoneme=1, batch_reduction="none", input_len_norm=False,
                 target_len_norm=False):
        super().__init__()
        if int(states_per_phoneme) < 1:
            raise ValueError(f"HMMAligner: states_per_phoneme must be >= 1, got {states_per_phoneme}")
        if batch_reduction not in ("none", "mean", "sum"):
            raise ValueError(f"HMMAligner: batch_reduction must be none, mean or sum, got {batch_reduction!r}")
        self.states_per_phoneme = int(states_per_phoneme)
        self.batch_reduction = batch_reduction
        self.input_len_norm = bool(input_len_norm)
        self.target_len_norm = bool(target_len_norm)
        self.align_dict = {}

    def expand_phns_by_states_per_phoneme(self, phns, phn_lens):
        """[B, L] phoneme ids -> [B, L * spp] state classes id * spp + j (padding expands too)."""
        spp = self.states_per_phoneme
        j = torch.arange(spp, device=phns.device, dtype=phns.dtype)
        return (phns.unsqueeze(-1) * spp + j).reshape(phns.shape[0], -1)

    def _reduce(self, score, T, lens, U, phn_lens):
        if self.input_len_norm:
            score = score / torch.round(T * lens.to(score.device, torch.float32)).clamp(min=1.0)
        if self.target_len_norm:
            score = score / torch.round(U * phn_lens.to(score.device, torch.float32)).clamp(min=1.0)
        if self.batch_reduction == "mean":
            return score.mean()
        if self.batch_reduction == "sum":
            return score.sum()
        return score

    def forward(self, pout, lens, phns, phn_lens, dp_algorithm):
        """pout [B, T, C] log-probabilities, phns [B, U] expanded state classes.
        'forward': the reduced forward score (autograd).  'viterbi': (reduced Viterbi score,
        alignments int32 [B, T]: the state position per frame, -1 past the utterance)."""
        T, U = pout.shape[1], phns.shape[1]
        if dp_algorithm == "forward":
            score = ops.hmm_forward(pout, lens, phns, phn_lens, 1)
            return self._reduce(score, T, lens, U, phn_lens)
        if dp_algorithm == "viterbi":
            vscore, align = ops.hmm_viterbi(pout, lens, phns, phn_lens, 1)
            return self._reduce(vscore, T, lens, U, phn_lens), align
        raise ValueError(f"HMMAligner: dp_algorithm must be 'forward' or 'viterbi', got {dp_algorithm!r}")

    def store_alignments(self, ids, alignments):
        """Keep each utterance's alignment row (a device tensor) under its id."""
        for i, utt in enumerate(ids):
            self.align_dict[utt] = alignments[i]
