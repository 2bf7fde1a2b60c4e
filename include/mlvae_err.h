/* The bits of libmlvae's device error words: the one definition, included by include/mlvae.h
 * (the ABI's prose refers to these names) and by csrc/common.h (the kernels OR them in).
 * mlvae_hip/ops/errors.py holds the same values with the exception each bit raises;
 * tests/test_err_bits.py compares the two.  A new bit takes the next free value of its word. */
#ifndef MLVAE_ERR_H
#define MLVAE_ERR_H

/* The shared word (the *err of the MD, decode, pi, frame-level-head, scoring, lattice and CTC
 * evaluation entry points).  Kernels OR bits in; each reader clears its own domain's bits alone.
 * (The decode kernels take a word of the caller's, OR-ed across a stage's batches on the device.) */
enum MlvaeErr {
  MLVAE_ERR_MD_SEGMENTS = 2,         /* md.hip: the boundaries do not give one segment per phoneme from frame 0 */
  MLVAE_ERR_MD_CLASS = 4,            /* md.hip: a phoneme id outside [0, C) */
  MLVAE_ERR_DECODE_BACKTRACK = 8,    /* decode.hip: the backtrack did not end at (l, t) = (0, 0) */
  MLVAE_ERR_DECODE_EMPTY = 16,       /* decode.hip: an empty or oversized utterance */
  MLVAE_ERR_PI_LABEL = 32,           /* pi.hip: a decoded frame label outside {-1, 0, 1} */
  MLVAE_ERR_FLVL_LABEL = 64,         /* flvl.hip: a valid frame's label is neither 0 nor 1 */
  MLVAE_ERR_SCORE_SEGMENTS = 128,    /* score.hip: the flags do not give L_b segments from frame 0 */
  MLVAE_ERR_SCORE_K = 256,           /* score.hip: more boundaries asked for than frames (k_b > T_b) */
  MLVAE_ERR_ALIGN_SHORT = 512,       /* align.hip: HMM chain infeasible (T_b < U_b, U_b = 0 or T_b = 0) */
  MLVAE_ERR_ALIGN_CLASS = 1024,      /* align.hip, ctc_eval.hip: a phoneme id whose class is outside [0, C) */
  MLVAE_ERR_ALIGN_BLANK = 2048,      /* align.hip, ctc_eval.hip: CTC, a target class equal to blank */
  MLVAE_ERR_CTC_PAIR = 4096          /* ctc_eval.hip: pronounced and canonical sequences differ in length */
};

/* The CMVN kernels' own word (kaldi_fbank.hip: mlvae_cmvn_accumulate / mlvae_cmvn_apply). */
enum MlvaeCmvnErr {
  MLVAE_CMVN_ERR_SPEAKER = 1,        /* a speaker id outside [0, S) */
  MLVAE_CMVN_ERR_NO_STATS = 2        /* a speaker of the batch has no accumulated statistics */
};

/* The persistent recurrences' hand-off word (the err of the mlvae_lstm* entry points) is a word of
 * its own and takes the single value 1: a hand-off timed out. */

#endif
