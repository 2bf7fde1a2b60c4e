"""The bits of the device error words and what each raises on the host: the Python side of
include/mlvae_err.h (tests/test_err_bits.py compares the two).  Pure: no tensor is touched here.

One int32 word per device (_core._md_err) is OR-ed into by the md, pi, frame-level-head, scoring,
lattice and CTC-evaluation kernels; each reader domain below owns a mask of it and clears that mask
alone.  The decode kernels write the same enum's bits into a word of the caller's, the CMVN kernels
have an enum and a word of their own.  (The recurrences' hand-off word is a third word, value 1.)"""

ERR = {  # enum MlvaeErr: MLVAE_ERR_<name>
    "MD_SEGMENTS": 2, "MD_CLASS": 4,
    "DECODE_BACKTRACK": 8, "DECODE_EMPTY": 16,
    "PI_LABEL": 32,
    "FLVL_LABEL": 64,
    "SCORE_SEGMENTS": 128, "SCORE_K": 256,
    "ALIGN_SHORT": 512, "ALIGN_CLASS": 1024, "ALIGN_BLANK": 2048,
    "CTC_PAIR": 4096,
}
CMVN_ERR = {"SPEAKER": 1, "NO_STATS": 2}  # enum MlvaeCmvnErr: MLVAE_CMVN_ERR_<name>

PI_ERR_LABEL = ERR["PI_LABEL"]              # a decoded frame label outside {-1, 0, 1}
FLVL_ERR_LABEL = ERR["FLVL_LABEL"]          # a valid frame's MD label is neither 0 nor 1
SCORE_ERR_SEGMENTS = ERR["SCORE_SEGMENTS"]  # the flags do not give L_i segments from frame 0
SCORE_ERR_K = ERR["SCORE_K"]                # more boundaries asked for than frames (k > T_i)
ALIGN_ERR_SHORT = ERR["ALIGN_SHORT"]        # HMM chain infeasible (T_i < U_i, U_i = 0 or T_i = 0)
ALIGN_ERR_CLASS = ERR["ALIGN_CLASS"]        # a phoneme id whose state class is outside [0, C)
ALIGN_ERR_BLANK = ERR["ALIGN_BLANK"]        # CTC, a target class equal to blank
CTC_ERR_PAIR = ERR["CTC_PAIR"]              # pronounced and canonical sequences differ in length

# A reader domain: its bits in reading order, each with the exception class and the phrase it
# contributes.  The message is head + sep.join(phrases of the set bits) + tail (every=False: the
# first set bit's phrase alone), the class that of the first set bit; %(who)s is the caller's name,
# %(code)d the whole word.
DOMAINS = {
    "md": dict(
        head="phoneme-recogniser targets: ", sep="", tail=" (ref:src/modules/phoneme_recognizer.py:65-67)", every=True,
        bits=((ERR["MD_SEGMENTS"], AssertionError, "boundaries do not give one segment per phoneme from frame 0 "),
              (ERR["MD_CLASS"], AssertionError, "phoneme id outside [0, n_phonemes + 2)"))),
    "pi": dict(
        head="", sep="", tail="", every=True,
        bits=((ERR["PI_LABEL"], ValueError, "pi_nll: frame label outside {0, 1} (-1 = past the utterance's end) "
                                            "(ref:src/models/MD_VAE/model.py:149)"),)),
    "flvl": dict(
        head="", sep="", tail="", every=True,
        bits=((ERR["FLVL_LABEL"], ValueError, "flvl_md_head: frame-level MD label outside {0, 1} in a valid frame "
                                              "(Only binary input values are supported)"),)),
    "score": dict(  # AssertionError as plvl_phn_acc_scoring's asserts, RuntimeError as torch.topk's
        head="", sep="", tail="", every=False,
        bits=((ERR["SCORE_SEGMENTS"], AssertionError,
               "phn_acc_counts: boundary_seqs do not give one segment per phoneme from frame 0 "
               "(ref:src/utils/metric_stats/phn_acc_metric_stats.py:69-73)"),
              (ERR["SCORE_K"], RuntimeError,
               "boundary_topk: k out of range: fa_boundary_seqs has more boundaries than "
               "the utterance has frames (ref:src/models/test_b_ind_classifier/model.py:61)"))),
    "align": dict(
        head="sequence lattice: ", sep="; ", tail="", every=True,
        bits=((ERR["ALIGN_SHORT"], AssertionError,
               "an utterance has fewer frames than HMM states (or no states, or no frames)"),
              (ERR["ALIGN_CLASS"], AssertionError, "a phoneme id expands to a state class outside [0, C)"),
              (ERR["ALIGN_BLANK"], AssertionError, "a CTC target class equals the blank index"))),
    "ctc_eval": dict(
        head="CTC evaluation: ", sep="; ", tail="", every=True,
        bits=((ERR["ALIGN_CLASS"], AssertionError, "a phoneme id is outside [0, C)"),
              (ERR["ALIGN_BLANK"], AssertionError, "a target phoneme equals the blank index"),
              (ERR["CTC_PAIR"], AssertionError, "gt_phn_seq and gt_cnncl_seq of an utterance differ in length"))),
    "decode": dict(  # the decode's own word: one message for either bit
        head="MD decode: backtrack did not end at (0, 0) / empty utterance (err %(code)d)", sep="", tail="",
        every=True,
        bits=((ERR["DECODE_BACKTRACK"], AssertionError, ""), (ERR["DECODE_EMPTY"], AssertionError, ""))),
    "cmvn": dict(  # the CMVN kernels' own word
        head="%(who)s: ", sep="", tail="", every=False,
        bits=((CMVN_ERR["SPEAKER"], ValueError, "speaker id outside [0, S)"),
              (CMVN_ERR["NO_STATS"], ValueError, "a speaker of the batch has no accumulated statistics"))),
}


def mask(domain):
    """The bits of its word that the domain reads and clears."""
    m = 0
    for bit, _, _ in DOMAINS[domain]["bits"]:
        m |= bit
    return m


def read(code, domain, who=None):
    """(exception to raise or None, bits to clear) for the word's integer value `code` as the
    domain's reader sees it: a word without a bit of the domain gives (None, 0)."""
    d = DOMAINS[domain]
    hit = [(cls, phrase) for bit, cls, phrase in d["bits"] if code & bit]
    if not hit:
        return None, 0
    phrases = [p for _, p in hit] if d["every"] else [hit[0][1]]
    text = (d["head"] + d["sep"].join(phrases) + d["tail"]) % {"who": who, "code": code}
    return hit[0][0](text), mask(domain)
