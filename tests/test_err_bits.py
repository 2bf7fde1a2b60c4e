"""The device error words' bits have one definition on each side -- include/mlvae_err.h for the
kernels, mlvae_hip/ops/errors.py for the readers -- and the two agree; the pure reader
(errors.read) gives, for every combination of a domain's bits, the exception class and the wording
the per-domain readers had before they shared it (the expectations below are written out from
those readers), and clears the domain's bits alone.  CPU only: no tensor, no library call."""
import itertools
import os
import re

import pytest

from conftest import PKG, ROOT
from mlvae_hip.ops import errors

SHARED_DOMAINS = ("md", "pi", "flvl", "score", "align", "ctc_eval")
FOREIGN = 1 << 20  # a bit no domain owns: every reader must leave it


def _enum(name):
    text = open(os.path.join(ROOT, "include", "mlvae_err.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # the comments first: they use braces too
    body = re.search(r"enum\s+%s\s*\{(.*?)\}" % name, text, re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"\b([A-Z0-9_]+)\s*=\s*(\d+)", body)}


def test_header_and_table_hold_the_same_values():
    shared, cmvn = _enum("MlvaeErr"), _enum("MlvaeCmvnErr")
    assert shared == {"MLVAE_ERR_" + k: v for k, v in errors.ERR.items()}
    assert cmvn == {"MLVAE_CMVN_ERR_" + k: v for k, v in errors.CMVN_ERR.items()}
    assert shared == {
        "MLVAE_ERR_MD_SEGMENTS": 2, "MLVAE_ERR_MD_CLASS": 4, "MLVAE_ERR_DECODE_BACKTRACK": 8,
        "MLVAE_ERR_DECODE_EMPTY": 16, "MLVAE_ERR_PI_LABEL": 32, "MLVAE_ERR_FLVL_LABEL": 64,
        "MLVAE_ERR_SCORE_SEGMENTS": 128, "MLVAE_ERR_SCORE_K": 256, "MLVAE_ERR_ALIGN_SHORT": 512,
        "MLVAE_ERR_ALIGN_CLASS": 1024, "MLVAE_ERR_ALIGN_BLANK": 2048, "MLVAE_ERR_CTC_PAIR": 4096}
    assert cmvn == {"MLVAE_CMVN_ERR_SPEAKER": 1, "MLVAE_CMVN_ERR_NO_STATS": 2}


def test_no_two_names_of_a_word_share_a_bit():
    for word in (_enum("MlvaeErr"), _enum("MlvaeCmvnErr"), errors.ERR, errors.CMVN_ERR):
        values = list(word.values())
        assert all(v > 0 and v & (v - 1) == 0 for v in values), word  # single bits
        assert len(set(values)) == len(values), word


def test_the_named_constants_come_from_the_table():
    assert (errors.PI_ERR_LABEL, errors.FLVL_ERR_LABEL, errors.SCORE_ERR_SEGMENTS, errors.SCORE_ERR_K,
            errors.ALIGN_ERR_SHORT, errors.ALIGN_ERR_CLASS, errors.ALIGN_ERR_BLANK, errors.CTC_ERR_PAIR) == \
        (32, 64, 128, 256, 512, 1024, 2048, 4096)
    from mlvae_hip import ops
    for name in ("PI_ERR_LABEL", "FLVL_ERR_LABEL", "SCORE_ERR_SEGMENTS", "SCORE_ERR_K", "ALIGN_ERR_SHORT",
                 "ALIGN_ERR_CLASS", "ALIGN_ERR_BLANK", "CTC_ERR_PAIR"):
        assert getattr(ops, name) == getattr(errors, name)


def test_domain_masks():
    m = {d: errors.mask(d) for d in errors.DOMAINS}
    assert m == {"md": 6, "pi": 32, "flvl": 64, "score": 384, "align": 3584, "ctc_eval": 7168, "decode": 24,
                 "cmvn": 3}
    for a, b in itertools.combinations(("md", "pi", "flvl", "score"), 2):
        assert m[a] & m[b] == 0, (a, b)
    for a in ("md", "pi", "flvl", "score"):
        assert m[a] & (m["align"] | m["ctc_eval"]) == 0, a
    assert m["align"] & m["ctc_eval"] == 1024 | 2048
    assert m["decode"] & (m["md"] | m["pi"] | m["flvl"] | m["score"] | m["align"] | m["ctc_eval"]) == 0


# domain -> bit -> (exception class, the phrase that bit puts into the message), as the readers
# worded them before they shared one table; PREFIX: what every message of the domain contains
EXPECT = {
    "md": {2: (AssertionError, "boundaries do not give one segment per phoneme from frame 0 "),
           4: (AssertionError, "phoneme id outside [0, n_phonemes + 2)")},
    "pi": {32: (ValueError, "pi_nll: frame label outside {0, 1} (-1 = past the utterance's end) "
                            "(ref:src/models/MD_VAE/model.py:149)")},
    "flvl": {64: (ValueError, "flvl_md_head: frame-level MD label outside {0, 1} in a valid frame "
                              "(Only binary input values are supported)")},
    "score": {128: (AssertionError, "phn_acc_counts: boundary_seqs do not give one segment per phoneme from frame 0 "
                                    "(ref:src/utils/metric_stats/phn_acc_metric_stats.py:69-73)"),
              256: (RuntimeError, "boundary_topk: k out of range: fa_boundary_seqs has more boundaries than "
                                  "the utterance has frames (ref:src/models/test_b_ind_classifier/model.py:61)")},
    "align": {512: (AssertionError, "an utterance has fewer frames than HMM states (or no states, or no frames)"),
              1024: (AssertionError, "a phoneme id expands to a state class outside [0, C)"),
              2048: (AssertionError, "a CTC target class equals the blank index")},
    "ctc_eval": {1024: (AssertionError, "a phoneme id is outside [0, C)"),
                 2048: (AssertionError, "a target phoneme equals the blank index"),
                 4096: (AssertionError, "gt_phn_seq and gt_cnncl_seq of an utterance differ in length")},
    "decode": {8: (AssertionError, "MD decode: backtrack did not end at (0, 0) / empty utterance (err "),
               16: (AssertionError, "MD decode: backtrack did not end at (0, 0) / empty utterance (err ")},
    "cmvn": {1: (ValueError, "cmvn_apply: speaker id outside [0, S)"),
             2: (ValueError, "cmvn_apply: a speaker of the batch has no accumulated statistics")},
}
PREFIX = {"md": ("phoneme-recogniser targets: ", " (ref:src/modules/phoneme_recognizer.py:65-67)"),
          "align": ("sequence lattice: ",), "ctc_eval": ("CTC evaluation: ",)}
FIRST_ONLY = ("score", "cmvn")  # the lower bit's error takes precedence: its class and message alone


def _subsets(bits):
    for n in range(1, len(bits) + 1):
        yield from itertools.combinations(bits, n)


@pytest.mark.parametrize("domain", sorted(EXPECT))
def test_reader_wording_class_and_cleared_bits(domain):
    assert sorted(EXPECT[domain]) == sorted(b for b, _, _ in errors.DOMAINS[domain]["bits"])
    mask = errors.mask(domain)
    for sub in _subsets(sorted(EXPECT[domain])):
        code = sum(sub) | FOREIGN
        exc, clear = errors.read(code, domain, who="cmvn_apply")
        said = sub[:1] if domain in FIRST_ONLY else sub
        assert type(exc) is EXPECT[domain][sub[0]][0], (domain, sub, exc)
        for bit in said:
            assert EXPECT[domain][bit][1] in str(exc), (domain, sub, str(exc))
        for bit in set(EXPECT[domain]) - set(said):
            if EXPECT[domain][bit][1] not in [EXPECT[domain][b][1] for b in said]:
                assert EXPECT[domain][bit][1] not in str(exc), (domain, sub, str(exc))
        for piece in PREFIX.get(domain, ()):
            assert piece in str(exc), (domain, str(exc))
        assert clear == mask and code & ~clear == FOREIGN, (domain, sub, clear)
    assert errors.read(FOREIGN, domain, who="cmvn_apply") == (None, 0)
    assert errors.read(0, domain, who="cmvn_apply") == (None, 0)


def test_whole_messages_of_the_joined_readers():
    """The joining itself (separator, order, tail), on the words with every bit of the domain set."""
    assert str(errors.read(6, "md")[0]) == (
        "phoneme-recogniser targets: boundaries do not give one segment per phoneme from frame 0 "
        "phoneme id outside [0, n_phonemes + 2) (ref:src/modules/phoneme_recognizer.py:65-67)")
    assert str(errors.read(3584, "align")[0]) == (
        "sequence lattice: an utterance has fewer frames than HMM states (or no states, or no frames); "
        "a phoneme id expands to a state class outside [0, C); a CTC target class equals the blank index")
    assert str(errors.read(7168, "ctc_eval")[0]) == (
        "CTC evaluation: a phoneme id is outside [0, C); a target phoneme equals the blank index; "
        "gt_phn_seq and gt_cnncl_seq of an utterance differ in length")
    assert str(errors.read(8, "decode")[0]) == \
        "MD decode: backtrack did not end at (0, 0) / empty utterance (err 8)"


def test_no_second_definition_is_left():
    """The kernels write the words through the enum's names alone, and the Python constants are
    defined in errors.py alone."""
    csrc = os.path.join(PKG, "csrc")
    for f in ("md.hip", "pi.hip", "decode.hip", "flvl.hip", "score.hip", "align.hip", "ctc_eval.hip",
              "kaldi_fbank.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert "MLVAE_ERR_" in text or "MLVAE_CMVN_ERR_" in text, f
        assert not re.search(r"constexpr\s+int\s+\w*ERR\w*\s*=", text), f
        assert not re.search(r"atomicOr\(\s*(a\.)?err\s*,\s*\d", text), f
        assert not re.search(r"\bbad\s*\|?=\s*[1-9]", text), f
    ops_dir = os.path.join(PKG, "mlvae_hip", "ops")
    for f in sorted(os.listdir(ops_dir)):
        if f.endswith(".py") and f != "errors.py":
            text = open(os.path.join(ops_dir, f)).read()
            assert not re.search(r"^\w*_ERR_\w+\s*=", text, re.M), f
    assert not os.path.exists(os.path.join(PKG, "mlvae_hip", "ops.py"))
