"""The readers of the device error word against the real word: each raises its domain's exception,
clears its own bits alone and leaves a foreign bit standing.  No kernel is launched (the word is
filled from the host; the kernels' side is tests/test_gpu_md.py, _pi, _flvl_head, _score, _align,
_ctc_eval, _kaldi_fbank)."""
import pytest
import torch

from gpu_utils import need_gpu

FOREIGN = 1 << 20  # a bit no domain owns


def _readers(ops, word):
    from utils.decode_utils import raise_decode_err
    return {
        "md": (lambda: ops._raise_md(word), AssertionError),
        "pi": (ops.raise_pi_err, ValueError),
        "flvl": (ops.raise_flvl_err, ValueError),
        "score": (ops.raise_score_err, AssertionError),  # the segments error before the k error
        "align": (ops.raise_align_err, AssertionError),
        "ctc_eval": (ops.raise_ctc_eval_err, AssertionError),
        "cmvn": (lambda: ops._raise_cmvn(word, "cmvn_apply"), ValueError),
        # the decode reader takes the word's value (its word is the caller's): it clears nothing
        "decode": (lambda: raise_decode_err(word.item()), AssertionError),
    }


@pytest.mark.gpu
def test_each_reader_raises_and_clears_its_own_bits_alone():
    need_gpu()
    from mlvae_hip import ops
    from mlvae_hip.ops import errors
    word = ops._md_err()
    assert word.dtype == torch.int32 and word.numel() == 1 and word is ops._md_err()
    try:
        readers = _readers(ops, word)
        assert sorted(readers) == sorted(errors.DOMAINS)
        for domain, (reader, exc) in readers.items():
            mask = errors.mask(domain)
            word.fill_(mask | FOREIGN)
            with pytest.raises(exc):
                reader()
            left = int(word.item())
            assert left == (mask | FOREIGN if domain == "decode" else FOREIGN), (domain, left)
            word.fill_(FOREIGN)
            reader()  # no bit of the domain: nothing raised, nothing cleared
            assert int(word.item()) == FOREIGN, domain
    finally:
        word.zero_()
