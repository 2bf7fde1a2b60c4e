"""mlvae_viterbi_md_ex's skip_empty (csrc/decode.hip): the zero-length filler rows a short rank
slice carries in data-parallel evaluation (utils/data_io.py) decode to nothing and set no error
bit, next to real rows that decode exactly as the reference did (tests/golden/decode_tiny.npz);
skip_empty = 0 is mlvae_viterbi_md, and a row that is empty in frames only stays an error."""
import numpy as np
import pytest
import torch

from gpu_utils import need_gpu
from test_oracle_decode_golden import expected, load

pytestmark = pytest.mark.gpu


def _with_filler(t, feat_len=0.0, seq_len=0.0):
    """decode_tiny with one more row of zeros whose relative lengths are the given ones."""
    out = {"prior": t["prior"]}
    for k in ("logits", "boundary_v", "pi_logits", "seqs"):
        out[k] = torch.cat([t[k], torch.zeros_like(t[k][:1])])
    out["feat_lens"] = torch.cat([t["feat_lens"], torch.tensor([feat_len], dtype=t["feat_lens"].dtype)])
    out["seq_lens"] = torch.cat([t["seq_lens"], torch.tensor([seq_len], dtype=t["seq_lens"].dtype)])
    return out


def _decode(t, weight, skip_empty):
    from utils.decode_utils import decode_md_device
    pred = {"phn_recog_out": t["logits"].cuda(), "boundary_v": t["boundary_v"].cuda(),
            "pi_logits": t["pi_logits"].cuda()}
    out = decode_md_device(pred, t["feat_lens"].cuda(), t["seqs"].cuda(), t["seq_lens"].cuda(),
                           t["prior"].cuda(), weight, skip_empty=skip_empty)
    return [x.cpu().numpy() for x in out]


def test_filler_row_decodes_to_nothing():
    need_gpu()
    r, t = load("decode_tiny")
    B = t["logits"].shape[0]
    bnd, flvl, plvl, lens, err = _decode(_with_filler(t), float(r["weight"]), True)
    assert err[0] == 0
    exp_b, exp_f, exp_p = expected(r)
    for i in range(B):
        Ti, Li = int(r["T_i"][i]), int(r["L_i"][i])
        assert tuple(lens[i]) == (Ti, Li)
        assert np.array_equal(bnd[i, :Ti], exp_b[i]) and bool((bnd[i, Ti:] == -1).all())
        assert np.array_equal(flvl[i, :Ti], exp_f[i]) and bool((flvl[i, Ti:] == -1).all())
        assert np.array_equal(plvl[i, :Li], exp_p[i]) and bool((plvl[i, Li:] == -1).all())
    assert tuple(lens[B]) == (0, 0)
    assert bool((bnd[B] == -1).all()) and bool((flvl[B] == -1).all()) and bool((plvl[B] == -1).all())
    # the host lists: the filler is an empty entry
    from utils.decode_utils import decoded_lists
    lists = decoded_lists(*[torch.from_numpy(x) for x in (bnd, flvl, plvl, lens, err)])
    assert [len(x[B]) for x in lists] == [0, 0, 0]


def test_without_skip_empty_the_filler_is_an_error():
    need_gpu()
    r, t = load("decode_tiny")
    *_, lens, err = _decode(_with_filler(t), float(r["weight"]), False)
    assert err[0] == 16
    assert tuple(lens[-1]) == (0, 0)


def test_frames_empty_but_phonemes_not_stays_an_error():
    need_gpu()
    r, t = load("decode_tiny")
    *_, err = _decode(_with_filler(t, 0.0, 0.5), float(r["weight"]), True)
    assert err[0] == 16
    *_, err = _decode(_with_filler(t, 0.5, 0.0), float(r["weight"]), True)  # and the other way round
    assert err[0] == 16
