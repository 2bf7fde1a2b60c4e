"""The CTC evaluation kernels (csrc/ctc_eval.hip) against the numpy oracle tests/ctc_np.py.  Every
comparison is exact: the kernels compute integers, or float64 sums of the fp32 emissions in frame
order (the Viterbi emissions here are multiples of 1/8, so the sums are exact and ties occur).
The log-softmax alone is floating point: 1e-5 relative-max forward, 1e-4 on the gradient, the
bounds the module-mode fp32 ops are held to (tests/test_gpu_align.py).

Shapes are the smallest at which each mechanism can break: frames across the 64-frame chunks of
the decode's compaction, more classes than lanes, a strided input; references across the lane
boundaries of the alignment (1, 5, 65 tokens) against hypotheses of 0, 1, 7, 130 tokens and a
tie-dense 3-symbol alphabet; CTC chains of 5 and 141 nodes (more than two per lane), T_b = L_b,
a repeated phoneme and chains without a path."""
import numpy as np
import pytest
import torch

import ctc_np
from ctc_np import round_len
from gpu_utils import need_gpu, rel_err

pytestmark = pytest.mark.gpu


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


# --------------------------------------------------------------------------- greedy decode
def _check_greedy(name, pout, lens, blank, dev_pout=None):
    from mlvae_hip import ops
    dev_pout = pout.cuda() if dev_pout is None else dev_pout
    pred, n = ops.ctc_greedy_decode(dev_pout, lens.cuda(), blank)
    pred2, n2 = ops.ctc_greedy_decode(dev_pout, lens.cuda(), blank)
    want, want_n = ctc_np.greedy_batch(pout.numpy(), lens.numpy(), blank)
    assert pred.dtype == torch.int32 and n.dtype == torch.int32 and pred.shape == pout.shape[:2]
    assert np.array_equal(n.cpu().numpy(), want_n), name
    assert np.array_equal(pred.cpu().numpy(), want), name
    assert torch.equal(pred, pred2) and torch.equal(n, n2)  # a rerun is bit-identical
    return pred.cpu(), n.cpu()


def test_greedy_lengths_blanks_ties_and_padding():
    need_gpu()
    B, T, C, blank = 4, 9, 5, 0
    g = torch.Generator().manual_seed(1)
    pout = torch.randn(B, T, C, generator=g)
    lens = _f32([1.0, 5 / 9, 1 / 9, 1.0])
    assert [round_len(v, T) for v in lens.numpy()] == [9, 5, 1, 9]
    pout[3, :, blank] = 9.0                 # an all-blank utterance: length 0
    pout[0, 2, 1] = pout[0, 2, 3] = 7.0     # an argmax tie: the lowest class
    pout[0, 3, 1], pout[0, 4, 2] = 7.0, 7.0
    pout[1, 5:, 4] = 8.0                    # a non-blank class at t >= T_b never contributes
    pout[1, 4, 0] = 8.0                     # ... the last valid frame is a blank
    pout[2, 0, 2] = 8.0
    pred, n = _check_greedy("small", pout, lens, blank)
    assert n[3] == 0 and (pred[3] == -1).all() and n[2] == 1 and pred[2, 0] == 2
    _check_greedy("blank = C - 1", pout, lens, C - 1)


def test_greedy_runs_across_the_64_frame_chunks_and_wide_classes():
    need_gpu()
    B, T, C, blank = 3, 130, 70, 69         # more classes than lanes
    g = torch.Generator().manual_seed(2)
    pout = torch.randn(B, T, C, generator=g)
    pout[0, 60:68, 66] = 9.0                # a run over frames 63 / 64: one token
    pout[0, 125:130, 67] = 9.0              # and over 127 / 128
    pout[1, 63, 5], pout[1, 64, 6] = 9.0, 9.0     # a change exactly at the chunk boundary: two tokens
    pout[1, 127, blank], pout[1, 128, 6] = 9.0, 9.0
    pout[2, :, :] = 0.0                     # every class ties everywhere: class 0 once
    lens = _f32([1.0, 1.0, 129 / 130])
    pred, n = _check_greedy("chunks", pout, lens, blank)
    assert n[2] == 1 and pred[2, 0] == 0
    # a strided input: rows ld > C floats apart, the columns beyond C hold larger values
    wide = torch.full((B, T, C + 9), 50.0)
    wide[:, :, :C] = pout
    dev = wide.cuda()[:, :, :C]
    assert not dev.is_contiguous() and dev.stride(1) == C + 9
    _check_greedy("strided", pout, lens, blank, dev_pout=dev)


# --------------------------------------------------------------------------- edit alignment
def _check_align(name, pred, pred_len, phns, phn_lens, cnncls, cnncl_lens):
    from mlvae_hip import ops
    args = (torch.from_numpy(pred).cuda(), torch.tensor(pred_len, dtype=torch.int32).cuda(),
            torch.from_numpy(phns).cuda(), _f32(phn_lens).cuda(), torch.from_numpy(cnncls).cuda(),
            _f32(cnncl_lens).cuda())
    ali, edits = ops.edit_align(*args)
    counts = ops.ctc_md_counts(ali, *args[2:])
    ali2, edits2 = ops.edit_align(*args)
    counts2 = ops.ctc_md_counts(ali2, *args[2:])
    want_ali, want_ops, want_counts = ctc_np.align_batch(pred, pred_len, phns, np.float32(phn_lens), cnncls,
                                                         np.float32(cnncl_lens))
    assert ali.dtype == edits.dtype == counts.dtype == torch.int32
    assert np.array_equal(edits.cpu().numpy(), want_ops), name
    assert np.array_equal(ali.cpu().numpy(), want_ali), name
    assert np.array_equal(counts.cpu().numpy(), want_counts), name
    assert torch.equal(ali, ali2) and torch.equal(edits, edits2) and torch.equal(counts, counts2)
    ops.raise_ctc_eval_err()  # nothing set
    return ali.cpu().numpy(), edits.cpu().numpy(), counts.cpu().numpy()


def _pad(seqs, width, fill, dtype):
    out = np.full((len(seqs), width), fill, dtype=dtype)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out


def test_edit_align_lengths_across_the_lane_boundaries():
    need_gpu()
    g = np.random.default_rng(5)
    L, Tp = 65, 130
    refs, hyps = [], []
    for la in (1, 5, 65):
        for lb in (0, 1, 7, 130):
            refs.append(g.integers(1, 4, la))
            hyps.append(g.integers(1, 4, lb))
    phns = _pad(refs, L, 0, np.int64)
    cnncls = phns.copy()
    flip = g.random(phns.shape) < 0.3
    cnncls[flip] = (cnncls[flip] % 3) + 1      # canonical differs at a third of the positions
    lens = [len(r) / L for r in refs]
    assert [round_len(np.float32(v), L) for v in lens] == [len(r) for r in refs]
    pred = _pad(hyps, Tp, -1, np.int32)
    ali, edits, counts = _check_align("lengths", pred, [len(h) for h in hyps], phns, lens, cnncls, lens)
    assert edits[:, :, 3].tolist() == [[len(r)] * 2 for r in refs]
    assert (edits[0, 0, :3] == [0, 1, 0]).all() and (ali[0, 0] == -1).all()  # no hypothesis: a deletion


def test_edit_align_tie_dense_random_pairs():
    need_gpu()
    g = np.random.default_rng(6)
    n, L, Tp = 200, 12, 14
    refs = [g.integers(0, 3, g.integers(0, L + 1)) for _ in range(n)]
    hyps = [g.integers(0, 3, g.integers(0, Tp + 1)) for _ in range(n)]
    phns = _pad(refs, L, 0, np.int64)
    cnncls = _pad([(r + (g.random(len(r)) < 0.3)) % 3 for r in refs], L, 0, np.int64)
    lens = [len(r) / L for r in refs]
    assert [round_len(np.float32(v), L) for v in lens] == [len(r) for r in refs]
    pred = _pad(hyps, Tp, -1, np.int32)
    ali, edits, counts = _check_align("random", pred, [len(h) for h in hyps], phns, lens, cnncls, lens)
    assert (counts[:, :4].sum(1) == edits[:, 0, 3]).all() and (counts[:, 4] + counts[:, 6] == edits[:, 0, 3]).all()
    # the hand-written case of the tie rule (tests/test_ctc_eval_cpu.py)
    a = np.array([[1, 2, 2, 3]])
    ali, edits, _ = _check_align("tie", np.array([[1, 2, 3]], dtype=np.int32), [3], a, [1.0], a, [1.0])
    assert ali[0, 0].tolist() == [1, 2, -1, 3] and edits[0, 0].tolist() == [0, 1, 0, 4]


def test_edit_align_cap_and_pair_error():
    need_gpu()
    from mlvae_hip import _lib, ops
    cap = _lib.lib().mlvae_edit_align_max_ref()
    assert cap == 1024
    pred = torch.zeros(1, 4, dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    big = torch.zeros(1, cap + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="at most 1024"):
        ops.edit_align(pred, n, big, torch.ones(1), big, torch.ones(1))
    # the library itself refuses the call with a status, before any launch
    assert _lib.lib().mlvae_edit_align_workspace_size(1, cap + 1, 4) == 0
    rc = _lib.lib().mlvae_edit_align(1, cap + 1, 4, big.data_ptr(), None, pred.data_ptr(), n.data_ptr(), None,
                                     None, None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 1 and "at most 1024" in _lib.last_error()
    # the cap itself runs: 1024 tokens against an empty hypothesis are 1024 deletions
    ok = torch.ones(1, cap, dtype=torch.int64, device="cuda")
    ali, edits = ops.edit_align(pred, n, ok, torch.ones(1), ok, torch.ones(1))
    assert edits[0, 0].tolist() == [0, cap, 0, cap] and bool((ali == -1).all())
    # pronounced and canonical sequences of different lengths: a bit of the error word
    phns = torch.ones(1, 4, dtype=torch.int64, device="cuda")
    ali, _ = ops.edit_align(pred, n, phns, torch.ones(1), phns, _f32([0.5]))
    ops.ctc_md_counts(ali, phns, torch.ones(1), phns, _f32([0.5]))
    with pytest.raises(AssertionError, match="differ in length"):
        ops.raise_ctc_eval_err()
    ops.raise_ctc_eval_err()  # cleared


# --------------------------------------------------------------------------- Viterbi
def _eighths(B, T, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.round(torch.randn(B, T, C, generator=g) * 8) / 8


def _check_viterbi(name, pout, lens, phns, phn_lens, blank):
    from mlvae_hip import ops
    args = (pout.cuda(), lens.cuda(), phns.cuda(), phn_lens.cuda(), blank)
    vs, bd, inf = ops.ctc_viterbi(*args)
    vs2, bd2, inf2 = ops.ctc_viterbi(*args)
    want_vs, want_bd, want_inf = ctc_np.viterbi_batch(pout.numpy(), lens.numpy(), phns.numpy(),
                                                      phn_lens.numpy(), blank)
    assert vs.dtype == torch.float32 and bd.dtype == inf.dtype == torch.int32
    assert np.array_equal(inf.cpu().numpy(), want_inf), name
    assert np.array_equal(bd.cpu().numpy(), want_bd), name
    assert np.array_equal(vs.cpu().numpy(), want_vs.astype(np.float32)), name
    assert torch.equal(vs, vs2) and torch.equal(bd, bd2) and torch.equal(inf, inf2)
    B, T, _ = pout.shape
    for b in range(B):
        Tb, Lb = round_len(lens[b].item(), T), round_len(phn_lens[b].item(), phns.shape[1])
        if not want_inf[b]:
            assert int((bd[b] == 1).sum()) == Lb and (Lb == 0 or bd[b, 0] == 1), name  # exactly L ones
        assert bool((bd[b, Tb:] == -1).all())
    ops.raise_ctc_eval_err()
    return vs.cpu(), bd.cpu(), inf.cpu()


def test_viterbi_small_chains_repeats_and_infeasible():
    need_gpu()
    B, T, C, blank = 7, 6, 5, 0
    pout = _eighths(B, T, C, 3)
    pout[6] = 0.0                                         # every path ties: the tie order decides
    phns = torch.tensor([[1, 2], [3, 3], [3, 3], [1, 2], [3, 1], [2, 2], [1, 2]])
    lens = _f32([1.0, 0.5, 1 / 3, 1 / 3, 0.0, 1.0, 1.0])
    phn_lens = _f32([1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 1.0])
    assert [round_len(v, T) for v in lens.numpy()] == [6, 3, 2, 2, 0, 6, 6]
    _, bd, inf = _check_viterbi("small", pout, lens, phns, phn_lens, blank)
    # [3, 3] needs a blank between: no path in 2 frames, one in 3; T_b = L_b with different classes
    # is feasible (the skip); no frames is no path
    assert inf.tolist() == [0, 0, 1, 0, 1, 0, 0]
    assert bd[1, :3].tolist() == [1, 0, 1] and bd[2, :2].tolist() == [1, 1] and bd[3, :2].tolist() == [1, 1]
    _check_viterbi("blank = C - 1", pout, lens, phns, phn_lens, C - 1)


def test_viterbi_long_chain_more_than_two_nodes_per_lane():
    need_gpu()
    B, T, C, L, blank = 3, 150, 40, 70, 39
    pout = _eighths(B, T, C, 4)
    phns = torch.randint(0, C - 1, (B, L), generator=torch.Generator().manual_seed(9))
    phns[0, 10] = phns[0, 11]                              # a repeat inside the chain
    lens = _f32([1.0, 0.6, 70 / 150])                      # 150, 90 and 70 frames
    phn_lens = _f32([1.0, 0.5, 1.0])                       # 141, 71 and 141 nodes
    assert [round_len(v, T) for v in lens.numpy()] == [150, 90, 70]
    _, _, inf = _check_viterbi("long", pout, lens, phns, phn_lens, blank)
    assert inf[0] == 0 and inf[1] == 0  # utterance 2 has T_b = L_b: feasible iff it has no repeat


def test_viterbi_data_errors_and_limits():
    need_gpu()
    from mlvae_hip import ops
    pout = _eighths(2, 6, 5, 5).cuda()
    ones = torch.ones(2)
    vs, bd, inf = ops.ctc_viterbi(pout, ones, torch.tensor([[1, 2], [1, 0]]), ones, 0)  # a target equal to blank
    assert vs[1] == 0 and bool((bd[1] == -1).all()) and inf.tolist() == [0, 0] and int((bd[0] == 1).sum()) == 2
    with pytest.raises(AssertionError, match="blank"):
        ops.raise_ctc_eval_err()
    ops.ctc_viterbi(pout, ones, torch.tensor([[1, 2], [1, 5]]), ones, 0)               # an id outside [0, C)
    with pytest.raises(AssertionError, match=r"outside \[0, C\)"):
        ops.raise_ctc_eval_err()
    with pytest.raises(ValueError, match="blank 5 outside"):
        ops.ctc_viterbi(pout, ones, torch.tensor([[1, 2], [1, 2]]), ones, 5)
    with pytest.raises(ValueError, match="1025 nodes"):
        ops.ctc_viterbi(pout, ones, torch.zeros(2, 512, dtype=torch.int64), ones, 0)


# --------------------------------------------------------------------------- log-softmax
def test_log_softmax_forward_and_backward():
    need_gpu()
    from mlvae_hip import ops
    g = torch.Generator().manual_seed(7)
    for shape in ((3, 7, 41), (2, 5, 70), (5, 1)):
        x = (torch.randn(*shape, generator=g) * 3).cuda().requires_grad_(True)
        w = torch.randn(*shape, generator=g).cuda()
        y = ops.log_softmax(x)
        (y * w).sum().backward()
        xr = x.detach().double().cpu().requires_grad_(True)
        yr = torch.log_softmax(xr, -1)
        (yr * w.double().cpu()).sum().backward()
        ef, eb = rel_err(y, yr), rel_err(x.grad, xr.grad)
        print(f"log_softmax {shape}: forward rel {ef:.2e}, backward rel {eb:.2e}")
        if shape[-1] == 1:
            assert bool((y == 0).all()) and bool((x.grad == 0).all())
        else:
            assert ef < 1e-5 and eb < 1e-4
