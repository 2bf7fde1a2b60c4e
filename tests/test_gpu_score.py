"""The per-utterance scoring kernels (csrc/score.hip) through mlvae_hip.ops and the C ABI.

* every case of tests/golden/score_cases.npz (the reference's own scores, make_golden_score.py),
  batched with its padding (NaN, inf and stray ones past T_i): counts and chosen frames exact;
* random inputs at (B, T, C, L) = (1,1,1,1), (3,21,7,6), (5,13,41,4), (2,257,67,40), (1,1025,3,128)
  -- T = 1, odd sizes, C below / at / above a wave, T past one 256-frame chunk and past four --
  against the host functions of utils/metric_stats: a zero-length row where B >= 3, a full-length
  row, NaN / inf logits, inf in v, stray flags past T_i; exact ties in v pin the index rule; a
  rerun is identical;
* the error bits 128 and 256, set by a bad flag count and by k > T_i and by nothing else, raised
  and cleared by ops.raise_score_err alone; status 1 for null pointers and for T over the limit.
Everything compared is an integer: the tolerance is 0."""
import os

import numpy as np
import pytest
import torch

from gpu_utils import P, need_gpu, stream

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_cases.npz")
SHAPES = [(1, 1, 1, 1), (3, 21, 7, 6), (5, 13, 41, 4), (2, 257, 67, 40), (1, 1025, 3, 128)]


@pytest.fixture(scope="module")
def cases():
    d = np.load(GOLD)
    return {k: d[k] for k in d.files}


def _err_word():
    from mlvae_hip import ops
    return ops._md_err()


def _clean_err():
    e = _err_word()
    e.zero_()  # whatever an earlier test left
    return e


# --------------------------------------------------------------------------- the reference's cases
def test_cases_counts_and_chosen_frames(cases):
    need_gpu()
    from mlvae_hip import ops
    c = cases
    err = _clean_err()
    cu = lambda k: torch.from_numpy(c[k]).cuda()
    fl, plens = cu("feat_lens"), cu("phn_lens")
    counts = ops.phn_acc_counts(cu("logits"), fl, cu("flvl_tgt"), cu("plvl_tgt"), plens, cu("phn_boundary"))
    want = np.stack([c["flvl_correct"], c["T"], c["plvl_correct"], c["L"]], 1)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want)
    none = ops.phn_acc_counts(cu("logits"), fl, cu("flvl_tgt"))
    want[:, 2:] = 0
    assert np.array_equal(none.cpu().numpy(), want)
    pred = ops.boundary_topk(cu("boundary_v"), fl, cu("fa_boundary"))
    assert pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy(), c["chosen"])
    bc = ops.boundary_counts(pred, cu("gt_boundary"), fl)
    assert np.array_equal(bc.cpu().numpy(), np.stack([c["correct"], c["n_pred"], c["n_target"]], 1))
    assert int(err.item()) == 0
    # the stats objects: the reference's scores from the device counts
    from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
    from utils.metric_stats.phn_acc_metric_stats import PhnAccMetricStats
    ids = [f"utt{i}" for i in range(len(c["T"]))]
    ps, bs = PhnAccMetricStats(), BoundaryMetricStats()
    ps.append_counts(ids, counts)
    bs.append_counts(ids, bc)
    assert ps.scores_list == [] and bs.scores_list == []
    ps.summarize(), bs.summarize()
    for i in range(len(ids)):
        assert ps.scores_list[i]["flvl_acc"] == c["flvl_acc"][i] and ps.scores_list[i]["plvl_acc"] == c["plvl_acc"][i]
        for k in ("pre", "rec", "f1", "r_value"):
            assert bs.scores_list[i][k] == c[k][i], (i, k)


# --------------------------------------------------------------------------- random inputs
def _lengths(B, n, g, least=1):
    """Valid lengths: a full row first, a zero-length row last where B >= 3."""
    v = torch.randint(least, n + 1, (B,), generator=g)
    v[0] = n
    if B >= 3:
        v[-1] = 0
    return v


def _random(B, T, C, L, seed):
    g = torch.Generator().manual_seed(seed)
    Ti = _lengths(B, T, g)
    Li = torch.minimum(_lengths(B, L, g), Ti)
    Li[Ti == 0] = 0
    fl, pl = (Ti.float() / T), (Li.float() / L)
    assert torch.equal(torch.round(fl * T).long(), Ti) and torch.equal(torch.round(pl * L).long(), Li)
    logits = torch.randn(B, T, C, generator=g)
    # NaN and inf among the valid logits (torch.argmax's order), NaN past T_i
    hit = torch.rand(B, T, C, generator=g) * C  # about a quarter of the frames hold a special value
    logits[hit < 0.1] = float("nan")
    logits[(hit >= 0.1) & (hit < 0.2)] = float("inf")
    logits[(hit >= 0.2) & (hit < 0.3)] = float("-inf")
    flvl = torch.randint(-1, C + 1, (B, T), generator=g)  # out-of-range targets never match
    plvl = torch.randint(0, C, (B, L), generator=g)
    v = torch.rand(B, T, generator=g)
    v[torch.rand(B, T, generator=g) < 0.05] = float("inf")
    v = (v * 8).round() / 8 if T > 8 else v  # exact ties: the index rule decides
    pb, gt, fa = torch.zeros(B, T), torch.zeros(B, T), torch.zeros(B, T)
    for b in range(B):
        t, l = int(Ti[b]), int(Li[b])
        logits[b, t:] = float("nan")
        v[b, t:] = float("inf")
        pb[b, t:] = 1.0  # stray flags past T_i
        gt[b, t:] = 1.0
        if t:
            pb[b, 0] = 1.0
            pb[b, torch.randperm(t - 1, generator=g)[:l - 1] + 1] = 1.0
            # about half of the targets are the right ones, so that the counts are not all zero
            right = torch.rand(t, generator=g) < 0.5
            flvl[b, :t] = torch.where(right, torch.argmax(logits[b, :t], -1), flvl[b, :t])
            starts = torch.where(pb[b, :t] == 1)[0].tolist() + [t]
            for k_, (s_, e_) in enumerate(zip(starts[:-1], starts[1:])):
                if k_ % 2 == 0:
                    acc = torch.zeros(C)
                    for u in range(s_, e_):
                        acc = acc + logits[b, u]
                    plvl[b, k_] = torch.argmax(acc)
            gt[b, :t] = (torch.rand(t, generator=g) < 0.3).float()
            k = int(torch.randint(0, t + 1, (1,), generator=g))
            fa[b, torch.randperm(T, generator=g)[:k]] = 1.0  # anywhere in the padded row
    return dict(Ti=Ti, Li=Li, fl=fl, pl=pl, logits=logits, flvl=flvl, plvl=plvl, v=v, pb=pb, gt=gt, fa=fa)


def _host(d, B):
    """The counts and chosen frames by the host functions, utterance by utterance."""
    from utils.metric_stats.boundary_metric_stats import boundary_scoring
    T = d["v"].shape[1]
    pc, bc, chosen = [], [], torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        t, l = int(d["Ti"][b]), int(d["Li"][b])
        x = d["logits"][b, :t]
        fc = int((torch.argmax(x, -1) == d["flvl"][b, :t]).sum()) if t else 0
        hit = 0
        if t:
            starts = torch.where(d["pb"][b, :t] == 1)[0].tolist() + [t]
            assert len(starts) - 1 == l
            for k, (s, e) in enumerate(zip(starts[:-1], starts[1:])):
                acc = torch.zeros(x.shape[1])
                for u in range(s, e):  # fp32 from 0, frames in increasing t
                    acc = acc + x[u]
                hit += int(torch.argmax(acc) == d["plvl"][b, k])
        pc.append([fc, t, hit, l])
        # (value descending, index ascending), a NaN above every number: a stable sort of -v
        k = int(d["fa"][b].sum())
        key = -torch.nan_to_num(d["v"][b, :t], nan=float("inf"), posinf=3e38)
        key[torch.isnan(d["v"][b, :t])] = -float("inf")
        order = torch.sort(key, stable=True).indices
        chosen[b, :t] = 0
        chosen[b, order[:k]] = 1
        if t:
            s = boundary_scoring(chosen[b, :t].float(), d["gt"][b, :t])
            n_pred, n_tgt = int(chosen[b, :t].sum()), int(d["gt"][b, :t].sum())
            bc.append([int(round(s["pre"] * (n_pred + 1e-6) / 100)), n_pred, n_tgt])
        else:
            bc.append([0, 0, 0])
    return torch.tensor(pc, dtype=torch.int32), torch.tensor(bc, dtype=torch.int32), chosen


@pytest.mark.parametrize("B,T,C,L", SHAPES)
def test_random_inputs_match_the_host_functions(B, T, C, L):
    need_gpu()
    from mlvae_hip import ops
    err = _clean_err()
    d = _random(B, T, C, L, seed=B * 1000 + T)
    want_pc, want_bc, want_chosen = _host(d, B)
    cu = {k: x.cuda() for k, x in d.items()}

    def run():
        pc = ops.phn_acc_counts(cu["logits"], cu["fl"], cu["flvl"], cu["plvl"], cu["pl"], cu["pb"])
        pred = ops.boundary_topk(cu["v"], cu["fl"], cu["fa"])
        return pc.cpu(), pred.cpu(), ops.boundary_counts(pred, cu["gt"], cu["fl"]).cpu()

    pc, pred, bc = run()
    assert torch.equal(pc, want_pc), (pc, want_pc)
    assert torch.equal(pred, want_chosen)
    assert torch.equal(bc, want_bc), (bc, want_bc)
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((pc, pred, bc), again))  # a rerun is identical
    assert int(err.item()) == 0


def test_ties_take_the_lower_index():
    need_gpu()
    from mlvae_hip import ops
    err = _clean_err()
    nan, inf = float("nan"), float("inf")
    v = torch.tensor([[0.5, 0.5, 0.5, 0.5, 0.5, 0.5],      # all equal: the first k
                      [0.0, -0.0, 1.0, 1.0, -1.0, 1.0],    # -0 and +0 are one value
                      [inf, nan, 1.0, nan, inf, 0.0],      # a NaN above inf, the first one first
                      [3.0, 2.0, 3.0, 2.0, 9.0, 9.0]])     # the last two are past T_i = 4
    fa = torch.zeros(4, 6)
    fa[0, 3:5] = 1   # k = 2
    fa[1, :4] = 1    # k = 4
    fa[2, 1:4] = 1   # k = 3
    fa[3, 5] = 1     # k = 1, counted in the padding of the row
    lens = torch.tensor([1.0, 1.0, 1.0, 4 / 6])
    pred = ops.boundary_topk(v.cuda(), lens.cuda(), fa.cuda()).cpu()
    assert pred.tolist() == [[1, 1, 0, 0, 0, 0], [1, 0, 1, 1, 0, 1], [1, 1, 0, 1, 0, 0], [1, 0, 0, 0, -1, -1]]
    assert int(err.item()) == 0


# --------------------------------------------------------------------------- error bits
def _valid_batch():
    """B = 2, T = 6: two segments each, k = 2."""
    logits = torch.randn(2, 6, 3, generator=torch.Generator().manual_seed(1))
    lens = torch.tensor([1.0, 0.5])
    flvl = torch.zeros(2, 6, dtype=torch.int64)
    plvl = torch.zeros(2, 2, dtype=torch.int64)
    pb = torch.tensor([[1.0, 0, 0, 1, 0, 0], [1.0, 0, 1, 1, 1, 1]])  # ones past T_1 = 3
    return [x.cuda() for x in (logits, lens, flvl, plvl, torch.ones(2), pb)]


def test_error_bits_and_raise_score_err():
    need_gpu()
    from mlvae_hip import ops
    err = _clean_err()
    logits, lens, flvl, plvl, plens, pb = _valid_batch()
    v = torch.rand(2, 6).cuda()
    ops.phn_acc_counts(logits, lens, flvl, plvl, plens, pb)
    pred = ops.boundary_topk(v, lens, pb)  # k = (2, 5 in the padded row): row 1 asks for more than T_1
    assert int(err.item()) == 256
    assert pred[1].tolist() == [0, 0, 0, -1, -1, -1]  # that row gets no ones
    with pytest.raises(RuntimeError, match="k out of range"):
        ops.raise_score_err()
    assert int(err.item()) == 0
    ops.raise_score_err()  # nothing set: nothing raised
    # a flag count that differs from L_i; no flag at frame 0; both leave plvl_correct at 0
    for bad in (torch.tensor([1.0, 1, 0, 1, 0, 0]), torch.tensor([0.0, 1, 0, 1, 0, 0])):
        x = pb.clone()
        x[0] = bad.cuda()
        counts = ops.phn_acc_counts(logits, lens, flvl, plvl, plens, x)
        assert int(err.item()) == 128
        assert counts[0, 2].item() == 0 and counts[:, 3].tolist() == [2, 2]
        err.bitwise_or_(64)  # another owner's bit stays
        with pytest.raises(AssertionError, match="one segment per phoneme"):
            ops.raise_score_err()
        assert int(err.item()) == 64
        err.zero_()
    # a zero-length row with no phonemes is a filler, not an error
    z = torch.tensor([1.0, 0.0]).cuda()
    counts = ops.phn_acc_counts(logits, z, flvl, plvl, z, pb)
    assert counts[1].tolist() == [0, 0, 0, 0] and int(err.item()) == 0
    ops.boundary_counts(ops.boundary_topk(v, z, torch.zeros(2, 6).cuda()), pb, z)
    assert int(err.item()) == 0


def test_status_codes_through_the_c_abi():
    need_gpu()
    from mlvae_hip import _lib, ops
    l = _lib.lib()
    err = _clean_err()
    logits, lens, flvl, plvl, plens, pb = _valid_batch()
    counts = torch.zeros(2, 4, dtype=torch.int32).cuda()
    pred = torch.zeros(2, 6, dtype=torch.int32).cuda()
    k = torch.zeros(2, dtype=torch.int32).cuda()
    s = stream()
    ok = lambda: l.mlvae_phn_acc(2, 6, 3, 2, P(logits), 3, P(lens), flvl.data_ptr(), plvl.data_ptr(),
                                 P(plens), P(pb), counts.data_ptr(), P(err), s)
    assert ok() == 0
    # empty batches are no-ops, whatever the pointers
    assert l.mlvae_phn_acc(0, 6, 3, 2, None, 3, None, None, None, None, None, None, None, s) == 0
    assert l.mlvae_boundary_topk(2, 0, None, None, None, None, None, None, s) == 0
    assert l.mlvae_boundary_score(0, 0, None, None, None, None, s) == 0
    # null pointers and negative sizes
    assert l.mlvae_phn_acc(2, 6, 3, 2, None, 3, P(lens), flvl.data_ptr(), plvl.data_ptr(), P(plens), P(pb),
                           counts.data_ptr(), P(err), s) == 1
    assert "null" in _lib.last_error()
    assert l.mlvae_phn_acc(2, 6, 3, 2, P(logits), 3, P(lens), flvl.data_ptr(), plvl.data_ptr(), P(plens),
                           P(pb), counts.data_ptr(), None, s) == 1
    assert l.mlvae_phn_acc(2, 6, 3, 2, P(logits), 3, P(lens), flvl.data_ptr(), plvl.data_ptr(), None,
                           P(pb), counts.data_ptr(), P(err), s) == 1
    assert l.mlvae_phn_acc(-1, 6, 3, 2, P(logits), 3, P(lens), flvl.data_ptr(), plvl.data_ptr(), P(plens),
                           P(pb), counts.data_ptr(), P(err), s) == 1
    assert l.mlvae_phn_acc(2, 6, 0, 2, P(logits), 3, P(lens), flvl.data_ptr(), plvl.data_ptr(), P(plens),
                           P(pb), counts.data_ptr(), P(err), s) == 1
    assert l.mlvae_boundary_topk(2, 6, None, P(lens), P(pb), pred.data_ptr(), k.data_ptr(), P(err), s) == 1
    assert l.mlvae_boundary_topk(2, 6, P(pb), P(lens), P(pb), pred.data_ptr(), k.data_ptr(), None, s) == 1
    assert l.mlvae_boundary_topk(2, -6, P(pb), P(lens), P(pb), pred.data_ptr(), k.data_ptr(), P(err), s) == 1
    assert l.mlvae_boundary_score(2, 6, None, P(pb), P(lens), counts.data_ptr(), s) == 1
    assert l.mlvae_boundary_score(2, 6, pred.data_ptr(), P(pb), P(lens), None, s) == 1
    # T over the LDS limit: status 1 before any launch, and the Python side names the limit
    limit = l.mlvae_boundary_topk_max_frames()
    assert limit >= 8192
    assert l.mlvae_boundary_topk(1, limit + 1, P(pb), P(lens), P(pb), pred.data_ptr(), k.data_ptr(),
                                 P(err), s) == 1
    assert str(limit) in _lib.last_error()
    with pytest.raises(ValueError, match=str(limit)):
        ops.boundary_topk(torch.zeros(1, limit + 1).cuda(), lens[:1], torch.zeros(1, limit + 1).cuda())
    torch.cuda.synchronize()
    assert int(err.item()) == 0
