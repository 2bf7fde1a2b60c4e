"""The HMM / CTC sequence lattice and the CTC evaluation path (csrc/align.hip,
csrc/ctc_eval.hip)."""
import torch

from .._lib import check, lib
from ._core import _md_err, _need, _p, raise_err, _score_lens, _stream, _workspace, _ws_bytes


# --------------------------------------------------------------------------- HMM / CTC sequence lattice
TOPO_HMM, TOPO_CTC = 0, 1


def raise_align_err():
    """Read the device error word's lattice bits (one host sync) and clear them alone:
    AssertionError naming the condition (what the aligner's own asserts would have said per batch)."""
    raise_err(_md_err(), "align")


class CenterLogSoftmaxFn(torch.autograd.Function):
    """y = log_softmax(x - mean_t(x), dim=-1) over [B, T, C], the mean over all T rows of the
    padded batch (ref:src/models/HMM_DNN_ALI/model.py:43-44)."""

    @staticmethod
    def forward(ctx, x):
        x = _need(x, "center_log_softmax x")
        B, T, C = x.shape
        y = torch.empty_like(x)
        ws = _workspace(lib().mlvae_center_lsm_workspace_size(B, C), "center_lsm")
        check(lib().mlvae_center_lsm_fwd(B, T, C, _p(x), _p(y), _p(ws), _ws_bytes(ws), _stream()),
              "center_lsm_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        B, T, C = y.shape
        dy = _need(dy, "center_log_softmax grad")
        dx = torch.empty_like(y)
        ws = _workspace(lib().mlvae_center_lsm_workspace_size(B, C), "center_lsm")
        check(lib().mlvae_center_lsm_bwd(B, T, C, _p(dy), _p(y), _p(dx), _p(ws), _ws_bytes(ws),
                                         _stream()), "center_lsm_bwd")
        return dx


def center_log_softmax(x):
    if x.dim() != 3 or x.shape[2] < 1:
        raise ValueError(f"center_log_softmax: x must be [B, T, C] with C >= 1, got {tuple(x.shape)}")
    return CenterLogSoftmaxFn.apply(x)


def _lattice_args(what, pout, lens, phns, phn_lens, spp):
    if pout.dim() != 3 or pout.shape[2] < 1:
        raise ValueError(f"{what}: pout must be [B, T, C] with C >= 1, got {tuple(pout.shape)}")
    if phns.dim() != 2 or phns.shape[0] != pout.shape[0]:
        raise ValueError(f"{what}: phns must be [{pout.shape[0]}, L], got {tuple(phns.shape)}")
    spp = int(spp)
    if spp < 1:
        raise ValueError(f"{what}: states per phoneme must be >= 1, got {spp}")
    B, L = phns.shape
    fl = _score_lens(lens, B, pout.device, f"{what} frame")
    pl = _score_lens(phn_lens, B, pout.device, f"{what} phoneme")
    ids = phns.to(pout.device, torch.int64).contiguous()
    return fl, pl, ids, L, spp


class LatticeFn(torch.autograd.Function):
    """score [B] = log of the summed path likelihoods of the HMM or CTC chain (csrc/align.hip).
    The forward runs the alpha chain (and, when a gradient is wanted, the beta chain beside it);
    the backward is the occupancy pass with g = the incoming gradient."""

    @staticmethod
    def forward(ctx, pout, fl, ids, pl, spp, topo, blank):
        pout = _need(pout, "lattice pout")
        B, T, C = pout.shape
        L = ids.shape[1]
        limit = lib().mlvae_lattice_max_nodes()
        nodes = L * spp * (2 if topo == TOPO_CTC else 1) + (1 if topo == TOPO_CTC else 0)
        if nodes > limit:
            raise ValueError(f"lattice: {L} phonemes of {spp} states give a chain of {nodes} nodes, "
                             f"the kernel holds at most {limit}")
        need_beta = bool(ctx.needs_input_grad[0])
        nbytes = lib().mlvae_lattice_workspace_size(B, T, L, spp, topo)
        ws = torch.empty(max(nbytes // 4, 1), device=pout.device, dtype=torch.float32)
        score = torch.empty(B, device=pout.device, dtype=torch.float32)
        check(lib().mlvae_lattice_fb(B, T, C, L, _p(pout), C, _p(fl), ids.data_ptr(), _p(pl), spp, topo,
                                     blank, int(need_beta), _p(score), _p(ws), _ws_bytes(ws),
                                     _p(_md_err()), _stream()), "lattice_fb")
        if need_beta:
            ctx.save_for_backward(pout, fl, ids, pl, ws)
        ctx.cfg = (spp, topo, blank)
        return score

    @staticmethod
    def backward(ctx, g):
        pout, fl, ids, pl, ws = ctx.saved_tensors
        spp, topo, blank = ctx.cfg
        B, T, C = pout.shape
        g = _need(g, "lattice grad")
        dpout = torch.empty_like(pout)
        check(lib().mlvae_lattice_grad(B, T, C, ids.shape[1], _p(pout), C, _p(fl), ids.data_ptr(), _p(pl),
                                       spp, topo, blank, _p(g), _p(ws), _ws_bytes(ws), _p(dpout), C,
                                       _stream()), "lattice_grad")
        return dpout, None, None, None, None, None, None


def hmm_forward(pout, lens, phns, phn_lens, spp):
    """score [B]: log sum over the left-to-right HMM paths of exp(sum_t pout[b, t, state_t]) --
    the forward score SpeechBrain's HMMAligner trains on.  pout [B, T, C] log-probabilities, phns
    [B, L] phoneme ids (each expands into spp states of classes id * spp + j), lens / phn_lens the
    relative lengths.  Autograd: d score_b / d pout = the state occupancies.  An infeasible
    utterance or a bad id scores 0 and sets a bit of the device error word (raise_align_err)."""
    fl, pl, ids, _, spp = _lattice_args("hmm_forward", pout, lens, phns, phn_lens, spp)
    return LatticeFn.apply(pout, fl, ids, pl, spp, TOPO_HMM, 0)


def ctc_nll(pout, lens, phns, phn_lens, spp, blank):
    """nll [B] = -log p(targets | pout) of the CTC chain over the spp-expanded phonemes:
    F.ctc_loss(reduction='none', zero_infinity=True) per utterance, on log-probabilities pout.
    The gradient is the true partial derivative with respect to pout (minus the occupancies), not
    torch's, which folds the log-softmax backward in: chained through a log-softmax both agree."""
    fl, pl, ids, _, spp = _lattice_args("ctc_nll", pout, lens, phns, phn_lens, spp)
    blank = int(blank)
    if not 0 <= blank < pout.shape[2]:
        raise ValueError(f"ctc_nll: blank {blank} outside [0, {pout.shape[2]})")
    return -LatticeFn.apply(pout, fl, ids, pl, spp, TOPO_CTC, blank)


def hmm_viterbi(pout, lens, phns, phn_lens, spp):
    """(vscore [B] fp32, align [B, T] int32): the best HMM path's score (float64 sums, rounded
    once) and its state position per frame in [0, U_i), -1 past T_i; a tie keeps "stay".  No
    gradient; errors as hmm_forward's."""
    fl, pl, ids, L, spp = _lattice_args("hmm_viterbi", pout, lens, phns, phn_lens, spp)
    pout = _need(pout.detach(), "hmm_viterbi pout")
    B, T, C = pout.shape
    limit = lib().mlvae_lattice_max_nodes()
    if L * spp > limit:
        raise ValueError(f"hmm_viterbi: {L} phonemes of {spp} states, the kernel holds at most {limit} states")
    ws = _workspace(lib().mlvae_hmm_viterbi_workspace_size(B, T), "hmm_viterbi")
    vscore = torch.empty(B, device=pout.device, dtype=torch.float32)
    align = torch.empty(B, T, device=pout.device, dtype=torch.int32)
    check(lib().mlvae_hmm_viterbi(B, T, C, L, _p(pout), C, _p(fl), ids.data_ptr(), _p(pl), spp,
                                  _p(vscore), align.data_ptr(), _p(ws), _ws_bytes(ws), _p(_md_err()),
                                  _stream()), "hmm_viterbi")
    return vscore, align


def align_counts(align, lens, phns, phn_lens, spp, phn_ends, samples_per_frame):
    """int32 [B, 2] = (frames correct, T_i) per utterance of a Viterbi alignment (int32 [B, T] state
    positions): frame t is correct iff the phoneme of its state, phns[i, align[i, t] // spp], is
    the phoneme of the ground-truth segment that holds it -- the first k with t * samples_per_frame
    < phn_ends[i, k] (exclusive ends in samples), the last phoneme if none.  What
    AlignAccMetricStats.append_counts takes; stays on the device."""
    if align.dim() != 2 or align.dtype != torch.int32 or not align.is_cuda:
        raise TypeError(f"align_counts: align must be an int32 [B, T] HIP tensor, got {align.dtype} "
                        f"{tuple(align.shape)} on {align.device}")
    align = align.contiguous()
    B, T = align.shape
    if phns.dim() != 2 or phns.shape[0] != B or tuple(phn_ends.shape) != tuple(phns.shape):
        raise ValueError(f"align_counts: phns and phn_ends must be [{B}, L], got {tuple(phns.shape)} "
                         f"and {tuple(phn_ends.shape)}")
    spp, spf = int(spp), int(samples_per_frame)
    if spp < 1 or spf < 1:
        raise ValueError(f"align_counts: spp {spp} and samples_per_frame {spf} must be >= 1")
    L = phns.shape[1]
    fl = _score_lens(lens, B, align.device, "align_counts frame")
    pl = _score_lens(phn_lens, B, align.device, "align_counts phoneme")
    ids = phns.to(align.device, torch.int64).contiguous()
    ends = phn_ends.to(align.device, torch.int64).contiguous()
    counts = torch.zeros(B, 2, device=align.device, dtype=torch.int32)
    check(lib().mlvae_align_counts(B, T, L, align.data_ptr(), _p(fl), ids.data_ptr(), _p(pl), spp,
                                   ends.data_ptr(), spf, counts.data_ptr(), _stream()), "align_counts")
    return counts


# --------------------------------------------------------------------------- CTC evaluation (csrc/ctc_eval.hip)
def raise_ctc_eval_err():
    """Read the device error word's CTC-evaluation bits (one host sync) and clear them alone (the
    class and blank bits are the lattice's, worded for the evaluation)."""
    raise_err(_md_err(), "ctc_eval")


class LogSoftmaxFn(torch.autograd.Function):
    """y = log_softmax(x, dim=-1) over [.., C]."""

    @staticmethod
    def forward(ctx, x):
        x = _need(x, "log_softmax x")
        C = x.shape[-1]
        y = torch.empty_like(x)
        check(lib().mlvae_log_softmax_fwd(x.numel() // C, C, _p(x), _p(y), _stream()), "log_softmax_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        C = y.shape[-1]
        dy = _need(dy, "log_softmax grad")
        dx = torch.empty_like(y)
        check(lib().mlvae_log_softmax_bwd(y.numel() // C, C, _p(dy), _p(y), _p(dx), _stream()),
              "log_softmax_bwd")
        return dx


def log_softmax(x):
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"log_softmax: x must be [.., C] with C >= 1, got {tuple(x.shape)}")
    return LogSoftmaxFn.apply(x)


def _rows_ld(pout, what):
    """(tensor, ld) of a float32 HIP [B, T, C] whose rows lie ld >= C floats apart (a column slice
    of a wider contiguous tensor is taken as it is); anything else is made contiguous."""
    if pout.dim() != 3 or pout.shape[2] < 1:
        raise ValueError(f"{what}: pout must be [B, T, C] with C >= 1, got {tuple(pout.shape)}")
    if not (pout.is_cuda and pout.dtype == torch.float32):
        raise TypeError(f"{what} pout: expected a float32 HIP tensor, got {pout.dtype} on {pout.device} "
                        "(the HIP path has no CPU fallback)")
    B, T, C = pout.shape
    s0, s1, s2 = pout.stride()
    if B and T and s2 == 1 and s1 >= C and (s0 == T * s1 or B == 1):
        return pout, s1
    return pout.contiguous(), C


def _blank_arg(what, blank, C):
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f"{what}: blank {blank} outside [0, {C})")
    return blank


def ctc_greedy_decode(pout, lens, blank):
    """(pred [B, T] int32 padded with -1, pred_len [B] int32): SpeechBrain's ctc_greedy_decode for
    the whole batch on the device -- per frame t < T_i the argmax over the classes (a tie keeps the
    lowest), consecutive repeats merged, blanks dropped.  No gradient."""
    pout, ld = _rows_ld(pout.detach(), "ctc_greedy_decode")
    B, T, C = pout.shape
    blank = _blank_arg("ctc_greedy_decode", blank, C)
    fl = _score_lens(lens, B, pout.device, "ctc_greedy_decode frame")
    pred = torch.empty(B, T, device=pout.device, dtype=torch.int32)
    pred_len = torch.empty(B, device=pout.device, dtype=torch.int32)
    check(lib().mlvae_ctc_greedy_decode(B, T, C, _p(pout), ld, _p(fl), blank, pred.data_ptr(),
                                        pred_len.data_ptr(), _stream()), "ctc_greedy_decode")
    return pred, pred_len


def _ref_pair(what, phns, phn_lens, cnncls, cnncl_lens, dev):
    """refs int64 [B, 2, L] and ref_lens fp32 [B, 2] of the pronounced and the canonical sequences."""
    if phns.dim() != 2 or tuple(cnncls.shape) != tuple(phns.shape):
        raise ValueError(f"{what}: phns and cnncls must both be [B, L], got {tuple(phns.shape)} and "
                         f"{tuple(cnncls.shape)}")
    B = phns.shape[0]
    refs = torch.stack([phns.to(dev, torch.int64), cnncls.to(dev, torch.int64)], dim=1).contiguous()
    ref_lens = torch.stack([_score_lens(phn_lens, B, dev, f"{what} phoneme"),
                            _score_lens(cnncl_lens, B, dev, f"{what} canonical")], dim=1).contiguous()
    return refs, ref_lens


def edit_align(pred, pred_len, phns, phn_lens, cnncls, cnncl_lens):
    """(ali [B, 2, L] int32, ops [B, 2, 4] int32): the decoded sequences pred[i, :pred_len[i]]
    aligned by edit distance to the pronounced (index 0) and the canonical (index 1) phonemes.
    ali = the hypothesis token at every reference position, -1 for a deletion and past L_i
    (insertions dropped, align_sequences(ignore_insertion=True)); ops = (insertions, deletions,
    substitutions, L_i).  Tie rule: include/mlvae.h; the definition is tests/ctc_np.py."""
    if pred.dim() != 2 or pred.dtype != torch.int32 or not pred.is_cuda:
        raise TypeError(f"edit_align: pred must be an int32 [B, T] HIP tensor, got {pred.dtype} "
                        f"{tuple(pred.shape)} on {pred.device}")
    B, Tp = pred.shape
    if tuple(pred_len.shape) != (B,) or pred_len.dtype != torch.int32 or pred_len.device != pred.device:
        raise TypeError(f"edit_align: pred_len must be an int32 [{B}] tensor on {pred.device}")
    if phns.shape[0] != B:
        raise ValueError(f"edit_align: phns must be [{B}, L], got {tuple(phns.shape)}")
    pred, pred_len = pred.contiguous(), pred_len.contiguous()
    refs, ref_lens = _ref_pair("edit_align", phns, phn_lens, cnncls, cnncl_lens, pred.device)
    L = refs.shape[2]
    limit = lib().mlvae_edit_align_max_ref()
    if L > limit:
        raise ValueError(f"edit_align: a reference of {L} tokens, the kernel holds at most {limit}")
    ws = _workspace(lib().mlvae_edit_align_workspace_size(B, L, Tp), "edit_align")
    ali = torch.empty(B, 2, L, device=pred.device, dtype=torch.int32)
    ops_ = torch.empty(B, 2, 4, device=pred.device, dtype=torch.int32)
    check(lib().mlvae_edit_align(B, L, Tp, refs.data_ptr(), _p(ref_lens), pred.data_ptr(),
                                 pred_len.data_ptr(), ali.data_ptr(), ops_.data_ptr(), _p(ws),
                                 _ws_bytes(ws), _stream()), "edit_align")
    return ali, ops_


def ctc_md_counts(ali, phns, phn_lens, cnncls, cnncl_lens):
    """int32 [B, 8] per utterance from edit_align's ali [B, 2, L], over the alignment to the
    pronounced sequence, with pred_md = (ali != cnncl) (a deletion counts as a predicted
    mispronunciation) and gt_md = (phn != cnncl): (both correct, both mispronounced, missed, false
    alarm) as MDMetricStats counts them, then (canonical positions, of them recognised wrongly,
    mispronounced positions, of them recognised wrongly): per_scoring's correct_per / misp_per.
    Stays on the device; sequences of unequal length set a bit of the error word."""
    if ali.dim() != 3 or ali.shape[1] != 2 or ali.dtype != torch.int32 or not ali.is_cuda:
        raise TypeError(f"ctc_md_counts: ali must be an int32 [B, 2, L] HIP tensor, got {ali.dtype} "
                        f"{tuple(ali.shape)} on {ali.device}")
    B, _, L = ali.shape
    if tuple(phns.shape) != (B, L):
        raise ValueError(f"ctc_md_counts: phns must be [{B}, {L}], got {tuple(phns.shape)}")
    refs, ref_lens = _ref_pair("ctc_md_counts", phns, phn_lens, cnncls, cnncl_lens, ali.device)
    ali = ali.contiguous()
    counts = torch.zeros(B, 8, device=ali.device, dtype=torch.int32)
    check(lib().mlvae_ctc_md_counts(B, L, refs.data_ptr(), _p(ref_lens), ali.data_ptr(), counts.data_ptr(),
                                    _p(_md_err()), _stream()), "ctc_md_counts")
    return counts


def ctc_viterbi(pout, lens, phns, phn_lens, blank):
    """(vscore [B] fp32, boundary [B, T] int32, infeasible [B] int32): the best path of the CTC
    chain over phns (one state per phoneme) -- what the reference asks the ctc_segmentation package
    for.  boundary is 1 at frame 0 and at the first frame of every later phoneme (exactly L_i
    ones), 0 elsewhere, -1 past T_i; a chain without a path scores 0, sets infeasible and marks
    frames 0 .. min(L_i, T_i) - 1.  Tie order: stay, next, skip; the final blank over the last
    phoneme.  No gradient; a bad id sets a bit of the error word (raise_ctc_eval_err)."""
    pout, ld = _rows_ld(pout.detach(), "ctc_viterbi")
    B, T, C = pout.shape
    blank = _blank_arg("ctc_viterbi", blank, C)
    if phns.dim() != 2 or phns.shape[0] != B:
        raise ValueError(f"ctc_viterbi: phns must be [{B}, L], got {tuple(phns.shape)}")
    L = phns.shape[1]
    limit = lib().mlvae_lattice_max_nodes()
    if 2 * L + 1 > limit:
        raise ValueError(f"ctc_viterbi: {L} phonemes give a chain of {2 * L + 1} nodes, the kernel holds "
                         f"at most {limit}")
    fl = _score_lens(lens, B, pout.device, "ctc_viterbi frame")
    pl = _score_lens(phn_lens, B, pout.device, "ctc_viterbi phoneme")
    ids = phns.to(pout.device, torch.int64).contiguous()
    ws = _workspace(lib().mlvae_ctc_viterbi_workspace_size(B, T), "ctc_viterbi")
    vscore = torch.empty(B, device=pout.device, dtype=torch.float32)
    boundary = torch.empty(B, T, device=pout.device, dtype=torch.int32)
    infeasible = torch.empty(B, device=pout.device, dtype=torch.int32)
    check(lib().mlvae_ctc_viterbi(B, T, C, L, _p(pout), ld, _p(fl), ids.data_ptr(), _p(pl), blank,
                                  _p(vscore), boundary.data_ptr(), infeasible.data_ptr(), _p(ws),
                                  _ws_bytes(ws), _p(_md_err()), _stream()), "ctc_viterbi")
    return vscore, boundary, infeasible
