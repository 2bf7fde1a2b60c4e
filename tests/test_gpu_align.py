"""The aligner's sequence-lattice kernels (csrc/align.hip) against the float64 oracle
tests/hmm_np.py, fp32, at the bounds the module-mode fp32 ops are held to
(test_gpu_upstream_recipes.py): 1e-5 relative-max on outputs and scores, 1e-4 relative-max on
gradients.  Viterbi paths, Viterbi scores (float64 sums rounded once) and the accuracy counts are
exact.  The HMM gradient is compared at dpout; the CTC gradient at the logits x with
pout = log_softmax(x), against torch's CPU ctc_loss in float64 (torch's CTC backward folds the
log-softmax in, so the two agree only there).

Shapes are the smallest at which each mechanism can break: chains across the lane boundaries
(64 lanes x 1, 2, 4, 8, 16 nodes per lane), T_b = U_b (a single path) and U_b + 1, lengths on the
half-to-even rule, repeated phonemes, peaky inputs, and the recipe-like B = 4, T = 200, L = 20,
spp = 3.  The data-error paths (short utterance, id out of range, CTC target equal to blank) are
ordinary validation: the launch returns 0, the bits raise through ops.raise_align_err()."""
import functools

import numpy as np
import pytest
import torch

import hmm_np
from gpu_utils import need_gpu, rel_err

pytestmark = pytest.mark.gpu

SCORE_TOL, GRAD_TOL = 1e-5, 1e-4


def _pout(B, T, C, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(B, T, C, generator=g) * scale, -1)


def _phns(B, L, hi, seed):
    return torch.randint(0, hi, (B, L), generator=torch.Generator().manual_seed(seed))


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _gpu_lattice(pout, lens, phns, phn_lens, spp, topo, blank, w):
    """(score [B], dpout for the upstream gradient w) from the ops."""
    from mlvae_hip import ops
    p = pout.cuda().requires_grad_(True)
    if topo == hmm_np.HMM:
        s = ops.hmm_forward(p, lens.cuda(), phns.cuda(), phn_lens.cuda(), spp)
    else:
        s = -ops.ctc_nll(p, lens.cuda(), phns.cuda(), phn_lens.cuda(), spp, blank)
    (s * w.cuda()).sum().backward()
    return s.detach().cpu(), p.grad.cpu()


def _check_lattice(name, pout, lens, phns, phn_lens, spp, topo, blank=None, want_ok=None):
    B, T, C = pout.shape
    w = torch.linspace(0.5, 1.5, B)
    score, dp = _gpu_lattice(pout, lens, phns, phn_lens, spp, topo, blank, w)
    ref_s, ref_dp, ok = hmm_np.lattice_batch(pout.numpy(), lens.numpy(), phns.numpy(), phn_lens.numpy(),
                                             spp, topo, blank)
    if want_ok is not None:
        assert ok.tolist() == want_ok
    ref_dp = torch.from_numpy(ref_dp) * w.double()[:, None, None]
    es, eg = rel_err(score, torch.from_numpy(ref_s)), rel_err(dp, ref_dp)
    print(f"{name}: score rel {es:.2e}, dpout rel {eg:.2e}")
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(dp).all())
    assert es < SCORE_TOL and eg < GRAD_TOL
    # exact zeros: frames past T_b, classes without a node, utterances without a score
    assert bool((dp[ref_dp == 0] == 0).all())
    for b in range(B):
        if not ok[b]:
            assert score[b] == 0 and not bool(dp[b].any())
    return score, dp, ref_s


def _check_viterbi(name, pout, lens, phns, phn_lens, spp):
    from mlvae_hip import ops
    vs, al = ops.hmm_viterbi(pout.cuda(), lens.cuda(), phns.cuda(), phn_lens.cuda(), spp)
    ref_vs, ref_al = hmm_np.viterbi_batch(pout.numpy(), lens.numpy(), phns.numpy(), phn_lens.numpy(), spp)
    assert al.dtype == torch.int32 and vs.dtype == torch.float32
    assert np.array_equal(al.cpu().numpy(), ref_al), name
    assert np.array_equal(vs.cpu().numpy(), ref_vs.astype(np.float32)), name
    return vs.cpu(), al.cpu()


# --------------------------------------------------------------------------- chain length
@pytest.mark.parametrize("L,spp", [(1, 1), (2, 1), (63, 1), (64, 1), (65, 1), (129, 1), (20, 3), (180, 3)])
def test_chain_lengths_single_path_and_one_spare_frame(L, spp):
    need_gpu()
    from mlvae_hip import ops
    U = L * spp
    T, C = U + 1, 123 if spp == 3 else 50
    pout = _pout(2, T, C, 100 + U)
    phns = _phns(2, L, C // spp, 200 + U)
    lens, ones = _f32([U / T, 1.0]), torch.ones(2)
    assert [hmm_np.round_len(v, T) for v in lens.numpy()] == [U, T]
    score, _, _ = _check_lattice(f"hmm L={L} spp={spp}", pout, lens, phns, ones, spp, hmm_np.HMM,
                                 want_ok=[True, True])
    vs, al = _check_viterbi(f"viterbi L={L} spp={spp}", pout, lens, phns, ones, spp)
    # T_b = U_b: a single path -- score = Viterbi score = the diagonal sum
    cls = hmm_np.expand(phns[0].numpy(), spp)
    diag = 0.0
    for v in pout[0, torch.arange(U), torch.from_numpy(cls)].double().tolist():
        diag += v  # in frame order, as the kernel adds
    assert al[0, :U].tolist() == list(range(U)) and al[0, U] == -1
    assert vs[0].item() == float(np.float32(diag))
    assert abs(score[0].item() - diag) <= SCORE_TOL * abs(diag)
    ops.raise_align_err()  # nothing set


@pytest.mark.parametrize("L,spp", [(1, 1), (64, 1), (129, 1), (20, 3), (260, 1)])
def test_ctc_chain_lengths(L, spp):
    need_gpu()
    U = L * spp
    C = 123 if spp == 3 else 50
    blank = C - 1
    phns = _phns(2, L, (C - 1) // spp, 300 + U)
    rep = int((hmm_np.expand(phns[0].numpy(), spp)[1:] == hmm_np.expand(phns[0].numpy(), spp)[:-1]).sum())
    T = U + rep + 3
    pout = _pout(2, T, C, 400 + U)
    lens = _f32([(U + rep) / T, 1.0])  # utterance 0 has exactly the frames its targets need
    assert hmm_np.round_len(lens[0].item(), T) == U + rep
    _check_lattice(f"ctc L={L} spp={spp}", pout, lens, phns, torch.ones(2), spp, hmm_np.CTC, blank,
                   want_ok=[True, True])


# --------------------------------------------------------------------------- mixed batch
def _mixed():
    T, C, L = 40, 123, 4
    pout = _pout(4, T, C, 7)
    phns = torch.tensor([[1, 1, 2, 1], [3, 4, 0, 0], [5, 6, 5, 7], [8, 8, 9, 0]])
    lens = _f32([1.0, 0.0625, 0.0875, 0.5])         # T lens = 40, 2.5 -> 2, 3.5 -> 4, 20
    phn_lens = _f32([1.0, 0.625, 0.875, 0.75])      # L phn_lens = 4, 2.5 -> 2, 3.5 -> 4, 3
    assert np.float32(T) * lens.numpy()[1] == 2.5 and np.float32(T) * lens.numpy()[2] == 3.5
    assert [hmm_np.round_len(v, T) for v in lens.numpy()] == [40, 2, 4, 20]
    assert [hmm_np.round_len(v, L) for v in phn_lens.numpy()] == [4, 2, 4, 3]
    return pout, lens, phns, phn_lens


def test_mixed_batch_hmm_and_ctc():
    need_gpu()
    from mlvae_hip import ops
    pout, lens, phns, phn_lens = _mixed()
    _check_lattice("mixed hmm", pout, lens, phns, phn_lens, 1, hmm_np.HMM, want_ok=[True] * 4)
    _check_viterbi("mixed viterbi", pout, lens, phns, phn_lens, 1)
    _check_lattice("mixed ctc", pout, lens, phns, phn_lens, 1, hmm_np.CTC, 122, want_ok=[True] * 4)
    ops.raise_align_err()


def test_ctc_infeasible_is_zero_and_no_error():
    need_gpu()
    from mlvae_hip import ops
    pout, lens, phns, phn_lens = _mixed()
    phns = phns.clone()
    phns[2] = torch.tensor([5, 5, 5, 5])  # 4 equal targets need 7 frames, the utterance has 4
    _check_lattice("ctc infeasible", pout, lens, phns, phn_lens, 1, hmm_np.CTC, 122,
                   want_ok=[True, True, False, True])
    ops.raise_align_err()  # zero_infinity, not an error


def test_peaky_inputs_stay_finite():
    need_gpu()
    B, T, C, L, spp = 2, 30, 20, 6, 2
    pout = _pout(B, T, C, 9, scale=20.0)
    assert float(pout.min()) < -60
    phns = _phns(B, L, 9, 10)
    lens, phn_lens = _f32([1.0, 0.8]), _f32([1.0, 5 / 6])
    _check_lattice("peaky hmm", pout, lens, phns, phn_lens, spp, hmm_np.HMM, want_ok=[True, True])
    _check_lattice("peaky ctc", pout, lens, phns, phn_lens, spp, hmm_np.CTC, 19, want_ok=[True, True])
    _check_viterbi("peaky viterbi", pout, lens, phns, phn_lens, spp)


# --------------------------------------------------------------------------- mid case
@functools.lru_cache(maxsize=None)
def _mid():
    B, T, C, L = 4, 200, 123, 20
    return (_pout(B, T, C, 21), _f32([1.0, 0.9, 0.75, 0.6]), _phns(B, L, 40, 22),
            _f32([1.0, 0.8, 0.9, 1.0]))


def test_mid_case_hmm():
    need_gpu()
    pout, lens, phns, phn_lens = _mid()
    _check_lattice("mid hmm", pout, lens, phns, phn_lens, 3, hmm_np.HMM, want_ok=[True] * 4)
    _check_viterbi("mid viterbi", pout, lens, phns, phn_lens, 3)


def test_mid_case_ctc():
    need_gpu()
    pout, lens, phns, phn_lens = _mid()
    _check_lattice("mid ctc", pout, lens, phns, phn_lens, 3, hmm_np.CTC, 122, want_ok=[True] * 4)


def test_ctc_gradient_at_the_logits_against_torch():
    need_gpu()
    from mlvae_hip import ops
    pout, lens, phns, phn_lens = _mid()
    B, T, C = pout.shape
    spp, blank = 3, 122
    x0 = torch.randn(B, T, C, generator=torch.Generator().manual_seed(23))
    w = torch.linspace(0.5, 1.5, B)
    x = x0.cuda().requires_grad_(True)
    nll = ops.ctc_nll(torch.log_softmax(x, -1), lens.cuda(), phns.cuda(), phn_lens.cuda(), spp, blank)
    (nll * w.cuda()).sum().backward()
    xr = x0.double().requires_grad_(True)
    Tb = torch.tensor([hmm_np.round_len(v, T) for v in lens.numpy()])
    Lb = [hmm_np.round_len(v, phns.shape[1]) for v in phn_lens.numpy()]
    tg = torch.zeros(B, phns.shape[1] * spp, dtype=torch.int64)
    for b in range(B):
        tg[b, :Lb[b] * spp] = torch.from_numpy(hmm_np.expand(phns[b, :Lb[b]].numpy(), spp))
    ref = torch.nn.functional.ctc_loss(torch.log_softmax(xr, -1).transpose(0, 1), tg, Tb,
                                       torch.tensor(Lb) * spp, blank=blank, reduction="none",
                                       zero_infinity=True)
    (ref * w.double()).sum().backward()
    es, eg = rel_err(nll, ref), rel_err(x.grad, xr.grad)
    print(f"ctc vs torch: nll rel {es:.2e}, dx rel {eg:.2e}")
    assert es < SCORE_TOL and eg < GRAD_TOL


def test_rerun_is_bit_identical():
    need_gpu()
    pout, lens, phns, phn_lens = _mid()
    w = torch.linspace(0.5, 1.5, 4)
    for topo, blank in ((hmm_np.HMM, None), (hmm_np.CTC, 122)):
        s1, d1 = _gpu_lattice(pout, lens, phns, phn_lens, 3, topo, blank, w)
        s2, d2 = _gpu_lattice(pout, lens, phns, phn_lens, 3, topo, blank, w)
        assert torch.equal(s1, s2) and torch.equal(d1, d2)


# --------------------------------------------------------------------------- Viterbi ties
def test_viterbi_tie_rule_decides_an_all_equal_input():
    need_gpu()
    B, T, C, L, spp = 2, 70, 12, 11, 3     # 33 states; a second utterance of 66 states over 2 lanes
    pout = torch.full((B, T, C * spp), float(-np.log(C * spp)))
    phns = _phns(B, 2 * L, C, 31)
    lens, phn_lens = _f32([0.5, 1.0]), _f32([0.5, 1.0])
    vs, al = _check_viterbi("tie", pout, lens, phns, phn_lens, spp)
    assert al[0, :35].tolist() == list(range(33)) + [32, 32]  # climbs first, rests at the end
    assert al[1].tolist() == list(range(66)) + [65] * 4


# --------------------------------------------------------------------------- accuracy counts
def test_align_counts_are_exact():
    need_gpu()
    from mlvae_hip import ops
    B, T, L, spp, spf = 3, 50, 6, 3, 320
    g = torch.Generator().manual_seed(41)
    phns = _phns(B, L, 5, 42)              # few ids: repeats inside an utterance
    lens, phn_lens = _f32([1.0, 0.8, 0.5]), _f32([1.0, 5 / 6, 0.5])
    Tb = [hmm_np.round_len(v, T) for v in lens.numpy()]
    Lb = [hmm_np.round_len(v, L) for v in phn_lens.numpy()]
    ends = torch.zeros(B, L, dtype=torch.int64)
    truth = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        cut = torch.sort(torch.randperm(Tb[b] - 1, generator=g)[:Lb[b] - 1] + 1).values.tolist() + [Tb[b]]
        ends[b, :Lb[b]] = torch.tensor(cut) * spf
        start = 0
        for k, e in enumerate(cut):
            truth[b, start:e] = k * spp + (torch.arange(e - start) % spp).to(torch.int32)
            start = e
    got = ops.align_counts(truth.cuda(), lens.cuda(), phns.cuda(), phn_lens.cuda(), spp, ends.cuda(), spf)
    assert got.dtype == torch.int32 and got.cpu().tolist() == [[t, t] for t in Tb]  # 100 %
    # a random alignment, and the Viterbi one of random posteriors
    rnd = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        rnd[b, :Tb[b]] = torch.randint(0, Lb[b] * spp, (Tb[b],), generator=g).to(torch.int32)
    pout = _pout(B, T, 5 * spp, 43)
    _, vit = ops.hmm_viterbi(pout.cuda(), lens.cuda(), phns.cuda(), phn_lens.cuda(), spp)
    for al in (rnd, vit.cpu()):
        got = ops.align_counts(al.cuda(), lens.cuda(), phns.cuda(), phn_lens.cuda(), spp, ends.cuda(), spf)
        want = hmm_np.align_counts(al.numpy(), lens.numpy(), phns.numpy(), phn_lens.numpy(), spp,
                                   ends.numpy(), spf)
        assert got.cpu().tolist() == want.tolist()
        assert 0 < want[:, 0].sum() < sum(Tb)


# --------------------------------------------------------------------------- error bits
def _err_word():
    from mlvae_hip import ops
    return int(ops._md_err().item())


def test_error_bits_raise_only_through_raise_align_err():
    need_gpu()
    from mlvae_hip import ops
    B, T, C, L = 2, 12, 10, 4
    pout = _pout(B, T, C, 51).cuda()
    ones = torch.ones(B).cuda()
    phns = torch.tensor([[1, 2, 3, 4], [0, 1, 0, 1]])
    ops.raise_align_err()
    base = _err_word()
    mask = ops.ALIGN_ERR_SHORT | ops.ALIGN_ERR_CLASS | ops.ALIGN_ERR_BLANK
    assert base & mask == 0

    def expect(bit, match, run):
        out = run()  # the launch itself returns 0: nothing raises here
        assert _err_word() & mask == bit
        with pytest.raises(AssertionError, match=match):
            ops.raise_align_err()
        assert _err_word() == base  # cleared, the other bits untouched
        ops.raise_align_err()
        return out

    # a short utterance: 3 frames for 4 states
    short = torch.tensor([1.0, 0.25]).cuda()
    s = expect(ops.ALIGN_ERR_SHORT, "fewer frames",
               lambda: ops.hmm_forward(pout, short, phns.cuda(), ones, 1))
    ref, _, ok = hmm_np.lattice_batch(pout.cpu().numpy(), [1.0, 0.25], phns.numpy(), [1.0, 1.0], 1, hmm_np.HMM)
    assert ok.tolist() == [True, False] and s[1] == 0 and rel_err(s, torch.from_numpy(ref)) < SCORE_TOL
    vs, al = expect(ops.ALIGN_ERR_SHORT, "fewer frames",
                    lambda: ops.hmm_viterbi(pout, short, phns.cuda(), ones, 1))
    assert vs[1] == 0 and bool((al[1] == -1).all()) and bool((al[0] >= 0).all())
    # an id whose state class is past C (spp 3: class 3 * 3 + 1 = 10), a negative one, and id = C
    good = torch.tensor([[1, 2, 0, 2], [0, 1, 0, 1]])
    for bad, spp in ((3, 3), (-1, 1), (C, 1)):
        ids = good.clone()
        ids[1, 2] = bad
        s = expect(ops.ALIGN_ERR_CLASS, "outside",
                   lambda: ops.hmm_forward(pout, ones, ids.cuda(), ones, spp))
        assert s[1] == 0 and s[0] != 0
    # a CTC target equal to blank
    nll = expect(ops.ALIGN_ERR_BLANK, "blank", lambda: ops.ctc_nll(pout, ones, phns.cuda(), ones, 1, 4))
    assert nll[0] == 0 and nll[1] != 0
    # the gradient of an utterance in error is exactly 0
    p = pout.clone().requires_grad_(True)
    ops.hmm_forward(p, short, phns.cuda(), ones, 1).sum().backward()
    assert not bool(p.grad[1].any()) and bool(p.grad[0].any())
    with pytest.raises(AssertionError, match="fewer frames"):
        ops.raise_align_err()


def test_status_errors_beyond_the_chain_limit():
    need_gpu()
    from mlvae_hip import ops
    from mlvae_hip._lib import lib
    assert lib().mlvae_lattice_max_nodes() == 1024
    pout, ones = _pout(1, 4, 6, 61).cuda(), torch.ones(1).cuda()
    phns = torch.zeros(1, 1025, dtype=torch.int64).cuda()
    with pytest.raises(ValueError, match="at most 1024"):
        ops.hmm_forward(pout, ones, phns, ones, 1)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.ctc_nll(pout, ones, phns[:, :512], ones, 1, 5)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.hmm_viterbi(pout, ones, phns[:, :342], ones, 3)


# --------------------------------------------------------------------------- centre + log-softmax
@pytest.mark.parametrize("shape", [(3, 17, 123), (2, 5, 7)])
def test_center_log_softmax_forward_and_backward(shape):
    need_gpu()
    from mlvae_hip import ops
    g = torch.Generator().manual_seed(71)
    x0 = torch.randn(*shape, generator=g) * 3 + 1.5  # every row non-zero: the mean is unmasked
    dy = torch.randn(*shape, generator=g)
    x = x0.cuda().requires_grad_(True)
    y = ops.center_log_softmax(x)
    (y * dy.cuda()).sum().backward()
    xr = x0.double().requires_grad_(True)
    yr = torch.log_softmax(xr - xr.mean(1).unsqueeze(1), -1)
    (yr * dy.double()).sum().backward()
    ey, eg = rel_err(y, yr), rel_err(x.grad, xr.grad)
    print(f"center_log_softmax {shape}: y rel {ey:.2e}, dx rel {eg:.2e}")
    assert ey < SCORE_TOL and eg < GRAD_TOL


# --------------------------------------------------------------------------- the aligner module
def test_hmm_aligner_reductions():
    need_gpu()
    from modules.hmm_aligner import HMMAligner
    pout, lens, phns, phn_lens = _mixed()
    ref, _, _ = hmm_np.lattice_batch(pout.numpy(), lens.numpy(), phns.numpy(), phn_lens.numpy(), 1, hmm_np.HMM)
    Tb, Ub = np.array([40, 2, 4, 20]), np.array([4, 2, 4, 3])
    args = (pout.cuda(), lens.cuda(), phns.cuda(), phn_lens.cuda())
    for red, iln, tln, want in (("none", False, False, ref), ("mean", True, False, (ref / Tb).mean()),
                                ("sum", False, True, (ref / Ub).sum()),
                                ("mean", True, True, (ref / Tb / Ub).mean())):
        a = HMMAligner(1, red, iln, tln)
        got = a(*args, "forward")
        assert rel_err(got, torch.as_tensor(want)) < SCORE_TOL
        vs, al = a(*args, "viterbi")
        assert vs.shape == got.shape and al.shape == (4, 40)
