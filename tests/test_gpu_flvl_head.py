"""ops.flvl_md_head / mlvae_flvl_head_{fwd,bwd} (csrc/flvl.hip): the LSTM_FC recipe's fused head.

The oracle is torch fp64 on the same fp32 inputs: F.linear, the reference's
binary_cross_entropy_with_logits(..., pos_weight=...) expression (ref:src/models/LSTM_FC/
model.py:50-53) and autograd for dh / dw / db under a random dloss_e.  Bounds: the fp32
module-mode bounds of test_gpu_pi.py / test_gpu_sfl.py, outputs 1e-5 and gradients 1e-4,
relative-max.  pred, counts and reruns are compared exactly."""
import ctypes

import pytest
import torch
import torch.nn.functional as F_

from gpu_utils import P, need_gpu, rel_err, stream

pytestmark = pytest.mark.gpu

GRID_SWEEP = 65536  # frames one sweep of either capped grid covers (csrc/flvl.hip)


def _lens(B, g):
    """Mixed relative lengths: a full-length and a zero-length utterance where B allows."""
    lens = 0.1 + 0.85 * torch.rand(B, generator=g)
    lens[0] = 1.0
    if B >= 3:
        lens[1] = 0.0
    return lens


def _inputs(B, T, E, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return dict(h=torch.randn(B, T, E, generator=g), w=scale * torch.randn(2, E, generator=g),
                b=torch.randn(2, generator=g), labels=(torch.rand(B, T, generator=g) < 0.4).float(),
                lens=_lens(B, g), dloss=torch.randn(B, T, 2, generator=g))


def _oracle(a, pw):
    h, w, b = (a[k].double().requires_grad_(True) for k in ("h", "w", "b"))
    x = F_.linear(h, w, b)
    l = a["labels"].double()
    y = torch.stack([1 - l, l], dim=-1)
    loss = F_.binary_cross_entropy_with_logits(x, y, reduction="none",
                                               pos_weight=torch.tensor(pw, dtype=torch.float64))
    dh, dw, db = torch.autograd.grad(loss, (h, w, b), a["dloss"].double())
    return x.detach(), loss.detach(), dh, dw, db


def _valid(a):
    B, T = a["labels"].shape
    lim = a["lens"] * T  # fp32, as the kernels' valid_frames
    return torch.arange(T, dtype=torch.float32)[None, :] < lim[:, None]


def _host_counts(pred, labels, valid):
    p, g, v = pred.long(), labels.long(), valid.long()
    return torch.stack([((1 - p) * (1 - g) * v).sum(1), (p * g * v).sum(1), ((1 - p) * g * v).sum(1),
                        (p * (1 - g) * v).sum(1)], dim=1).int()


def _run(a, pw):
    from mlvae_hip import ops
    h, w, b = (a[k].cuda().requires_grad_(True) for k in ("h", "w", "b"))
    logits, loss_e, pred, counts = ops.flvl_md_head(h, w, b, a["labels"].cuda(), a["lens"].cuda(), pw)
    dh, dw, db = torch.autograd.grad(loss_e, (h, w, b), a["dloss"].cuda())
    return logits, loss_e, pred, counts, dh, dw, db


def _check(a, pw, tag):
    logits, loss_e, pred, counts, dh, dw, db = _run(a, pw)
    x, loss, rdh, rdw, rdb = _oracle(a, pw)
    errs = {"logits": rel_err(logits, x), "loss_e": rel_err(loss_e, loss), "dh": rel_err(dh, rdh),
            "dw": rel_err(dw, rdw), "db": rel_err(db, rdb)}
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["logits"] < 1e-5 and errs["loss_e"] < 1e-5, (tag, errs)
    assert max(errs["dh"], errs["dw"], errs["db"]) < 1e-4, (tag, errs)
    valid = _valid(a)
    lg = logits.cpu()
    want_pred = torch.where(valid, (lg[..., 1] > lg[..., 0]).int(), torch.full_like(pred.cpu(), -1))
    assert pred.dtype == torch.int32 and torch.equal(pred.cpu(), want_pred), tag
    assert counts.dtype == torch.int32 and counts.shape == (a["h"].shape[0], 4)
    assert torch.equal(counts.cpu(), _host_counts(want_pred.clamp(min=0), a["labels"], valid)), tag
    assert torch.equal(counts.cpu().sum(1), valid.sum(1).int())
    return errs


@pytest.mark.parametrize("pw", [(1.0, 1.0), (1.0, 10.0)])
@pytest.mark.parametrize("E", [1, 4, 64, 67])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 21), (5, 13), (1, 257)])
def test_parity_with_fp64(B, T, E, pw):
    need_gpu()
    a = _inputs(B, T, E, seed=1000 * B + 10 * T + E)
    _check(a, pw, f"B={B} T={T} N={B * T} E={E} pw={pw}")
    if B >= 3:  # the zero-length utterance: nothing counted, every frame past its end
        _, _, pred, counts, *_ = _run(a, pw)
        assert torch.equal(counts[1].cpu(), torch.zeros(4, dtype=torch.int32))
        assert bool((pred[1] == -1).all()) and bool((pred[0] >= 0).all())


@pytest.mark.parametrize("E", [259, 1028])
def test_wide_rows_take_a_second_column_pass(E):
    """More than 256 column units (scalar: E > 256; float4: E > 1024): the backward's second
    pass over the columns, two chunks of frames."""
    need_gpu()
    a = _inputs(2, 150, E, seed=E, scale=E ** -0.5)
    _check(a, (1.0, 10.0), f"B=2 T=150 N=300 E={E}")


def test_past_the_grid_caps_and_rerun_is_bit_equal():
    """N just past one sweep of the forward's and the backward's capped grids: the grid-stride
    loops take a second turn and the partials' second pass sums a full set of workgroups."""
    need_gpu()
    B, T, E = 3, GRID_SWEEP // 3 + 2, 4
    assert GRID_SWEEP < B * T < GRID_SWEEP + 16
    a = _inputs(B, T, E, seed=3)
    _check(a, (1.0, 10.0), f"B={B} T={T} N={B * T} E={E}")
    first, second = _run(a, (1.0, 10.0)), _run(a, (1.0, 10.0))
    for name, p, q in zip(("logits", "loss_e", "pred", "counts", "dh", "dw", "db"), first, second):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("B,T,E", [(5, 13, 67), (4, 300, 64)])
def test_rerun_is_bit_equal(B, T, E):
    need_gpu()
    a = _inputs(B, T, E, seed=11)
    first, second = _run(a, (1.0, 10.0)), _run(a, (1.0, 10.0))
    for name, p, q in zip(("logits", "loss_e", "pred", "counts", "dh", "dw", "db"), first, second):
        assert torch.equal(p, q), name


@pytest.mark.parametrize("big", [200.0, 1e4])
def test_saturated_logits_stay_finite(big):
    need_gpu()
    pw = (1.0, 10.0)
    for sign in (1.0, -1.0):
        a = _inputs(4, 19, 8, seed=5)
        a["w"].zero_()  # the logits are the bias exactly
        a["b"] = torch.tensor([sign * big, -sign * big])
        logits, loss_e, pred, counts, dh, dw, db = _run(a, pw)
        for name, t in (("logits", logits), ("loss_e", loss_e), ("dh", dh), ("dw", dw), ("db", db)):
            assert bool(torch.isfinite(t).all()), name
        x = logits.cpu()
        assert torch.equal(x, a["b"].expand_as(x))
        l = a["labels"]
        y = torch.stack([1 - l, l], dim=-1)
        # y = 1: pos_w softplus(-x) = pos_w |x| at x < 0, else 0; y = 0: softplus(x) = |x| at x > 0
        want = torch.where(y == 1, torch.tensor(pw) * x.abs() * (x < 0), x.abs() * (x > 0))
        assert torch.equal(loss_e.cpu(), want)
        _, _, rdh, rdw, rdb = _oracle(a, pw)
        assert rel_err(dw, rdw) < 1e-4 and rel_err(db, rdb) < 1e-4
        assert torch.equal(dh.cpu(), torch.zeros_like(a["h"]))  # w = 0


def test_ties_give_zero_and_padding_minus_one():
    need_gpu()
    a = _inputs(4, 23, 12, seed=9)
    a["w"][1] = a["w"][0]  # both classes the same row and bias: x1 == x0 in every frame
    a["b"][1] = a["b"][0]
    logits, _, pred, counts, *_ = _run(a, (1.0, 10.0))
    assert torch.equal(logits[..., 0], logits[..., 1])
    valid = _valid(a)
    assert torch.equal(pred.cpu(), torch.where(valid, 0, -1).int())
    assert torch.equal(counts.cpu(), _host_counts(torch.zeros_like(a["labels"]), a["labels"], valid))
    # ties in some frames only: h = 0 there, so both logits are the (equal) biases
    b = _inputs(4, 23, 12, seed=10)
    b["b"][1] = b["b"][0]
    b["h"][:, ::3] = 0.0
    logits, _, pred, _, *_ = _run(b, (1.0, 10.0))
    lg, valid = logits.cpu(), _valid(b)
    assert torch.equal(lg[:, ::3, 0], lg[:, ::3, 1]) and not torch.equal(lg[..., 0], lg[..., 1])
    assert torch.equal(pred.cpu(), torch.where(valid, (lg[..., 1] > lg[..., 0]).int(), -1).int())
    assert bool((pred.cpu()[:, ::3][valid[:, ::3]] == 0).all())


def test_only_loss_e_carries_gradient():
    need_gpu()
    from mlvae_hip import ops
    a = _inputs(2, 9, 6, seed=2)
    h, w, b = (a[k].cuda().requires_grad_(True) for k in ("h", "w", "b"))
    logits, loss_e, pred, counts = ops.flvl_md_head(h, w, b, a["labels"].cuda(), a["lens"].cuda(), (1, 10))
    assert loss_e.requires_grad and loss_e.grad_fn is not None
    for t in (logits, pred, counts):
        assert not t.requires_grad and t.grad_fn is None
    (loss_e.sum() + logits.sum()).backward()  # the logits add nothing
    _, _, rdh, rdw, rdb = _oracle(dict(a, dloss=torch.ones(2, 9, 2)), (1.0, 10.0))
    assert rel_err(h.grad, rdh) < 1e-4 and rel_err(w.grad, rdw) < 1e-4 and rel_err(b.grad, rdb) < 1e-4


def test_bad_label_sets_the_error_bit_in_valid_frames_only():
    need_gpu()
    from mlvae_hip import ops
    ops.raise_flvl_err()  # clean word
    a = _inputs(3, 10, 4, seed=4)
    a["lens"] = torch.tensor([1.0, 0.5, 0.3])
    a["labels"][1, 7] = 2.0  # past utterance 1's five frames
    a["labels"][2, 3] = 2.0  # past utterance 2's three frames
    _run(a, (1.0, 10.0))
    ops.raise_flvl_err()  # padded frames are not looked at
    a["labels"][1, 4] = 2.0  # its last valid frame
    _run(a, (1.0, 10.0))
    with pytest.raises(ValueError, match="outside"):
        ops.raise_flvl_err()
    ops.raise_flvl_err()  # the bit was cleared by the read


def test_c_entry_argument_checks():
    need_gpu()
    from mlvae_hip import _lib
    l = _lib.lib()
    B, T, E = 2, 5, 4
    f = lambda *s: torch.zeros(*s, device="cuda")
    h, w, b, lab, lens = f(B, T, E), f(2, E), f(2), f(B, T), torch.ones(B, device="cuda")
    logits, loss, dl = f(B, T, 2), f(B, T, 2), f(B, T, 2)
    pred = torch.zeros(B, T, dtype=torch.int32, device="cuda")
    counts = torch.full((B, 4), 7, dtype=torch.int32, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    dh, dw, db = f(B, T, E), f(2, E), f(2)
    fwd = lambda B_=B, T_=T, E_=E, h_=P(h), counts_=counts.data_ptr(): l.mlvae_flvl_head_fwd(
        B_, T_, E_, h_, P(w), P(b), P(lab), P(lens), 1.0, 10.0, P(logits), P(loss), pred.data_ptr(),
        counts_, err.data_ptr(), stream())
    need = l.mlvae_flvl_head_workspace_size(B, T, E)
    assert need == (2 * E + 2) * 4  # one workgroup's partials
    assert l.mlvae_flvl_head_workspace_size(1, GRID_SWEEP + 1, E) == 256 * (2 * E + 2) * 4  # capped
    assert l.mlvae_flvl_head_workspace_size(1, 10 * GRID_SWEEP, E) == 256 * (2 * E + 2) * 4
    assert l.mlvae_flvl_head_workspace_size(B, T, 0) == 0
    ws = torch.zeros(need // 4, device="cuda")
    bwd = lambda B_=B, T_=T, E_=E, dh_=P(dh), ws_=P(ws), n_=need: l.mlvae_flvl_head_bwd(
        B_, T_, E_, P(h), P(w), P(logits), P(lab), P(dl), 1.0, 10.0, dh_, P(dw), P(db), ws_,
        ctypes.c_size_t(n_), stream())
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert int(counts.sum()) == B * T  # zeroed by the entry, then one count per valid frame
    for call, what in ((lambda: fwd(h_=None), "null pointer"), (lambda: fwd(counts_=None), "null pointer"),
                       (lambda: fwd(E_=0), "E >= 1"), (lambda: fwd(B_=-1), "must be"),
                       (lambda: fwd(T_=-3), "must be"),
                       (lambda: bwd(dh_=None), "null pointer"), (lambda: bwd(ws_=None), "null pointer"),
                       (lambda: bwd(E_=-2), "E >= 1"), (lambda: bwd(B_=-1), "must be"),
                       (lambda: bwd(n_=need - 1), "workspace")):
        assert call() == 1
        assert what in _lib.last_error(), (what, _lib.last_error())
    # N = 0: a no-op that succeeds, whatever the pointers
    assert fwd(B_=0) == 0 and fwd(T_=0, h_=None) == 0 and bwd(B_=0) == 0 and bwd(T_=0, dh_=None) == 0
    torch.cuda.synchronize()
