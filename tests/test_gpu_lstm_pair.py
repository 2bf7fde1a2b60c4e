"""The paired unidirectional recurrence (mlvae_lstm_pair_fwd / _bwd, ops.lstm_pair): two independent
nn.LSTM(batch_first=True) stacks of one shape in one launch per layer (the joint recipes'
recogniser and detector, ref:src/modules/phoneme_recognizer.py:13, boundary_detector.py:19).

* the entry points against mlvae_lstm1_fwd / _bwd on each stack, bit for bit: per (stack, batch
  group) the same kernel performs the same arithmetic in the same order, only strides and the
  source of the time index differ, so any difference is a bug in the split of `dir`'s two roles;
* both halves against fp64 torch.nn.LSTM (a half that kept the reverse time order fails at order
  one), within tests/test_gpu_lstm_module.py's bounds;
* ops.lstm_pair (L = 2) against two fp64 nn.LSTMs: outputs, input gradient, every parameter
  gradient; one output outside the loss; an input without gradient;
* refusals."""
import ctypes

import pytest
import torch

from gpu_utils import P, need_gpu, norm_rel, stream

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1


def _workspace(B, H, prec):
    from mlvae_hip._lib import SZ, check, lib
    xb = SZ()
    check(lib().mlvae_lstm_workspace_size(B, H, prec, ctypes.byref(xb)))
    xbuf = torch.zeros(xb.value // 4 + 4, device="cuda", dtype=torch.float32)
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    return xbuf, xbuf.numel() * 4, err


def _single(prec, B, T, H, w, G_in, dy):
    """mlvae_lstm1_fwd / _bwd (with and without the bf16 outputs) on one stack."""
    from mlvae_hip._lib import check, lib
    xbuf, xbytes, err = _workspace(B, H, prec)
    N = B * T
    G = G_in.clone()
    Cs, Y = torch.empty(N, H, device="cuda"), torch.empty(N, H, device="cuda")
    Yb = torch.empty(N, H, device="cuda", dtype=torch.bfloat16)
    check(lib().mlvae_lstm1_fwd(prec, B, T, H, P(w), P(G), P(Cs), P(Y), Yb.data_ptr(), P(xbuf), xbytes,
                                P(err), stream()), "lstm1_fwd")
    act = G.clone()
    dG = G.clone()
    check(lib().mlvae_lstm1_bwd(prec, B, T, H, P(w), P(dG), P(Cs), P(dy), None, P(xbuf), xbytes, P(err),
                                stream()), "lstm1_bwd")
    G2 = act.clone()
    dGb = torch.empty(N, 4 * H, device="cuda", dtype=torch.bfloat16)
    check(lib().mlvae_lstm1_bwd(prec, B, T, H, P(w), P(G2), P(Cs), P(dy), dGb.data_ptr(), P(xbuf), xbytes,
                                P(err), stream()), "lstm1_bwd (bf16 dG)")
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    return dict(act=act, Cs=Cs, Y=Y, Yb=Yb, dG=dG, dGb=dGb)


def _pair(prec, B, T, H, wa, wb, Ga, Gb, dya, dyb):
    """mlvae_lstm_pair_fwd / _bwd on the interleaved buffers; the results half by half."""
    from mlvae_hip._lib import check, lib
    xbuf, xbytes, err = _workspace(B, H, prec)
    N = B * T
    G = torch.cat([Ga, Gb], dim=1).contiguous()
    dy = torch.cat([dya, dyb], dim=1).contiguous()
    Cs, Y = torch.empty(N, 2 * H, device="cuda"), torch.empty(N, 2 * H, device="cuda")
    Yb = torch.empty(N, 2 * H, device="cuda", dtype=torch.bfloat16)
    check(lib().mlvae_lstm_pair_fwd(prec, B, T, H, P(wa), P(wb), P(G), P(Cs), P(Y), Yb.data_ptr(), P(xbuf),
                                    xbytes, P(err), stream()), "lstm_pair_fwd")
    act = G.clone()
    dG = G.clone()
    check(lib().mlvae_lstm_pair_bwd(prec, B, T, H, P(wa), P(wb), P(dG), P(Cs), P(dy), None, P(xbuf), xbytes,
                                    P(err), stream()), "lstm_pair_bwd")
    G2 = act.clone()
    dGb = torch.empty(N, 8 * H, device="cuda", dtype=torch.bfloat16)
    check(lib().mlvae_lstm_pair_bwd(prec, B, T, H, P(wa), P(wb), P(G2), P(Cs), P(dy), dGb.data_ptr(), P(xbuf),
                                    xbytes, P(err), stream()), "lstm_pair_bwd (bf16 dG)")
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    halves = []
    for s in range(2):
        g = slice(4 * H * s, 4 * H * (s + 1))
        h = slice(H * s, H * (s + 1))
        halves.append(dict(act=act[:, g], Cs=Cs[:, h], Y=Y[:, h], Yb=Yb[:, h], dG=dG[:, g], dGb=dGb[:, g]))
    return halves


# the smallest shapes that reach each code path of the batch-group kernels
CASES = [
    (F32, 16, 3, 7),     # HJ 16, NJ 1
    (F32, 12, 17, 5),    # HJ 4; two batch groups, the second holding one utterance
    (F32, 40, 2, 9),     # HJ 8, NJ 5
    (F32, 528, 2, 4),    # stepwise BPTT (H > 512); forward with NJ 33
    (BF16, 128, 3, 9),   # reduce-scatter BPTT, NTW 2; forward io wave
    (BF16, 64, 18, 6),   # non-reduce-scatter bf16 BPTT; two batch groups
    (BF16, 512, 2, 6),   # the recipes' width; reduce-scatter NJ 32; XCD-local forward
]


@pytest.mark.parametrize("prec,H,B,T", CASES)
def test_pair_equals_two_single_stacks_bit_for_bit(prec, H, B, T):
    need_gpu()
    g = torch.Generator().manual_seed(100 + H + B)
    N = B * T
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    Ga, Gb = r(N, 4 * H), r(N, 4 * H)
    wa, wb = r(4 * H, H) / H ** 0.5, r(4 * H, H) / H ** 0.5
    dya, dyb = r(N, H), r(N, H)
    ref = [_single(prec, B, T, H, wa, Ga, dya), _single(prec, B, T, H, wb, Gb, dyb)]
    got = _pair(prec, B, T, H, wa, wb, Ga, Gb, dya, dyb)
    for s in range(2):
        for k in ("act", "Cs", "Y", "Yb", "dG", "dGb"):
            assert torch.equal(got[s][k], ref[s][k]), (s, k)
    # the halves are different stacks, not one computed twice
    assert not torch.equal(got[0]["Y"], got[1]["Y"])


def test_both_halves_run_forward_in_time():
    """fp32, H = 16: each half against fp64 nn.LSTM; dG checked through dx = dG W_ih and the bias
    gradient (its column sums), which autograd gives for the fp64 module."""
    need_gpu()
    B, T, H, I = 3, 7, 16, 8
    torch.manual_seed(11)
    refs = [torch.nn.LSTM(I, H, 1, batch_first=True).double() for _ in range(2)]
    x = torch.randn(B, T, I).double()
    cots = [torch.randn(B, T, H).double() for _ in range(2)]
    Gs, want = [], []
    for m, cot in zip(refs, cots):
        xr = x.clone().requires_grad_(True)
        out = m(xr)[0]
        (out * cot).sum().backward()
        want.append((out.detach(), xr.grad, m.bias_ih_l0.grad))
        Gs.append((x.reshape(-1, I) @ m.weight_ih_l0.detach().t() + m.bias_ih_l0.detach()
                   + m.bias_hh_l0.detach()).float().cuda())
    w = [m.weight_hh_l0.detach().float().cuda().contiguous() for m in refs]
    dys = [c.reshape(-1, H).float().cuda() for c in cots]
    got = _pair(F32, B, T, H, w[0], w[1], Gs[0], Gs[1], dys[0], dys[1])
    for s in range(2):
        out, dx, db = want[s]
        e_out = norm_rel(got[s]["Y"].reshape(B, T, H), out)
        dG = got[s]["dG"].double().cpu()
        e_dx = norm_rel((dG @ refs[s].weight_ih_l0.detach()).reshape(B, T, I), dx)
        e_db = norm_rel(dG.sum(0), db)
        print(f"half {s}: out {e_out:.2e} dx {e_dx:.2e} db {e_db:.2e}")
        assert e_out < 1e-5 and e_dx < 1e-4 and e_db < 1e-4, (s, e_out, e_dx, e_db)


def _pair_modules(I, H, L, seed):
    torch.manual_seed(seed)
    refs = [torch.nn.LSTM(I, H, L, batch_first=True).double() for _ in range(2)]
    mine = []
    for m in refs:
        c = torch.nn.LSTM(I, H, L, batch_first=True)
        c.load_state_dict({k: v.float() for k, v in m.state_dict().items()})
        mine.append(c.cuda())
    return refs, mine


@pytest.mark.parametrize("prec,tol_out,tol_grad,H,B,T", [("fp32", 1e-5, 1e-4, 16, 3, 7),
                                                         ("bf16", 1e-2, 3e-2, 128, 3, 9)])
@pytest.mark.parametrize("variant", ["both", "only_a", "no_input_grad"])
def test_ops_lstm_pair_matches_two_nn_lstms(prec, tol_out, tol_grad, H, B, T, variant):
    need_gpu()
    from mlvae_hip import ops
    I, L = 8, 2
    refs, mine = _pair_modules(I, H, L, seed=21)
    x = torch.randn(B, T, I)
    cots = [torch.randn(B, T, H), torch.randn(B, T, H)]
    used = (0,) if variant == "only_a" else (0, 1)
    xd = x.cuda().requires_grad_(variant != "no_input_grad")
    prev = ops.get_precision()
    ops.set_precision(prec)
    try:
        outs = ops.lstm_pair(xd, mine[0], mine[1], True)
        sum((outs[s] * cots[s].cuda()).sum() for s in used).backward()
    finally:
        ops.set_precision(prev)
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    routs = [m(xr)[0] for m in refs]
    sum((routs[s] * cots[s].double()).sum() for s in used).backward()
    errs = {}
    for s in range(2):
        assert outs[s].shape == (B, T, H)
        errs[f"out{s}"] = norm_rel(outs[s], routs[s])
        assert errs[f"out{s}"] < tol_out, (s, errs)
    for s in used:
        for (k, a), (_, b) in zip(mine[s].named_parameters(), refs[s].named_parameters()):
            errs[f"{s}.{k}"] = norm_rel(a.grad, b.grad)
    if variant == "no_input_grad":
        assert xd.grad is None
    else:
        errs["x"] = norm_rel(xd.grad, xr.grad)
    print(f"\n[lstm_pair {prec} {variant}] " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        if not k.startswith("out"):
            assert v < tol_grad, (k, v)
    if variant == "only_a":
        # stack b stayed outside the loss: its dy is zero, so nothing reaches its parameters but
        # the hand-off's step tag (the lowest mantissa bit of a published zero: a denormal, below
        # 1e-38 times the weights and activations, all of order one here)
        for k, a in mine[1].named_parameters():
            assert a.grad is None or float(a.grad.abs().max()) < 1e-30, k


def test_refusals():
    need_gpu()
    from mlvae_hip import ops
    from mlvae_hip._lib import last_error, lib
    a = torch.nn.LSTM(8, 16, 2, batch_first=True).cuda()
    x = torch.randn(2, 5, 8).cuda()
    for b in (torch.nn.LSTM(8, 32, 2, batch_first=True), torch.nn.LSTM(8, 16, 1, batch_first=True),
              torch.nn.LSTM(8, 16, 2, batch_first=True, bidirectional=True),
              torch.nn.LSTM(8, 16, 2, batch_first=True, dropout=0.15)):
        assert not ops.lstm_pair_ok(a, b, True)
        with pytest.raises(ValueError):
            ops.lstm_pair(x, a, b.cuda(), True)
    # the C entry: H must be a multiple of 4; an empty batch is a no-op
    xbuf, xbytes, err = _workspace(2, 16, F32)
    t = torch.zeros(64, device="cuda")
    args = lambda B, H: (F32, B, 3, H, P(t), P(t), P(t), P(t), P(t), None, P(xbuf), xbytes, P(err), stream())
    assert lib().mlvae_lstm_pair_fwd(*args(2, 10)) == 1
    assert "H" in last_error()
    assert lib().mlvae_lstm_pair_bwd(*args(2, 10)) == 1
    assert "H" in last_error()
    assert lib().mlvae_lstm_pair_fwd(*args(0, 16)) == 0
    assert lib().mlvae_lstm_pair_bwd(*args(0, 16)) == 0
    torch.cuda.synchronize()
    assert int(err.item()) == 0
