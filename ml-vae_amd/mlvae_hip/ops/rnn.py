"""nn.LSTM on the persistent HIP recurrences (csrc/lstm.hip, csrc/lstm_wide.hip)."""
import ctypes

import torch

from .._lib import SZ, check, lib
from ._core import (_bt, colsum, current_shard, _dev_word, gemm, _need, _p, _prec, _stream, _workspace,
                    _ws_bytes)


# --------------------------------------------------------------------------- BiLSTM
def _lstm_ws(B, H):
    xb = SZ()
    check(lib().mlvae_lstm_workspace_size(B, H, _prec(), ctypes.byref(xb)), "lstm_workspace_size")
    # the recurrences' hand-off word (a word of its own: 1 = a hand-off timed out)
    return _workspace(xb.value, "lstm_x"), _dev_word("lstm_err")


def _dropout(src, dst, seed, p, sh=None):
    if sh is not None:
        B, T, C = _bt(src.shape, "lstm dropout")
        check(lib().mlvae_dropout_rows(B, T, C, _p(src), _p(dst), seed, p, sh.map(B), _stream()),
              "dropout_rows")
        return
    check(lib().mlvae_dropout(src.numel(), _p(src), _p(dst), None, seed, p, _stream()), "dropout")


class LSTMFn(torch.autograd.Function):
    """nn.LSTM(batch_first=True) on libmlvae, bidirectional (ndir 2: ref:src/modules/decoder.py:14-15,22)
    or not (ndir 1: ref:src/modules/phoneme_recognizer.py:13, boundary_detector.py:19): per layer
    an input-projection GEMM per direction + the persistent recurrence; inter-layer dropout
    (Philox, recomputed in backward) in train mode.  weights = the layer-major list
    [w_ih, w_hh, b_ih, b_hh] (+ [w_ih_r, w_hh_r, b_ih_r, b_hh_r] when bidirectional) * L."""

    @staticmethod
    def forward(ctx, x, H, L, ndir, dropout, seed, *weights):
        x = _need(x, "lstm input")
        B, T, _ = x.shape
        N = B * T
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        nw = 4 * ndir
        saved, inputs, seeds = [], [], []
        h = x
        for li in range(L):
            w = [_need(t, "lstm weight") for t in weights[nw * li:nw * li + nw]]
            din = h.shape[-1]
            G = torch.empty(N, 4 * H * ndir, device=x.device, dtype=torch.float32)
            for d in range(ndir):
                wi, _, bi, bh = w[4 * d:4 * d + 4]
                gemm(0, 1, N, 4 * H, din, _p(h), din, _p(wi), din, _p(G, 4 * H * d), 4 * H * ndir,
                     bias1=_p(bi), bias2=_p(bh))
            Cs = torch.empty(N, H * ndir, device=x.device, dtype=torch.float32)
            Y = torch.empty(B, T, H * ndir, device=x.device, dtype=torch.float32)
            if ndir == 2:
                check(l.mlvae_lstm_fwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(Y),
                                       _p(xbuf), _ws_bytes(xbuf), _p(err), _stream()), "lstm_fwd")
            else:
                check(l.mlvae_lstm1_fwd(_prec(), B, T, H, _p(w[1]), _p(G), _p(Cs), _p(Y), None,
                                        _p(xbuf), _ws_bytes(xbuf), _p(err), _stream()), "lstm1_fwd")
            inputs.append(h)
            saved += [G, Cs, Y]
            h = Y
            if li < L - 1 and dropout > 0:
                s = (seed * 1000003 + li) & ((1 << 63) - 1)
                hd = torch.empty_like(Y)
                _dropout(Y, hd, s, dropout, current_shard())
                seeds.append(s)
                h = hd
            else:
                seeds.append(None)
        ctx.save_for_backward(*inputs, *saved, *weights)
        ctx.H, ctx.L, ctx.ndir, ctx.dropout, ctx.seeds = H, L, ndir, dropout, seeds
        ctx.shard = current_shard()  # the backward recomputes the masks under the forward's map
        # nn.LSTM's (h_n, c_n) [L*ndir, B, H]: every layer's state after its last step (t = T-1
        # forward, t = 0 reverse; no packing, as nn.LSTM on a padded batch)
        hn = torch.empty(L * ndir, B, H, device=x.device, dtype=torch.float32)
        cn = torch.empty_like(hn)
        for li in range(L):
            G_, Cs_, Y_ = saved[3 * li:3 * li + 3]
            Cv = Cs_.view(B, T, H * ndir)
            for d in range(ndir):
                t_last = 0 if d else T - 1
                hn[li * ndir + d] = Y_[:, t_last, d * H:(d + 1) * H]
                cn[li * ndir + d] = Cv[:, t_last, d * H:(d + 1) * H]
        # h_n is differentiable (its gradient joins the layer output's at the last step); c_n's
        # gradient would need an initial cell gradient the BPTT kernels do not take: refused
        # loudly in backward.  Unused outputs arrive as None (no materialised zero tensors).
        ctx.set_materialize_grads(False)
        ctx.out_shape = h.shape
        return h, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn=None, dcn=None):
        H, L, ndir = ctx.H, ctx.L, ctx.ndir
        nw, GL = 4 * ndir, 4 * H * ndir
        t = ctx.saved_tensors
        inputs, saved, weights = t[:L], t[L:4 * L], t[4 * L:]
        if dcn is not None and bool(dcn.ne(0).any()):
            raise NotImplementedError("gradient through c_n of the HIP LSTM is not supported "
                                      "(the BPTT starts from a zero cell gradient)")
        if dy is None:
            dy = torch.zeros(ctx.out_shape, device=t[0].device, dtype=torch.float32)
        dy = _need(dy, "lstm grad").clone()
        B, T = dy.shape[0], dy.shape[1]
        N = B * T
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        dW = [None] * len(weights)
        dx = None
        for li in range(L - 1, -1, -1):
            G, Cs, Y = saved[3 * li:3 * li + 3]
            w = weights[nw * li:nw * li + nw]
            xin = inputs[li]
            din = xin.shape[-1]
            if dhn is not None:  # h_n[li, d] is Y_li at t = T-1 (forward) / t = 0 (reverse)
                for d in range(ndir):
                    dy[:, 0 if d else T - 1, d * H:(d + 1) * H] += dhn[li * ndir + d]
            if ndir == 2:
                check(l.mlvae_lstm_bwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(dy),
                                       _p(xbuf), _ws_bytes(xbuf), _p(err), _stream()), "lstm_bwd")
            else:
                check(l.mlvae_lstm1_bwd(_prec(), B, T, H, _p(w[1]), _p(G), _p(Cs), _p(dy), None,
                                        _p(xbuf), _ws_bytes(xbuf), _p(err), _stream()), "lstm1_bwd")
            dx = torch.empty(B, T, din, device=dy.device, dtype=torch.float32)
            for d in range(ndir):
                wi = w[4 * d]
                gemm(0, 0, N, din, 4 * H, _p(G, 4 * H * d), GL, _p(wi), din, _p(dx), din,
                     beta=1.0 if d else 0.0)
                gwi = torch.empty_like(wi)
                gemm(1, 0, 4 * H, din, N, _p(G, 4 * H * d), GL, _p(xin), din, _p(gwi), din)
                gwh = torch.empty_like(w[4 * d + 1])
                # dW_hh = sum_t dG_t^T h_{t-1} (forward) / h_{t+1} (reverse): time-shifted B rows
                gemm(1, 0, 4 * H, H, N, _p(G, 4 * H * d), GL, _p(Y, H * d), H * ndir, _p(gwh), H,
                     kshift_T=T, kshift=1 if d else -1)
                gbi = torch.empty_like(w[4 * d + 2])
                gbh = torch.empty_like(w[4 * d + 3])
                colsum(N, 4 * H, _p(G, 4 * H * d), GL, _p(gbi), _p(gbh))
                base = nw * li + 4 * d
                dW[base:base + 4] = [gwi, gwh, gbi, gbh]
            if li > 0 and ctx.seeds[li - 1] is not None:
                _dropout(dx, dx, ctx.seeds[li - 1], ctx.dropout, ctx.shard)
            dy = dx
        if int(err.item()) != 0:
            raise RuntimeError("LSTM recurrence hand-off timed out")
        return (dx, None, None, None, None, None, *dW)


def _lstm_weights(lstm_module):
    """The module's parameters as LSTMFn's layer-major list (direction-major inside a layer)."""
    return [getattr(lstm_module, f"{kind}_l{li}{sfx}") for li in range(lstm_module.num_layers)
            for sfx in ("", "_reverse")[:2 if lstm_module.bidirectional else 1]
            for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def lstm(x, lstm_module, train):
    """Run an nn.LSTM's parameters (batch_first, uni- or bidirectional) through the HIP
    recurrence; its own forward is not used."""
    if not lstm_module.batch_first:
        raise ValueError("the HIP LSTM path is batch_first only (as every reference LSTM)")
    H, L = lstm_module.hidden_size, lstm_module.num_layers
    ndir = 2 if lstm_module.bidirectional else 1
    p = float(lstm_module.dropout) if train else 0.0
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
    return LSTMFn.apply(x, H, L, ndir, p, seed, *_lstm_weights(lstm_module))[0]


def lstm_full(x, lstm_module, train, seed=None):
    """nn.LSTM's whole forward on the HIP recurrence: (output, (h_n, c_n)).  seed: the
    inter-layer dropout's Philox key (drawn from torch's generator when None)."""
    if not lstm_module.batch_first:
        raise ValueError("the HIP LSTM path is batch_first only (as every reference LSTM)")
    H, L = lstm_module.hidden_size, lstm_module.num_layers
    ndir = 2 if lstm_module.bidirectional else 1
    p = float(lstm_module.dropout) if train else 0.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if p > 0 else 0
    out, hn, cn = LSTMFn.apply(x, H, L, ndir, p, seed, *_lstm_weights(lstm_module))
    return out, (hn, cn)


class LSTMPairFn(torch.autograd.Function):
    """Two independent unidirectional nn.LSTM(batch_first=True) stacks of one shape over the same
    input (the joint recipes' recogniser and detector, ref:src/modules/phoneme_recognizer.py:13,
    boundary_detector.py:19): per layer two input-projection GEMMs into the column halves of one
    G [N, 8H] and ONE paired recurrence launch (mlvae_lstm_pair_fwd / _bwd), so the two stacks'
    latency-bound step chains overlap.  No dropout inside a paired stack.  weights = the
    layer-major list [w_ih, w_hh, b_ih, b_hh] of stack a + the same of stack b, * L."""

    @staticmethod
    def forward(ctx, x, H, L, *weights):
        x = _need(x, "lstm input")
        B, T, _ = x.shape
        N = B * T
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        saved, inputs = [], []
        h = x
        for li in range(L):
            w = [_need(t, "lstm weight") for t in weights[8 * li:8 * li + 8]]
            # layer 0: both stacks read x; above it stack s reads its own half of Y (lda = 2H)
            din, lda = (h.shape[-1], h.shape[-1]) if li == 0 else (H, 2 * H)
            G = torch.empty(N, 8 * H, device=x.device, dtype=torch.float32)
            for s in range(2):
                wi, _, bi, bh = w[4 * s:4 * s + 4]
                gemm(0, 1, N, 4 * H, din, _p(h, H * s if li else 0), lda, _p(wi), din,
                     _p(G, 4 * H * s), 8 * H, bias1=_p(bi), bias2=_p(bh))
            Cs = torch.empty(N, 2 * H, device=x.device, dtype=torch.float32)
            Y = torch.empty(B, T, 2 * H, device=x.device, dtype=torch.float32)
            check(l.mlvae_lstm_pair_fwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(Y), None,
                                        _p(xbuf), _ws_bytes(xbuf), _p(err), _stream()), "lstm_pair_fwd")
            inputs.append(h)
            saved += [G, Cs, Y]
            h = Y
        ctx.save_for_backward(*inputs, *saved, *weights)
        ctx.H, ctx.L = H, L
        ctx.set_materialize_grads(False)  # an output outside the loss arrives as None
        return h[..., :H].contiguous(), h[..., H:].contiguous()

    @staticmethod
    def backward(ctx, dya, dyb):
        H, L = ctx.H, ctx.L
        GL = 8 * H
        t = ctx.saved_tensors
        inputs, saved, weights = t[:L], t[L:4 * L], t[4 * L:]
        B, T = inputs[0].shape[0], inputs[0].shape[1]
        N = B * T
        dev = inputs[0].device
        dy = torch.zeros(B, T, 2 * H, device=dev, dtype=torch.float32)
        for s, g in enumerate((dya, dyb)):
            if g is not None:
                dy[..., H * s:H * (s + 1)] = _need(g, "lstm grad")
        l = lib()
        xbuf, err = _lstm_ws(B, H)
        dW = [None] * len(weights)
        dx = None
        for li in range(L - 1, -1, -1):
            G, Cs, Y = saved[3 * li:3 * li + 3]
            w = weights[8 * li:8 * li + 8]
            xin = inputs[li]
            din, ldx = (xin.shape[-1], xin.shape[-1]) if li == 0 else (H, 2 * H)
            check(l.mlvae_lstm_pair_bwd(_prec(), B, T, H, _p(w[1]), _p(w[5]), _p(G), _p(Cs), _p(dy), None,
                                        _p(xbuf), _ws_bytes(xbuf), _p(err), _stream()), "lstm_pair_bwd")
            if li > 0:  # the dgrads fill the column halves of the layer below's dy
                dx = torch.empty(B, T, 2 * H, device=dev, dtype=torch.float32)
            elif ctx.needs_input_grad[0]:  # dx = dx_a + dx_b
                dx = torch.empty(B, T, din, device=dev, dtype=torch.float32)
            else:
                dx = None
            for s in range(2):
                wi = w[4 * s]
                if li > 0:
                    gemm(0, 0, N, H, 4 * H, _p(G, 4 * H * s), GL, _p(wi), H, _p(dx, H * s), 2 * H)
                elif dx is not None:
                    gemm(0, 0, N, din, 4 * H, _p(G, 4 * H * s), GL, _p(wi), din, _p(dx), din,
                         beta=1.0 if s else 0.0)
                gwi = torch.empty_like(wi)
                gemm(1, 0, 4 * H, din, N, _p(G, 4 * H * s), GL, _p(xin, H * s if li else 0), ldx,
                     _p(gwi), din)
                gwh = torch.empty_like(w[4 * s + 1])
                # dW_hh = sum_t dG_t^T h_{t-1}: both stacks run forward in time
                gemm(1, 0, 4 * H, H, N, _p(G, 4 * H * s), GL, _p(Y, H * s), 2 * H, _p(gwh), H,
                     kshift_T=T, kshift=-1)
                gbi = torch.empty_like(w[4 * s + 2])
                gbh = torch.empty_like(w[4 * s + 3])
                colsum(N, 4 * H, _p(G, 4 * H * s), GL, _p(gbi), _p(gbh))
                base = 8 * li + 4 * s
                dW[base:base + 4] = [gwi, gwh, gbi, gbh]
            dy = dx
        if int(err.item()) != 0:
            raise RuntimeError("LSTM recurrence hand-off timed out")
        return (dx, None, None, *dW)


def lstm_pair_ok(lstm_a, lstm_b, train):
    """True where lstm_pair can run the two modules as one paired recurrence."""
    for m in (lstm_a, lstm_b):
        if not isinstance(m, torch.nn.LSTM) or not m.batch_first or m.bidirectional or m.proj_size:
            return False
    if (lstm_a.input_size, lstm_a.hidden_size, lstm_a.num_layers) != \
            (lstm_b.input_size, lstm_b.hidden_size, lstm_b.num_layers):
        return False
    if lstm_a.hidden_size % 4:
        return False
    return not train or (float(lstm_a.dropout) == 0.0 and float(lstm_b.dropout) == 0.0)


def lstm_pair(x, lstm_a, lstm_b, train):
    """Two unidirectional nn.LSTMs of one shape over the same input x, their recurrences paired
    in one launch per layer: (out_a, out_b), each [B, T, H]."""
    if not lstm_pair_ok(lstm_a, lstm_b, train):
        raise ValueError("lstm_pair: two batch_first unidirectional nn.LSTMs of equal input_size, "
                         "hidden_size (a multiple of 4) and num_layers, without projection and "
                         "without dropout in training")
    H, L = lstm_a.hidden_size, lstm_a.num_layers
    wa, wb = _lstm_weights(lstm_a), _lstm_weights(lstm_b)  # layer-major: stack a's four, then stack b's
    weights = [w for li in range(L) for stack in (wa, wb) for w in stack[4 * li:4 * li + 4]]
    return LSTMPairFn.apply(x, H, L, *weights)


def bilstm(x, lstm_module, train):
    """The decoder's bidirectional nn.LSTM (ref:src/modules/decoder.py:22)."""
    return lstm(x, lstm_module, train)
