"""The 12-wave TPW-2 forward recurrence (csrc/lstm_wide.hip, lstm_fwd_wide_kernel W12 with two
M-tiles per MFMA wave: 128 < B <= 256 at H = 512) against the 8-wave equal-shares form it replaces
(debug mode bit 11) and against the fp64 loop of test_gpu_lstm_wide.

Both forms accumulate each tile's k-chunks in the same order and share the cell math, so on the
same inputs and seeds every output is the same bits: h (bf16), dropout(h) (bf16), c (fp32), the
activated gates (fp16) and, in the fused-z form with y_bf16_prev, the pre-shifted h rows with
their zero rows.  The fp64 loop stays the yardstick for the values themselves (the bounds of
test_wide_recurrence_matches_fp64_loop).

Shapes: B = 129 (9 batch groups, the last with one utterance: valid[] masking, padded group slots,
idle workgroups), 144 (full groups), 256 (256 workgroups: the poll loop's partial-reload branch);
T = 1 (no hand-off), 2 (the first hand-off, both ring slots), 5 (LDS rings and exchange slots wrap
twice).  Reference op: nn.LSTM bidirectional at ref:src/modules/decoder.py:14-15,22."""
import ctypes
import functools

import pytest
import torch

from gpu_utils import P, need_gpu, rel_err, stream
from mlvae_hip._lib import check, lib
from philox_np import dropout_mask
from test_gpu_lstm_wide import H, TOL_Y, _reference

pytestmark = pytest.mark.gpu

SHAPES = [(B, T) for B in (129, 144, 256) for T in (1, 2, 5)]
MODES = (0, 2048)   # the 12-wave form (default) and the 8-wave equal-shares form
Z = 32


@functools.lru_cache(maxsize=None)
def _plain_case(B, T):
    w, gx, y, cs, gates, _, _ = _reference(B, T, 11 * B + T)
    return w, gx, y, cs, gates


@functools.lru_cache(maxsize=None)
def _z_case(B, T):
    g = torch.Generator().manual_seed(1234 + 7 * B + T)
    zf = torch.randn(B * T, Z, generator=g, dtype=torch.float64).to(torch.bfloat16)
    wih = [((torch.rand(4 * H, Z, generator=g, dtype=torch.float64) * 2 - 1) * 0.4).float() for _ in range(2)]
    bias = [((torch.rand(4 * H, generator=g, dtype=torch.float64) * 2 - 1) * 0.1).float() for _ in range(4)]
    gx = torch.cat([zf.double() @ wih[d].to(torch.bfloat16).double().t() + bias[2 * d].double() +
                    bias[2 * d + 1].double() for d in range(2)], 1).view(B, T, 8 * H)
    w, _, y, cs, gates, _, _ = _reference(B, T, 5 * B + T, gx=gx)
    return zf, wih, bias, w, y, cs, gates


def _workspace(B):
    xb = ctypes.c_size_t()
    check(lib().mlvae_lstm_workspace_size(B, H, 1, ctypes.byref(xb)))
    return torch.empty(xb.value, device="cuda", dtype=torch.uint8), xb.value


def _check_fp64(B, T, Y, Cs, G, y, cs, gates, what):
    ey, ec, eg = (rel_err(Y.view(B, T, 2 * H), y), rel_err(Cs.view(B, T, 2 * H), cs),
                  rel_err(G.float().view(B, T, 8 * H), gates))
    print(f"\n{what}: h {ey:.2e} c {ec:.2e} gates {eg:.2e}")
    assert ey < TOL_Y and ec < TOL_Y and eg < TOL_Y


@pytest.mark.parametrize("B,T", SHAPES)
def test_plain_forward_same_bits_as_8_waves(B, T):
    need_gpu()
    w, gx, y, cs, gates = _plain_case(B, T)
    N = B * T
    G0 = gx.reshape(N, 8 * H).to(torch.float16).cuda().contiguous()
    W0, W1 = w[0].float().cuda(), w[1].float().cuda()
    xbuf, xbytes = _workspace(B)
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    seed, doff, p = 0x12A5 + B, 4 * 2 * H, 0.15
    mask = torch.from_numpy(dropout_mask(seed, doff + N * 2 * H, p)[doff:]).cuda().view(N, 2 * H)
    outs = {}
    try:
        for mode in MODES:
            lib().mlvae_lstm_set_debug_mode(mode)
            G = G0.clone()
            Cs = torch.full((N, 2 * H), float("nan"), device="cuda")
            Y = torch.full((N, 2 * H), float("nan"), device="cuda")
            Yb = torch.full((N, 2 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
            Ydb = torch.full((N, 2 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
            check(lib().mlvae_lstm_fwd_ex2(1, B, T, H, P(W0), P(W1), P(G), 1, P(Cs), P(Y), Yb.data_ptr(),
                                           Ydb.data_ptr(), seed, doff, p, P(xbuf), xbytes, P(err), stream()))
            torch.cuda.synchronize()
            assert err.item() == 0, f"mode {mode}"
            _check_fp64(B, T, Y, Cs, G, y, cs, gates, f"plain B={B} T={T} mode={mode}")
            assert torch.equal(Yb, Y.to(torch.bfloat16))
            assert torch.equal(Ydb, (Y * mask).to(torch.bfloat16))
            outs[mode] = (Yb, Ydb, Cs, G, Y)
    finally:
        lib().mlvae_lstm_set_debug_mode(0)
    for name, a, b in zip(("h bf16", "dropout(h) bf16", "c fp32", "gates fp16", "h fp32"), outs[0], outs[2048]):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("ldz", [32, 40])
@pytest.mark.parametrize("B,T", SHAPES)
def test_fused_z_forward_same_bits_as_8_waves(B, T, ldz):
    need_gpu()
    zf, wih, bias, w, y, cs, gates = _z_case(B, T)
    N = B * T
    zpad = torch.zeros(N, ldz, dtype=torch.bfloat16)
    zpad[:, :Z] = zf
    zb = zpad.cuda().contiguous()
    W0, W1 = w[0].float().cuda(), w[1].float().cuda()
    wi = [x.cuda() for x in wih]
    bs = [x.cuda() for x in bias]
    xbuf, xbytes = _workspace(B)
    err = torch.zeros(1, device="cuda", dtype=torch.int32)
    seed, doff, p = 0x2A77 + B, 8 * 2 * H, 0.15
    mask = torch.from_numpy(dropout_mask(seed, doff + N * 2 * H, p)[doff:]).cuda().view(N, 2 * H)
    outs = {}
    try:
        for mode in MODES:
            lib().mlvae_lstm_set_debug_mode(mode)
            G = torch.full((N, 8 * H), float("nan"), device="cuda").to(torch.float16)   # output only
            Cs = torch.full((N, 2 * H), float("nan"), device="cuda")
            Y = torch.full((N, 2 * H), float("nan"), device="cuda")
            Yb = torch.full((N, 2 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
            Ydb = torch.full((N, 2 * H), float("nan"), device="cuda", dtype=torch.bfloat16)
            check(lib().mlvae_lstm_fwd_z2(B, T, H, P(W0), P(W1), zb.data_ptr(), ldz, Z, P(wi[0]), P(wi[1]), P(bs[0]),
                                          P(bs[1]), P(bs[2]), P(bs[3]), P(G), P(Cs), P(Y), Yb.data_ptr(), 1,
                                          Ydb.data_ptr(), None, 0.0, seed, doff, p, P(xbuf), xbytes, P(err), stream()))
            torch.cuda.synchronize()
            assert err.item() == 0, f"mode {mode}"
            _check_fp64(B, T, Y, Cs, G, y, cs, gates, f"fused z B={B} T={T} ldz={ldz} mode={mode}")
            assert torch.equal(Ydb, (Y * mask).to(torch.bfloat16))
            # bf16 row t holds the h entering step t: h_{t-1} forward, h_{t+1} reverse, zeros at each
            # utterance's first step
            y3, p3 = Y.to(torch.bfloat16).view(B, T, 2 * H), Yb.view(B, T, 2 * H)
            assert torch.equal(p3[:, 1:, :H], y3[:, :-1, :H]) and torch.equal(p3[:, :-1, H:], y3[:, 1:, H:])
            assert (p3[:, 0, :H] == 0).all() and (p3[:, -1, H:] == 0).all()
            outs[mode] = (Yb, Ydb, Cs, G, Y)
    finally:
        lib().mlvae_lstm_set_debug_mode(0)
    for name, a, b in zip(("pre-shifted h bf16", "dropout(h) bf16", "c fp32", "gates fp16", "h fp32"),
                          outs[0], outs[2048]):
        assert torch.equal(a, b), name
