"""The 12-wave TPW-2 forward recurrence (csrc/lstm_wide.hip, lstm_fwd_wide_kernel W12 with two M-tiles
per MFMA wave: 128 < B <= 256 at H = 512) after the reshaped poll loop -- the first sweep's loads
issued back to back, the per-chunk staleness test kept for the retry sweeps only -- at the lengths
and under the load the earlier tests do not reach.

The poll loop decides when a wave reads the exchange, never what it reads: a granule is taken into
the h image only with the step's tag.  So the 12-wave form and the 8-wave equal-shares form (debug
mode bit 11), which share the accumulation order and the cell, give the same bits in every output:
h (bf16; in the fused-z form with y_bf16_prev the pre-shifted rows), dropout(h) (bf16), c (fp32),
the activated gates (fp16) and h (fp32).  The fp64 loop of test_gpu_lstm_wide bounds the values
themselves (TOL_Y, the bound that test uses for this kernel).

Shapes: B = 129 (9 batch groups, the last with one utterance: padded group slots, idle workgroups),
144 (full groups), 256 (256 workgroups: the retry sweep's partial-reload branch); T = 1 (no
hand-off: no poll), 2 (the first hand-off), 3 (both h-image buffers and both exchange slots written
a second time), 40 (steady state; fp64 reference at B = 129 and 256).  Both directions run in every
launch; dropout is on; the fused-z launches pre-shift h.

Race checks (T = 40): three launches on fresh NaN-poisoned outputs give the same bits with a clean
error word; at B = 129 and 144, where the grid leaves CUs free, once more while a second stream
copies a few hundred MB.  (Not at B = 256: the recurrence needs every CU resident.)
Reference op: nn.LSTM bidirectional at ref:src/modules/decoder.py:14-15,22."""
import functools

import pytest
import torch

from gpu_utils import P, need_gpu, stream
from mlvae_hip._lib import check, lib
from philox_np import dropout_mask
from test_gpu_lstm_wide import H
from test_gpu_lstm_wide_w12 import Z, _check_fp64, _plain_case, _workspace, _z_case

pytestmark = pytest.mark.gpu

# the 12-wave form (default) | the 8-wave equal-shares form (bit 11)
MODES = (0, 2048)
SHAPES = [(B, T) for B in (129, 144, 256) for T in (1, 2, 3)] + [(129, 40), (256, 40)]
NAMES = ("h bf16", "dropout(h) bf16", "c fp32", "gates fp16", "h fp32")
P_DROP = 0.15


@functools.lru_cache(maxsize=None)
def _random_case(B, T):
    """Inputs of the bits-only checks at shapes without an fp64 reference (same distributions)."""
    g = torch.Generator().manual_seed(977 * B + T)
    k = 1.0 / H ** 0.5
    w = [((torch.rand(4 * H, H, generator=g) * 2 - 1) * k) for _ in range(2)]
    gx = torch.randn(B * T, 8 * H, generator=g) * 0.5
    zf = torch.randn(B * T, Z, generator=g).to(torch.bfloat16)
    wih = [(torch.rand(4 * H, Z, generator=g) * 2 - 1) * 0.4 for _ in range(2)]
    bias = [(torch.rand(4 * H, generator=g) * 2 - 1) * 0.1 for _ in range(4)]
    return w, gx, zf, wih, bias


def _poisoned(N):
    nan = float("nan")
    return (torch.full((N, 2 * H), nan, device="cuda", dtype=torch.bfloat16),   # h bf16
            torch.full((N, 2 * H), nan, device="cuda", dtype=torch.bfloat16),   # dropout(h) bf16
            torch.full((N, 2 * H), nan, device="cuda"),                         # c
            torch.full((N, 2 * H), nan, device="cuda"))                         # h fp32


class _Plain:
    """One plain-forward problem on the device; launch() runs it on fresh poisoned outputs."""

    def __init__(self, B, T, w, gx):
        self.B, self.T, self.N = B, T, B * T
        self.G0 = gx.reshape(self.N, 8 * H).to(torch.float16).cuda().contiguous()
        self.W = [w[0].float().cuda(), w[1].float().cuda()]
        self.xbuf, self.xbytes = _workspace(B)
        self.err = torch.zeros(1, device="cuda", dtype=torch.int32)
        self.seed, self.doff = 0x51C3 + B, 4 * 2 * H

    def launch(self):
        Yb, Ydb, Cs, Y = _poisoned(self.N)
        G = self.G0.clone()
        check(lib().mlvae_lstm_fwd_ex2(1, self.B, self.T, H, P(self.W[0]), P(self.W[1]), P(G), 1, P(Cs), P(Y),
                                       Yb.data_ptr(), Ydb.data_ptr(), self.seed, self.doff, P_DROP,
                                       P(self.xbuf), self.xbytes, P(self.err), stream()))
        return Yb, Ydb, Cs, G, Y


class _FusedZ(_Plain):
    """The fused-z forward (layer 0) with the pre-shifted bf16 h rows."""

    def __init__(self, B, T, w, zf, wih, bias, ldz=40):
        self.B, self.T, self.N, self.ldz = B, T, B * T, ldz
        zpad = torch.zeros(self.N, ldz, dtype=torch.bfloat16)
        zpad[:, :Z] = zf
        self.zb = zpad.cuda().contiguous()
        self.W = [w[0].float().cuda(), w[1].float().cuda()]
        self.wi = [x.float().cuda() for x in wih]
        self.bs = [x.float().cuda() for x in bias]
        self.xbuf, self.xbytes = _workspace(B)
        self.err = torch.zeros(1, device="cuda", dtype=torch.int32)
        self.seed, self.doff = 0x3B19 + B, 8 * 2 * H

    def launch(self):
        Yb, Ydb, Cs, Y = _poisoned(self.N)
        G = torch.full((self.N, 8 * H), float("nan"), device="cuda").to(torch.float16)   # output only
        check(lib().mlvae_lstm_fwd_z2(self.B, self.T, H, P(self.W[0]), P(self.W[1]), self.zb.data_ptr(), self.ldz, Z,
                                      P(self.wi[0]), P(self.wi[1]), P(self.bs[0]), P(self.bs[1]), P(self.bs[2]),
                                      P(self.bs[3]), P(G), P(Cs), P(Y), Yb.data_ptr(), 1, Ydb.data_ptr(), None, 0.0,
                                      self.seed, self.doff, P_DROP, P(self.xbuf), self.xbytes, P(self.err), stream()))
        return Yb, Ydb, Cs, G, Y


def _mask(job):
    n = job.N * 2 * H
    return torch.from_numpy(dropout_mask(job.seed, job.doff + n, P_DROP)[job.doff:]).cuda().view(job.N, 2 * H)


def _all_modes(job):
    outs = {}
    try:
        for mode in MODES:
            lib().mlvae_lstm_set_debug_mode(mode)
            outs[mode] = job.launch()
            torch.cuda.synchronize()
            assert job.err.item() == 0, f"mode {mode}"
    finally:
        lib().mlvae_lstm_set_debug_mode(0)
    return outs


def _same_bits(outs, what):
    for other in MODES[1:]:
        for name, a, b in zip(NAMES, outs[0], outs[other]):
            assert torch.equal(a, b), f"{what}: {name} differs from mode {other}"


@pytest.mark.parametrize("B,T", SHAPES)
def test_plain_forward(B, T):
    need_gpu()
    w, gx, y, cs, gates = _plain_case(B, T)
    job = _Plain(B, T, w, gx)
    outs = _all_modes(job)
    mask = _mask(job)
    for mode in MODES:
        Yb, Ydb, Cs, G, Y = outs[mode]
        _check_fp64(B, T, Y, Cs, G, y, cs, gates, f"plain B={B} T={T} mode={mode}")
        assert torch.equal(Yb, Y.to(torch.bfloat16))
        assert torch.equal(Ydb, (Y * mask).to(torch.bfloat16))
    _same_bits(outs, f"plain B={B} T={T}")


@pytest.mark.parametrize("B,T", SHAPES)
def test_fused_z_forward(B, T):
    need_gpu()
    zf, wih, bias, w, y, cs, gates = _z_case(B, T)
    job = _FusedZ(B, T, w, zf, wih, bias)
    outs = _all_modes(job)
    mask = _mask(job)
    for mode in MODES:
        Yb, Ydb, Cs, G, Y = outs[mode]
        _check_fp64(B, T, Y, Cs, G, y, cs, gates, f"fused z B={B} T={T} mode={mode}")
        assert torch.equal(Ydb, (Y * mask).to(torch.bfloat16))
        # bf16 row t holds the h entering step t: h_{t-1} forward, h_{t+1} reverse, zeros at each
        # utterance's first step
        y3, p3 = Y.to(torch.bfloat16).view(B, T, 2 * H), Yb.view(B, T, 2 * H)
        assert torch.equal(p3[:, 1:, :H], y3[:, :-1, :H]) and torch.equal(p3[:, :-1, H:], y3[:, 1:, H:])
        assert (p3[:, 0, :H] == 0).all() and (p3[:, -1, H:] == 0).all()
    _same_bits(outs, f"fused z B={B} T={T}")


def _job(form, B, T):
    w, gx, zf, wih, bias = _random_case(B, T)
    return _Plain(B, T, w, gx) if form == "plain" else _FusedZ(B, T, w, zf, wih, bias)


@pytest.mark.parametrize("form", ["plain", "fused_z"])
@pytest.mark.parametrize("B", [129, 256])
def test_three_launches_same_bits(B, form):
    need_gpu()
    job = _job(form, B, 40)
    runs = []
    for _ in range(3):
        runs.append(job.launch())
        torch.cuda.synchronize()
        assert job.err.item() == 0
    for k in (1, 2):
        for name, a, b in zip(NAMES, runs[0], runs[k]):
            assert torch.equal(a, b), f"{form} B={B}: {name} of launch {k} differs"
    for name, a in zip(NAMES, runs[0]):
        assert not torch.isnan(a.float()).any(), f"{form} B={B}: {name} left unwritten"


@pytest.mark.parametrize("form", ["plain", "fused_z"])
@pytest.mark.parametrize("B", [129, 144])
def test_same_bits_beside_a_copy_stream(B, form):
    need_gpu()
    job = _job(form, B, 40)
    quiet = job.launch()
    torch.cuda.synchronize()
    assert job.err.item() == 0
    side = torch.cuda.Stream()
    src = torch.zeros(64 << 20, device="cuda", dtype=torch.uint8)
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):   # 8 x 64 MB read + written while the recurrence runs
            dst.copy_(src)
    loaded = job.launch()
    torch.cuda.synchronize()
    assert job.err.item() == 0
    for name, a, b in zip(NAMES, quiet, loaded):
        assert torch.equal(a, b), f"{form} B={B}: {name} differs beside the copy stream"
