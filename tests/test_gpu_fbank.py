"""The feature front end's HIP kernels (csrc/fbank.hip through mlvae_hip.ops.fbank and
brain.features.Fbank) against the float64 helper tests/fbank_ref.py.

Tolerance: the yardstick is the same helper run in float32 on the same input (same float64-built
tables rounded to fp32, every product and sum in fp32); its worst absolute error against float64
is computed here, and the device's worst error must be at most 4 x that, separately for statics,
deltas and delta-deltas (4: a different summation order over the window-long DFT sums, and the
device's log).  Frames per tile of the kernel: 32."""
import numpy as np
import pytest
import torch

import fbank_ref as R
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu

FT = 32  # csrc/fbank.hip
REF_GEO = dict(sample_rate=16000, hop_ms=20, win_ms=25, n_fft=400, n_mels=40)
# T_b = 1 .. 5 (the delta-delta edges), then one below, at and one above a tile of 32 frames, and
# three tiles
PARITY_N = [0, 1, 199, 200, 319, 320, 321, 4 * 320 + 7, (FT - 1) * 320 - 1, (FT - 1) * 320, FT * 320 + 1,
            (2 * FT + 2) * 320 + 5]


def _ops_kw(geo):
    return dict(sample_rate=geo["sample_rate"], hop_length=geo["hop_ms"], win_length=geo["win_ms"],
                n_fft=geo["n_fft"], n_mels=geo["n_mels"])


def spoken_like(n_samples, sample_rate, seed, noise=0.01):
    """Padded float32 batch of two-tone segments over a noise floor; NaN past each utterance."""
    g = np.random.default_rng(seed)
    wav = np.full((len(n_samples), max(max(n_samples), 1)), np.nan, dtype=np.float32)
    for b, N in enumerate(n_samples):
        n = np.arange(N)
        x = np.zeros(N)
        for lo in range(0, N, 2000):
            f1, f2 = g.uniform(300, 1100), g.uniform(1400, 0.45 * sample_rate)
            seg = n[lo:lo + 2000]
            x[lo:lo + 2000] = (0.5 * np.sin(2 * np.pi * f1 * seg / sample_rate + g.uniform(0, 6.28)) +
                               0.3 * np.sin(2 * np.pi * f2 * seg / sample_rate + g.uniform(0, 6.28)))
        wav[b, :N] = (x + noise * g.standard_normal(N)).astype(np.float32)
    return wav


def device_fbank(wav, n_samples, geo):
    from mlvae_hip import ops
    feats, frames = ops.fbank(torch.from_numpy(wav).cuda(), torch.tensor(n_samples, dtype=torch.int32),
                              **_ops_kw(geo))
    torch.cuda.synchronize()
    return feats.cpu().numpy(), frames.cpu().numpy()


def check_against_helper(wav, n_samples, geo, what):
    """Device vs float64 under the float32 yardstick; returns (device feats, float64 feats)."""
    ref64, frames64 = R.fbank_batch(wav.astype(np.float64), n_samples, dtype=np.float64, **geo)
    ref32, _ = R.fbank_batch(wav, n_samples, dtype=np.float32, **geo)
    got, frames = device_fbank(wav, n_samples, geo)
    assert got.shape == ref64.shape and got.dtype == np.float32
    assert np.array_equal(frames, frames64)
    assert np.isfinite(got).all()
    M = geo["n_mels"]
    for b, T in enumerate(frames64):
        assert not got[b, T:].any(), f"{what}: utterance {b} has non-zero rows past its {T} frames"
    for name, sl in (("static", slice(0, M)), ("delta", slice(M, 2 * M)), ("delta-delta", slice(2 * M, 3 * M))):
        e32 = np.abs(ref32[..., sl].astype(np.float64) - ref64[..., sl]).max()
        edev = np.abs(got[..., sl].astype(np.float64) - ref64[..., sl]).max()
        print(f"{what} {name}: device {edev:.3e} dB, float32 helper {e32:.3e} dB, ratio {edev / e32:.2f}")
        assert edev <= 4 * e32, (what, name, edev, e32)
    return got, ref64


@pytest.fixture(scope="module")
def parity_batch():
    return spoken_like(PARITY_N, 16000, seed=3)


def test_parity_with_the_float64_helper(parity_batch):
    need_gpu()
    check_against_helper(parity_batch, PARITY_N, REF_GEO, "parity")


def test_clamp_is_per_utterance():
    need_gpu()
    N = 24 * 320
    n = np.arange(N)
    loud = (0.5 * np.sin(2 * np.pi * 440 * n / 16000) + 0.3 * np.sin(2 * np.pi * 2450 * n / 16000 + 1.0))
    a = loud.copy()
    a[N // 2:] = 0.0  # digitally silent half: -100 dB before the clamp
    b = 0.01 * loud + 1e-4 * np.random.default_rng(9).standard_normal(N)  # 40 dB down
    wav = np.stack([a, b]).astype(np.float32)
    got, ref = check_against_helper(wav, [N, N], REF_GEO, "clamp")
    M = REF_GEO["n_mels"]
    silent = slice(N // 2 // 320 + 2, 1 + N // 320)  # frames wholly inside the silent half
    top_a, top_b = got[0, :, :M].max(), got[1, :, :M].max()
    assert ref[0, silent, :M].max() == ref[0, :, :M].max() - 80.0  # the clamp is active in the reference
    assert np.all(got[0, silent, :M] == np.float32(top_a - np.float32(80.0)))
    assert top_a - top_b > 30.0  # a batch-wide maximum would floor utterance b well above its own
    assert got[1, :, :M].min() < top_a - 80.0 - 10.0


@pytest.mark.parametrize("geo", [
    dict(sample_rate=8000, hop_ms=10, win_ms=25, n_fft=256, n_mels=23),
    # the limits: n_fft 512, 64 mels, an odd window (399 samples) shorter than n_fft
    dict(sample_rate=16000, hop_ms=10, win_ms=24.9375, n_fft=512, n_mels=64),
], ids=["8k-256-23", "16k-512-64-odd-window"])
def test_other_geometries(geo):
    need_gpu()
    hop, _ = R.geometry(geo["sample_rate"], geo["hop_ms"], geo["win_ms"])
    ns = [0, 1, hop - 1, hop, 3 * hop + 1, (FT - 1) * hop, FT * hop + 3, (2 * FT + 1) * hop + 7]
    check_against_helper(spoken_like(ns, geo["sample_rate"], seed=4), ns, geo, "geometry")


def test_independent_of_the_batch_and_deterministic(parity_batch):
    need_gpu()
    got, frames = device_fbank(parity_batch, PARITY_N, REF_GEO)
    again, _ = device_fbank(parity_batch, PARITY_N, REF_GEO)
    assert np.array_equal(got, again)
    for b, N in enumerate(PARITY_N):
        alone, f1 = device_fbank(parity_batch[b:b + 1], [N], REF_GEO)
        assert f1[0] == frames[b]
        assert np.array_equal(alone[0], got[b]), f"utterance {b} differs alone and in the batch"


def test_status_errors():
    need_gpu()
    from mlvae_hip import _lib, ops
    from brain.features import Fbank
    l = _lib.lib()
    wav = torch.zeros(1, 640, device="cuda")
    ns = torch.tensor([640], dtype=torch.int32, device="cuda")
    out = torch.zeros(1, 3, 120, device="cuda")
    frames = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf = torch.zeros(1 << 18, device="cuda")  # stands in for table and workspace: never launched
    s = torch.cuda.current_stream().cuda_stream
    for hop, win, n_fft, n_mels, word in ((320, 400, 401, 40, "even"), (320, 400, 514, 40, "512"),
                                          (320, 400, 256, 40, "window"), (320, 400, 400, 65, "n_mels"),
                                          (0, 400, 400, 40, "hop")):
        rc = l.mlvae_fbank(1, 640, wav.data_ptr(), 640, ns.data_ptr(), hop, win, n_fft, n_mels,
                           buf.data_ptr(), out.data_ptr(), 120, frames.data_ptr(), buf.data_ptr(),
                           buf.numel() * 4, s)
        assert rc != 0 and word in _lib.last_error(), (hop, win, n_fft, n_mels, _lib.last_error())
    with pytest.raises(_lib.MlvaeError, match="even"):
        Fbank(deltas=True, n_fft=401)(wav)
    with pytest.raises(RuntimeError, match="backward"):
        ops.fbank(wav.clone().requires_grad_(True))
    torch.cuda.synchronize()


def test_module_on_the_device(parity_batch):
    need_gpu()
    from brain.features import Fbank
    wav = torch.from_numpy(np.nan_to_num(parity_batch[-3:, :4000])).cuda()
    full = Fbank(deltas=True, hop_length=20)
    a = full(wav)
    b = full(wav, torch.ones(3))
    assert a.shape == (3, 1 + 4000 // 320, 120) and torch.equal(a, b)
    st = Fbank(deltas=False, hop_length=20)(wav)
    assert st.shape == (3, 13, 40) and torch.equal(st, a[..., :40])
    # relative lengths: N_b = round(N len_b), the rows past 1 + N_b // hop are zeros
    c = full(wav, torch.tensor([1.0, 0.5, 0.25]))
    assert torch.equal(c[0], a[0]) and not c[1, 1 + 2000 // 320:].any() and not c[2, 1 + 1000 // 320:].any()
    want, _ = R.fbank_batch(wav.cpu().numpy().astype(np.float64), [4000, 2000, 1000], **REF_GEO)
    assert np.abs(c.cpu().numpy() - want).max() < 1e-2
