"""modules.wav2vec2.Wav2Vec2 on the device against the HuggingFace fixtures
(tests/golden/w2v_tiny*.npz) and tests/w2v_ref.py, stage by stage, in both precisions.

Tolerance rule ("The wav2vec2 encoder"): per stage, the yardstick is
tests/w2v_ref.py on the CPU on the same input -- in float32 for precision='fp32', under torch bf16
autocast for precision='bf16' -- and its maximum and relative-RMS error against the float64
reference; the device is held to 4 x both (a different summation order, the MFMA's accumulation).
The yardsticks are computed here, once per input, and printed with the device's figures.  Measured
on the fixture's batch (tests/golden/make_golden_w2v.py; max, relative RMS against float64):

    stage     float32                 bf16 autocast
    conv0     9.2e-07, 1.1e-07        2.1e-02, 3.8e-03
    conv1     1.3e-06, 2.0e-07        2.9e-02, 4.9e-03
    conv2     1.1e-06, 2.6e-07        3.5e-02, 5.7e-03
    conv3     1.2e-06, 3.0e-07        2.7e-02, 6.4e-03
    conv4     1.3e-06, 3.7e-07        3.2e-02, 8.4e-03
    conv5     1.6e-06, 3.9e-07        3.8e-02, 9.4e-03
    conv6     1.8e-06, 5.3e-07        3.9e-02, 1.2e-02
    proj      3.0e-06, 6.2e-07        6.7e-02, 1.4e-02
    pos       3.5e-06, 6.8e-07        8.2e-02, 1.5e-02
    layer0    4.6e-06, 7.1e-07        9.4e-02, 1.5e-02
    layer1    5.0e-06, 6.9e-07        1.3e-01, 1.4e-02
    final     3.0e-06, 6.9e-07        6.5e-02, 1.4e-02
    out       2.9e-06, 6.9e-07        6.3e-02, 1.4e-02
    out at N = 400 / 719 / 720 / 3520:  float32 max 2.7e-06 / 2.4e-06 / 4.8e-06 / 2.8e-06,
                                        bf16    max 5.3e-02 / 6.9e-02 / 7.6e-02 / 6.7e-02
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import w2v_ref as R
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECS = ["fp32", "bf16"]


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["config"]))
    return z, cfg, R.fill_state(cfg, int(z["seed"]))


@functools.lru_cache(maxsize=None)
def cpu_stages(name, N):
    """(float64, float32, bf16-autocast) stage dicts of w2v_ref on the fixture's first N samples:
    computed once, shared, read only."""
    z, cfg, state = fixture(name)
    wav = torch.from_numpy(z["wav"])[:, :N].contiguous()
    s64, s32, s16 = {}, {}, {}
    with torch.no_grad():
        R.forward({k: v.double() for k, v in state.items()}, cfg, wav.double(), stages=s64)
        R.forward(state, cfg, wav, stages=s32)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            R.forward(state, cfg, wav, stages=s16)
    return wav, s64, s32, {k: v.float() for k, v in s16.items()}


def encoder(cfg, state, prec, **kw):
    from modules.wav2vec2 import Wav2Vec2
    m = Wav2Vec2(config=cfg, precision=prec, **kw)
    m.load_state_dict(state)
    return m.cuda()


def held(got, ref64, yard, what):
    e, y = R.errors(got.cpu(), ref64), R.errors(yard, ref64)
    print(f"{what}: device (max {e[0]:.3e}, rms {e[1]:.3e}), yardstick (max {y[0]:.3e}, rms {y[1]:.3e})")
    assert torch.isfinite(got).all(), what
    assert e[0] <= 4 * y[0] and e[1] <= 4 * y[1], (what, e, y)


@pytest.mark.parametrize("prec", PRECS)
def test_fixture_stage_by_stage(prec):
    need_gpu()
    z, cfg, state = fixture("w2v_tiny")
    wav, s64, s32, s16 = cpu_stages("w2v_tiny", z["wav"].shape[1])
    yard = s32 if prec == "fp32" else s16
    got = {}
    out = encoder(cfg, state, prec)(wav.cuda(), stages=got)
    assert out.dtype == torch.float32 and out.shape == (3, R.n_frames(cfg, wav.shape[1]), cfg["hidden_size"])
    assert torch.equal(out, got["out"])
    for n in R.stage_names(cfg)[1:]:
        keep = R.keep_frames(s64[n].shape[1])
        stored = torch.from_numpy(z[n]).double()  # the live HuggingFace model's float64 output
        held(got[n][:, keep], stored, yard[n][:, keep], f"{prec} {n} against the fixture")
        held(got[n], s64[n], yard[n], f"{prec} {n} against w2v_ref, every frame")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", [400, 719, 720, 3520])  # 1, 1, 2 and 10 frames
def test_frame_count_edges(N, prec):
    need_gpu()
    z, cfg, state = fixture("w2v_tiny")
    wav, s64, s32, s16 = cpu_stages("w2v_tiny", N)
    out = encoder(cfg, state, prec)(wav.cuda())
    assert out.shape[1] == (N - 400) // 320 + 1
    held(out, s64["out"], (s32 if prec == "fp32" else s16)["out"], f"{prec} N={N} out")


@pytest.mark.parametrize("prec", PRECS)
def test_head_width_32(prec):
    need_gpu()
    z, cfg, state = fixture("w2v_tiny_d32")
    assert cfg["hidden_size"] // cfg["num_attention_heads"] == 32
    wav, s64, s32, s16 = cpu_stages("w2v_tiny_d32", z["wav"].shape[1])
    out = encoder(cfg, state, prec)(wav.cuda())
    held(out, torch.from_numpy(z["out"]).double(), (s32 if prec == "fp32" else s16)["out"], f"{prec} d=32 out")


@pytest.mark.parametrize("prec", PRECS)
def test_without_the_whole_tensor_norms(prec):
    need_gpu()
    z, cfg, state = fixture("w2v_tiny")
    wav = torch.from_numpy(z["wav"])[:, :3520].contiguous()
    ref = lambda st, w: R.forward(st, cfg, w, normalize_wav=False, output_norm=False)
    with torch.no_grad():
        r64 = ref({k: v.double() for k, v in state.items()}, wav.double())
        if prec == "fp32":
            yard = ref(state, wav)
        else:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                yard = ref(state, wav).float()
    out = encoder(cfg, state, prec, normalize_wav=False, output_norm=False)(wav.cuda())
    held(out, r64, yard, f"{prec} no norms")


@pytest.mark.parametrize("prec", PRECS)
def test_one_layer_at_the_real_sizes(prec):
    """hidden 1024, 16 heads of 64, FFN 4096, positional conv K = 128 in 16 groups, T = 50, B = 1
    (a small conv stack in front): the layer's output against w2v_ref."""
    need_gpu()
    cfg = dict(R.LARGE_LV60, conv_dim=[32] * 7, num_hidden_layers=1)
    state = R.fill_state(cfg, 31)
    N = 400 + 320 * 49
    wav = R.ragged_wav(31, B=1, N=N, lens=(N - 2000,))
    s64, yard = {}, {}
    with torch.no_grad():
        R.forward({k: v.double() for k, v in state.items()}, cfg, wav.double(), stages=s64)
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=prec == "bf16"):
            R.forward(state, cfg, wav, stages=yard)
    got = {}
    encoder(cfg, state, prec)(wav.cuda(), stages=got)
    assert got["layer0"].shape == (1, 50, 1024)
    for n in ("pos", "layer0", "out"):
        held(got[n], s64[n], yard[n].float(), f"{prec} real-size {n}")


def test_reproducible_bits():
    need_gpu()
    z, cfg, state = fixture("w2v_tiny")
    wav = torch.from_numpy(z["wav"]).cuda()
    m = encoder(cfg, state, "bf16")
    assert torch.equal(m(wav), m(wav))


def test_unsupported_shape_raises_instead_of_falling_back():
    need_gpu()
    cfg = dict(R.TINY, hidden_size=96, intermediate_size=192)  # 2 heads of 48
    m = encoder(cfg, R.fill_state(cfg, 1), "bf16")
    assert not m.supported(12)
    with pytest.raises(ValueError, match="no fallback"):
        m(torch.zeros(1, 4000, device="cuda"))
    with pytest.raises(TypeError, match="no CPU fallback"):
        m(torch.zeros(1, 4000))
