"""modules.wav2vec2.Wav2Vec2(freeze=False, freeze_feature_extractor=True) on the device: every
trainable tensor's gradient against float64 autograd of tests/w2v_ref.py, the forward's bits
against the frozen module, reproducible bits, one layer at the real sizes and one Adam step.

Tolerance rule (tests/w2v_grad_ref.py): per tensor, 4 x the error against float64 of the same
autograd in float32 (precision 'fp32') or under bf16 autocast ('bf16'), maximum and relative RMS,
floored at 2^-23 relative.  The loss is sum(out * cot) with a fixed cotangent.  Measured (largest
maximum error over the tensors of a group, with and without output_norm: device, yardstick; the worst
single device / yardstick ratio, bound 4):

    w2v_tiny [3, 4000]        fp32 device  yardstick  ratio    bf16 device  yardstick  ratio
    feature_projection.*        5.2e-05     3.0e-05    1.91      4.3e-01     7.9e-01    1.15
    encoder.pos_conv_embed.*    3.3e-05     2.4e-05    2.07      3.3e-01     3.9e-01    0.84
    encoder.layers.* weights    3.0e-05     1.5e-05    2.42      2.7e-01     3.5e-01    1.37
    encoder.layers.* biases     1.1e-05     1.1e-05    2.83      1.4e-01     2.0e-01    1.92
    encoder.layer_norm.*        1.7e-05     1.7e-05    1.02      2.0e-01     2.5e-01    0.90
    w2v_tiny_d32, all tensors   3.8e-05     2.8e-05    2.04      4.1e-01     9.6e-01    1.62
    one layer, real sizes       3.5e-05     2.8e-04    1.97      3.5e-01     6.8e-01    0.92
    k_proj.bias (exact gradient 0): bf16 device 2.1e-03 .. 8.1e-03, yardstick 3.4e-03 .. 1.1e-02
    one Adam step: sign agreement 1.0000 (classifier) / 0.9995 (encoder), update error 0.0000 / 0.0301
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import w2v_grad_ref as GR
import w2v_ref as R
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PRECS = ["fp32", "bf16"]


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["config"]))
    return torch.from_numpy(z["wav"]), cfg, R.fill_state(cfg, int(z["seed"]))


def cotangent(shape, seed=3):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def oracle(name, output_norm):
    """{mode: (out, grads, dproj)} of the fixture's batch: computed once, shared, read only."""
    wav, cfg, state = fixture(name)
    cot = cotangent((wav.shape[0], R.n_frames(cfg, wav.shape[1]), cfg["hidden_size"]))
    return cot, {m: GR.encoder_grads(state, cfg, wav, cot, m, output_norm=output_norm) for m in ("fp64", "fp32", "bf16")}


def encoder(cfg, state, prec, trainable=True, **kw):
    from modules.wav2vec2 import Wav2Vec2
    extra = dict(freeze=False, freeze_feature_extractor=True) if trainable else {}
    m = Wav2Vec2(config=cfg, precision=prec, **extra, **kw)
    m.load_state_dict(state)
    return m.cuda()


def grads_of(m, wav, cot):
    for p in m.parameters():
        p.grad = None
    out = m(wav)
    (out * cot).sum().backward()
    return out.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("output_norm", [True, False])
@pytest.mark.parametrize("name", ["w2v_tiny", "w2v_tiny_d32"])
def test_encoder_gradients(name, output_norm, prec):
    need_gpu()
    wav, cfg, state = fixture(name)
    cot, ref = oracle(name, output_norm)
    (o64, g64, _), (_, gy, _) = ref["fp64"], ref[prec]
    m = encoder(cfg, state, prec, output_norm=output_norm)
    m.train()
    out, got = grads_of(m, wav.cuda(), cot.cuda())
    assert set(got) == {k for k in state if GR.trainable(k)} == set(g64)
    for k in g64:
        GR.held(got[k], g64[k], gy[k], f"{name} {prec} output_norm={output_norm} d {k}")
    # the conv stack is frozen: plain tensors that autograd never saw
    for k, t in m.state_dict(keep_vars=True).items():
        if not GR.trainable(k):
            assert not t.requires_grad and t.grad is None, k
    # the forward's bits are the frozen module's, in train() and in eval(); a rerun: the same bits
    assert torch.equal(out, encoder(cfg, state, prec, trainable=False, output_norm=output_norm)(wav.cuda()))
    m.eval()
    out2, got2 = grads_of(m, wav.cuda(), cot.cuda())
    assert torch.equal(out, out2)
    for k in got:
        assert torch.equal(got[k], got2[k]), k


@pytest.mark.parametrize("prec", PRECS)
def test_one_layer_at_the_real_sizes(prec):
    """hidden 1024, 16 heads of 64, FFN 4096, positional conv K = 128 in 16 groups, T = 50, B = 1 (a
    small conv stack in front): the gradients of the layer's tensors and of the positional conv."""
    need_gpu()
    cfg = dict(R.LARGE_LV60, conv_dim=[32] * 7, num_hidden_layers=1)
    state = R.fill_state(cfg, 31)
    N = 400 + 320 * 49
    wav = R.ragged_wav(31, B=1, N=N, lens=(N - 2000,))
    cot = cotangent((1, 50, 1024))
    _, g64, _ = GR.encoder_grads(state, cfg, wav, cot, "fp64")
    _, gy, _ = GR.encoder_grads(state, cfg, wav, cot, prec)
    _, got = grads_of(encoder(cfg, state, prec), wav.cuda(), cot.cuda())
    for k in g64:
        if k.startswith(("encoder.layers.0.", "encoder.pos_conv_embed.")):
            GR.held(got[k], g64[k], gy[k], f"real-size {prec} d {k}")


def test_adam_step_per_group():
    """One Adam step of each of the recipe's two groups (a classifier on the encoder's output with lr,
    the encoder with lr_wav2vec) against torch's Adam on the oracle's float64 gradients, by the
    project's update check (tests/step_parity.py: sign agreement >= 99.5 % where the direction is
    defined, update error <= 0.15 norm-relative), bf16.  The conv stack's weights keep their bits; the
    kernel-side copies are refreshed: the next forward equals the frozen module's on the new state."""
    need_gpu()
    from mlvae_hip import optim as hip_optim
    from step_parity import update_errors
    wav, cfg, state = fixture("w2v_tiny")
    H, T = cfg["hidden_size"], R.n_frames(cfg, wav.shape[1])
    g = torch.Generator().manual_seed(17)
    cw, cb = torch.randn(1, H, generator=g) / H ** 0.5, torch.zeros(1)
    cot = cotangent((wav.shape[0], T, 1), seed=4)
    lr, lr_w2v = 1e-3, 1e-4
    # the oracle: float64 autograd, torch's Adam
    st = {k: v.double().clone().requires_grad_(GR.trainable(k)) for k, v in state.items()}
    head = [cw.double().clone().requires_grad_(True), cb.double().clone().requires_grad_(True)]
    (torch.nn.functional.linear(R.forward(st, cfg, wav.double()), *head) * cot.double()).sum().backward()
    enc_params = {k: v for k, v in st.items() if GR.trainable(k)}
    old = {**{k: v.detach().clone() for k, v in enc_params.items()}, "cw": head[0].detach().clone(),
           "cb": head[1].detach().clone()}
    grads = {**{k: v.grad.clone() for k, v in enc_params.items()}, "cw": head[0].grad.clone(), "cb": head[1].grad.clone()}
    torch.optim.Adam(head, lr=lr).step()
    torch.optim.Adam(list(enc_params.values()), lr=lr_w2v).step()
    new_ref = {**{k: v.detach() for k, v in enc_params.items()}, "cw": head[0].detach(), "cb": head[1].detach()}
    # the device
    m = encoder(cfg, state, "bf16")
    before = {k: v.clone() for k, v in m.state_dict().items()}
    clf = torch.nn.Linear(H, 1).cuda()
    with torch.no_grad():
        clf.weight.copy_(cw)
        clf.bias.copy_(cb)
    opts = [hip_optim.Adam(clf.parameters(), lr=lr), hip_optim.Adam(m.parameters(), lr=lr_w2v)]
    out0 = m(wav.cuda())
    (clf(out0) * cot.cuda()).sum().backward()
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    now = {**dict(m.named_parameters()), "cw": clf.weight, "cb": clf.bias}

    class View:
        view = staticmethod(lambda k: now[k])
    for group, keys in (("classifier", ["cw", "cb"]), ("wav2vec2", list(enc_params))):
        sign, uerr, dmax = update_errors(View, {"grads": grads}, new_ref, {k: old[k] for k in keys})
        print(f"adam step, group {group}: sign agreement {sign:.4f}, update error {uerr:.4f}, max |p - oracle| {dmax:.2e}")
        assert sign >= 0.995 and uerr <= 0.15, (group, sign, uerr)
    after = m.state_dict()
    for k in after:
        if not GR.trainable(k):
            assert torch.equal(after[k], before[k]), k
        else:
            assert not torch.equal(after[k], before[k]), k
    out1 = m(wav.cuda())
    assert not torch.equal(out1, out0)
    assert torch.equal(out1, encoder(cfg, {k: v.cpu() for k, v in after.items()}, "bf16", trainable=False)(wav.cuda()))
