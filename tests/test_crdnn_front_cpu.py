"""The CRDNN front end's host-side parts (no GPU): modules.crdnn.CNNFront / ConvCRDNN construct on
the CPU with the sizes, parameter names and limits the module states; both model_cnn.yaml files
resolve to the reference's cnn_blocks: 2 / time_pooling: True on a ConvCRDNN; the recipe's frame
resampling follows the reference's rule; and the restatement tests/crdnn_front_ref.py, which the
GPU tests compare the kernels to, equals a direct torch.nn composition (SpeechBrain is absent: this
pins the helper to torch)."""
import os

import pytest
import torch
from torch import nn

import crdnn_front_ref as R
from conftest import PKG


def test_front_sizes_names_and_limits():
    from modules.crdnn import CNNFront, ConvCRDNN, CRDNN
    f = CNNFront(120, 2, (128, 256), (3, 3), 0.15, True)
    assert f.output_size == 30 * 256 == 7680
    assert CNNFront(13, 2, (16, 32), (3, 3), 0.15, False).output_size == 3 * 32
    assert CNNFront(40, 0, (16, 32), (3, 3), 0.15, True).output_size == 40
    want = {}
    for i, (cin, c, F) in enumerate(((1, 128, 120), (128, 256, 60))):
        want[f"block_{i}.conv_1.weight"], want[f"block_{i}.conv_1.bias"] = (c, cin, 3, 3), (c,)
        want[f"block_{i}.conv_2.weight"], want[f"block_{i}.conv_2.bias"] = (c, c, 3, 3), (c,)
        for j in (1, 2):
            want[f"block_{i}.norm_{j}.weight"] = want[f"block_{i}.norm_{j}.bias"] = (F, c)
    assert {k: tuple(v.shape) for k, v in f.state_dict().items()} == want
    assert torch.equal(f.block_0.norm_1.weight, torch.ones(120, 128)) and not f.block_1.norm_2.bias.any()
    bound = 1.0 / (128 * 9) ** 0.5  # torch's Conv2d default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
    assert f.block_1.conv_1.weight.abs().max() <= bound and f.block_1.conv_1.weight.abs().max() > 0.9 * bound
    with pytest.raises(ValueError):
        CNNFront(120, 2, (128, 256), (5, 5), 0.15, True)
    with pytest.raises(ValueError):
        ConvCRDNN(120, cnn_blocks=2, cnn_kernelsize=(3, 5), rnn_layers=1, rnn_neurons=8, dnn_blocks=1, dnn_neurons=8)
    with pytest.raises(ValueError):
        CNNFront(120, 2, (24, 32), (3, 3), 0.15, True)  # channels: multiples of 16
    net = ConvCRDNN(120, nn.LeakyReLU, 0.15, 2, (16, 32), (3, 3), True, 2, 8, True, 1, 8)
    assert isinstance(net, CRDNN) and net.front.output_size == 30 * 32 == net.rnn.input_size and net.output_size == 8
    assert {k.split(".")[0] for k in net.state_dict()} == {"front", "rnn", "dnn"}
    plain = ConvCRDNN(120, nn.LeakyReLU, 0.15, 0, (16, 32), (3, 3), False, 2, 8, True, 1, 8)
    assert plain.front is None and plain.rnn.input_size == 120
    assert set(plain.state_dict()) == set(CRDNN(120, nn.LeakyReLU, 0.15, 0, (16, 32), (3, 3), False, 2, 8, True, 1,
                                                8).state_dict())
    masks = f.draw_keep(4, "cpu")
    assert [tuple(m.shape) for m in masks] == [(4, 60), (4, 30)]
    assert all(set(m.unique().tolist()) <= {0.0, float(torch.tensor(1.0) / 0.85)} for m in masks)


def test_ops_argument_checks_need_no_device():
    from mlvae_hip import ops
    with pytest.raises(ValueError):
        ops.conv2d_3x3(torch.zeros(1, 4, 4, 16), torch.zeros(16, 16, 3, 5))
    with pytest.raises(ValueError):
        ops.conv2d_3x3(torch.zeros(1, 4, 4, 8), torch.zeros(16, 16, 3, 3))
    with pytest.raises(ValueError):
        ops.layer_norm_fc_act(torch.zeros(1, 4, 4, 16), torch.zeros(4, 8), torch.zeros(4, 8))
    with pytest.raises(ValueError):
        ops.layer_norm_fc_act(torch.zeros(1, 4, 4, 16), torch.zeros(4, 16), torch.zeros(4, 16), keep=torch.ones(1, 2))
    with pytest.raises(ValueError):
        ops.time_pool(torch.zeros(2, 1, 16))
    with pytest.raises(TypeError):  # no CPU fallback
        ops.time_pool(torch.zeros(2, 4, 16))


@pytest.mark.parametrize("name", ["CRDNN_CTC", "CRDNN_CTC_cnncl"])
def test_model_cnn_yaml_resolves(name):
    from hyperpyyaml import load_hyperpyyaml
    from modules.crdnn import CNNFront, ConvCRDNN
    ov = (f"dataset: synthetic\nmodel_class: {name}\nmodel_name: ctc\n"
          f"model: !include:../models/{name}/model_cnn.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [{}, ov])
    m = hp["model"]
    assert m["cnn_blocks"] == 2 and m["time_pooling"] is True and list(m["cnn_channels"]) == [128, 256]
    net = m["crdnn"]
    assert isinstance(net, ConvCRDNN) and isinstance(net.front, CNNFront)
    assert net.front.n_blocks == 2 and net.front.time_pooling and net.front.output_size == 7680
    assert net.rnn.input_size == 7680 and (net.rnn.hidden_size, net.rnn.num_layers) == (512, 4)
    with open(os.path.join(PKG, "models", name, "model.yaml")) as f:  # the same recipe otherwise
        old = f.read()
    with open(os.path.join(PKG, "models", name, "model_cnn.yaml")) as f:
        new = f.read()
    assert m["precision"] == "bf16"  # the Conv2d kernels have a bf16-operand form only
    body = lambda s: [l for l in s.splitlines() if not l.startswith("#") and l != "precision: bf16"]
    diff = [(a, b) for a, b in zip(body(old), body(new)) if a != b]
    assert len(body(old)) == len(body(new)) and len(diff) == 3, diff


def test_resample_frames_follows_the_reference_rule():
    from models.CRDNN_CTC.model import resample_frames
    p = torch.arange(2 * 3 * 2, dtype=torch.float32).reshape(2, 3, 2)
    assert resample_frames(p, 3) is p
    up = resample_frames(p, 7)  # factor 2, one zero frame appended
    assert up.shape == (2, 7, 2) and torch.equal(up[:, 0:6:2], p) and torch.equal(up[:, 1:6:2], p)
    assert not up[:, 6].any()
    assert torch.equal(resample_frames(p, 6), torch.repeat_interleave(p, 2, dim=1))
    assert torch.equal(resample_frames(p, 5), torch.cat([p, torch.zeros(2, 2, 2)], 1))  # factor 1: padded by two
    with pytest.raises(ValueError):
        resample_frames(p, 2)   # fewer target frames than source frames
    with pytest.raises(ValueError):
        resample_frames(torch.zeros(1, 5, 2), 9)  # factor 1 leaves 4 frames missing: more than 3
    assert resample_frames(p, 16).shape == (2, 16, 2)  # factor 5 gives 15, one padded


def test_restatement_equals_a_direct_torch_composition():
    torch.manual_seed(0)
    B, T, F, C1, C2 = 2, 7, 13, 4, 6
    x = torch.randn(B, T, F)
    convs = [nn.Conv2d(1, C1, 3, padding=1, padding_mode="reflect"), nn.Conv2d(C1, C1, 3, padding=1, padding_mode="reflect"),
             nn.Conv2d(C1, C2, 3, padding=1, padding_mode="reflect"), nn.Conv2d(C2, C2, 3, padding=1, padding_mode="reflect")]
    norms = [nn.LayerNorm([13, C1]), nn.LayerNorm([13, C1]), nn.LayerNorm([6, C2]), nn.LayerNorm([6, C2])]
    params = {}
    for i in range(2):
        for j in (1, 2):
            n = norms[2 * i + j - 1]
            with torch.no_grad():
                n.weight.add_(0.1 * torch.randn_like(n.weight))
                n.bias.add_(0.1 * torch.randn_like(n.bias))
            params[f"block_{i}.conv_{j}.weight"] = convs[2 * i + j - 1].weight.detach()
            params[f"block_{i}.conv_{j}.bias"] = convs[2 * i + j - 1].bias.detach()
            params[f"block_{i}.norm_{j}.weight"], params[f"block_{i}.norm_{j}.bias"] = n.weight.detach(), n.bias.detach()
    keep = [(torch.rand(B, 6) >= 0.3).float() / 0.7, (torch.rand(B, 3) >= 0.3).float() / 0.7]
    got = R.front(params, x, 2, True, keep=keep, dtype=torch.float32)
    # direct: channels-first torch modules, the layer norm on the [B, T, F, C] permutation
    act, h = nn.LeakyReLU(0.01), x[:, None]  # [B, 1, T, F]
    with torch.no_grad():
        for i in range(2):
            for j in (1, 2):
                h = convs[2 * i + j - 1](h)
                h = act(norms[2 * i + j - 1](h.permute(0, 2, 3, 1))).permute(0, 3, 1, 2)
            h = nn.MaxPool2d((1, 2))(h) * keep[i][:, None, None, :]
        h = nn.MaxPool2d((2, 1))(h)  # [B, C, T // 2, F']
    want = h.permute(0, 2, 3, 1).reshape(B, T // 2, -1)
    assert got.shape == (B, 3, 3 * C2) and torch.allclose(got, want, rtol=1e-5, atol=1e-6)
    # the bf16 option rounds MFMA-convolution operands only: with bf16-exact inputs it changes nothing
    xq, wq = torch.randn(1, 4, 5, 3).bfloat16().double(), torch.randn(2, 3, 3, 3).bfloat16().double()
    assert torch.equal(R.conv3x3(xq, wq, None, bf16=True), R.conv3x3(xq, wq, None))
    x1, w1 = torch.randn(1, 4, 5, dtype=torch.float64), torch.randn(2, 1, 3, 3, dtype=torch.float64)
    assert torch.equal(R.conv3x3(x1, w1, None, bf16=True), R.conv3x3(x1, w1, None))  # the first layer: fp32 kernel
    xr = torch.randn(1, 4, 5, 3, dtype=torch.float64)
    assert not torch.equal(R.conv3x3(xr, wq, None, bf16=True), R.conv3x3(xr, wq, None))
