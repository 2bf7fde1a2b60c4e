"""Plain-torch restatement of the frozen wav2vec2 forward (the stable-layer-norm family of the
HuggingFace architecture, wrapped as SpeechBrain's HuggingFaceWav2Vec2 wraps it with freeze=True):
the checker of modules/wav2vec2.py and csrc/w2v.hip.  Written from the published architecture;
tests/test_w2v_cpu.py pins it to a live `transformers` model where that package is importable.

    normalize_wav: F.layer_norm(wav, wav.shape)         -- over the WHOLE padded batch tensor
    7 x (conv -> LN over channels -> GELU); LN(conv_dim) -> Linear(conv_dim -> hidden)
    h += GELU(pos_conv(h))   grouped, pad K/2, the last frame dropped (K even)
    L x { h += out_proj(attn(LN(h)));  h += W2 GELU(W1 LN(h)) };  final LN
    output_norm: F.layer_norm(out, out.shape)           -- again the whole tensor

State dicts use HuggingFace's key names (Wav2Vec2Model.state_dict()).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LARGE_LV60 = dict(
    conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_bias=True,
    feat_extract_norm="layer", feat_extract_activation="gelu", hidden_size=1024, num_hidden_layers=24,
    num_attention_heads=16, intermediate_size=4096, num_conv_pos_embeddings=128,
    num_conv_pos_embedding_groups=16, do_stable_layer_norm=True, hidden_act="gelu", layer_norm_eps=1e-5)

# the fixtures' encoders (tests/golden/make_golden_w2v.py)
TINY = dict(LARGE_LV60, conv_dim=[32] * 7, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
            intermediate_size=256, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)
TINY_D32 = dict(TINY, hidden_size=64, intermediate_size=128)  # 2 heads of d = 32

POS_G = "encoder.pos_conv_embed.conv.parametrizations.weight.original0"
POS_V = "encoder.pos_conv_embed.conv.parametrizations.weight.original1"
POS_G_OLD = "encoder.pos_conv_embed.conv.weight_g"
POS_V_OLD = "encoder.pos_conv_embed.conv.weight_v"


def n_frames(cfg, n):
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        n = (n - k) // s + 1
    return n


def state_shapes(cfg):
    """HuggingFace's key -> shape, in a fixed order (the order fill_state draws in)."""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    K, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    out = {"masked_spec_embed": (H,)}
    cin = 1
    for i, (c, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])):
        p = f"feature_extractor.conv_layers.{i}."
        out[p + "conv.weight"] = (c, cin, k)
        out[p + "conv.bias"] = (c,)
        out[p + "layer_norm.weight"] = (c,)
        out[p + "layer_norm.bias"] = (c,)
        cin = c
    out["feature_projection.layer_norm.weight"] = (cin,)
    out["feature_projection.layer_norm.bias"] = (cin,)
    out["feature_projection.projection.weight"] = (H, cin)
    out["feature_projection.projection.bias"] = (H,)
    out["encoder.pos_conv_embed.conv.bias"] = (H,)
    out[POS_G] = (1, 1, K)
    out[POS_V] = (H, H // G, K)
    out["encoder.layer_norm.weight"] = (H,)
    out["encoder.layer_norm.bias"] = (H,)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out[p + f"attention.{n}.weight"] = (H, H)
            out[p + f"attention.{n}.bias"] = (H,)
        out[p + "layer_norm.weight"] = (H,)
        out[p + "layer_norm.bias"] = (H,)
        out[p + "feed_forward.intermediate_dense.weight"] = (I, H)
        out[p + "feed_forward.intermediate_dense.bias"] = (I,)
        out[p + "feed_forward.output_dense.weight"] = (H, I)
        out[p + "feed_forward.output_dense.bias"] = (H,)
        out[p + "final_layer_norm.weight"] = (H,)
        out[p + "final_layer_norm.bias"] = (H,)
    return out


def fill_state(cfg, seed):
    """A state dict drawn from numpy.random.default_rng(seed): matrices N(0, 1) / sqrt(fan_in), LN
    weights 1 +- 0.1, biases N(0, 0.1), the weight norm's g = the norms of v times 1 +- 0.1."""
    rng = np.random.default_rng(seed)
    state = {}
    for key, shape in state_shapes(cfg).items():
        if key == POS_G:
            continue  # drawn with v below
        if key.endswith("layer_norm.weight"):
            a = 1.0 + 0.1 * rng.uniform(-1.0, 1.0, shape)
        elif key.endswith(".bias") or key == "masked_spec_embed":
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[1:])))
        state[key] = torch.from_numpy(a.astype(np.float32))
        if key == POS_V:
            norm = np.sqrt((a.astype(np.float32).astype(np.float64) ** 2).sum(axis=(0, 1), keepdims=True))
            g = norm * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, norm.shape))
            state[POS_G] = torch.from_numpy(g.astype(np.float32))
    return {k: state[k] for k in state_shapes(cfg)}


def fold_pos_conv(g, v):
    """weight_norm(dim=2): w[:, :, k] = g[k] v[:, :, k] / ||v[:, :, k]||."""
    return v * (g / v.norm(dim=(0, 1), keepdim=True))


def attention(q, k, v, heads):
    """softmax(q k^T) v per head; q already carries the 1 / sqrt(d) scale.  [B, T, H d] each."""
    B, T, C = q.shape
    d = C // heads
    sp = lambda t: t.view(B, T, heads, d).transpose(1, 2)
    p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2), dim=-1)
    return (p.to(v.dtype) @ sp(v)).transpose(1, 2).reshape(B, T, C)


def layer(state, cfg, i, h):
    """One pre-LN transformer layer."""
    eps, H = cfg["layer_norm_eps"], cfg["hidden_size"]
    heads = cfg["num_attention_heads"]
    p = f"encoder.layers.{i}."
    x = F.layer_norm(h, (H,), state[p + "layer_norm.weight"], state[p + "layer_norm.bias"], eps)
    lin = lambda t, n: F.linear(t, state[p + n + ".weight"], state[p + n + ".bias"])
    q = lin(x, "attention.q_proj") * (H // heads) ** -0.5
    a = attention(q, lin(x, "attention.k_proj"), lin(x, "attention.v_proj"), heads)
    h = h + lin(a, "attention.out_proj")
    x = F.layer_norm(h, (H,), state[p + "final_layer_norm.weight"], state[p + "final_layer_norm.bias"], eps)
    return h + lin(F.gelu(lin(x, "feed_forward.intermediate_dense")), "feed_forward.output_dense")


def forward(state, cfg, wav, normalize_wav=True, output_norm=True, stages=None):
    """wav [B, N] -> [B, T_w, hidden].  stages: a dict that receives every intermediate
    (channels-last): conv0..conv6, proj, pos, layer0.., final, out."""
    eps = cfg["layer_norm_eps"]
    keep = (lambda n, t: stages.__setitem__(n, t)) if stages is not None else (lambda n, t: None)
    x = wav
    if normalize_wav:
        x = F.layer_norm(x, x.shape)
    keep("wav_norm", x)
    x = x.unsqueeze(1)  # [B, 1, N]
    for i, s in enumerate(cfg["conv_stride"]):
        p = f"feature_extractor.conv_layers.{i}."
        x = F.conv1d(x, state[p + "conv.weight"], state[p + "conv.bias"], stride=s)
        x = F.layer_norm(x.transpose(1, 2), (x.shape[1],), state[p + "layer_norm.weight"],
                         state[p + "layer_norm.bias"], eps)
        x = F.gelu(x).transpose(1, 2)
        keep(f"conv{i}", x.transpose(1, 2))
    x = x.transpose(1, 2)  # [B, T, C]
    x = F.layer_norm(x, (x.shape[-1],), state["feature_projection.layer_norm.weight"],
                     state["feature_projection.layer_norm.bias"], eps)
    h = F.linear(x, state["feature_projection.projection.weight"], state["feature_projection.projection.bias"])
    keep("proj", h)
    K, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    g = state[POS_G] if POS_G in state else state[POS_G_OLD]
    v = state[POS_V] if POS_V in state else state[POS_V_OLD]
    pos = F.conv1d(h.transpose(1, 2), fold_pos_conv(g, v), state["encoder.pos_conv_embed.conv.bias"],
                   padding=K // 2, groups=G)
    if K % 2 == 0:
        pos = pos[:, :, :-1]
    h = h + F.gelu(pos).transpose(1, 2)
    keep("pos", h)
    for i in range(cfg["num_hidden_layers"]):
        h = layer(state, cfg, i, h)
        keep(f"layer{i}", h)
    h = F.layer_norm(h, (h.shape[-1],), state["encoder.layer_norm.weight"], state["encoder.layer_norm.bias"], eps)
    keep("final", h)
    if output_norm:
        h = F.layer_norm(h, h.shape)
    keep("out", h)
    return h


def stage_names(cfg):
    return (["wav_norm"] + [f"conv{i}" for i in range(len(cfg["conv_dim"]))] + ["proj", "pos"]
            + [f"layer{i}" for i in range(cfg["num_hidden_layers"])] + ["final", "out"])


def keep_frames(T):
    """The frames of a T-frame stage the fixtures store: all of them up to 24, else every 16th plus
    the first and the last four (the conv stack's long early layers would not fit a small file)."""
    if T <= 24:
        return list(range(T))
    return sorted(set(range(0, T, 16)) | set(range(4)) | set(range(T - 4, T)))


def ragged_wav(seed, B=3, N=4000, lens=(4000, 3100, 1700)):
    """The fixtures' waveform batch: noise plus a tone, zero-padded past each utterance's length."""
    rng = np.random.default_rng(seed)
    t = np.arange(N) / 16000.0
    wav = np.zeros((B, N), dtype=np.float32)
    for b in range(B):
        w = 0.1 * rng.standard_normal(N) + 0.3 * np.sin(2 * np.pi * (200.0 + 150.0 * b) * t)
        wav[b, :lens[b]] = w[:lens[b]].astype(np.float32)
    return torch.from_numpy(wav)


def errors(got, ref):
    """(max |got - ref|, relative RMS) against a float64 reference."""
    d = got.double() - ref.double()
    return d.abs().max().item(), (d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt().clamp_min(1e-300)).item()
