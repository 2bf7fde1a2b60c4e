"""The frozen wav2vec2 encoder on the HIP kernels: the call surface of SpeechBrain's
HuggingFaceWav2Vec2 with ``freeze: True`` that the w2v_MD_VAE recipes use
(ref:src/models/w2v_MD_VAE/model.yaml:11-16, called at ref:src/models/w2v_MD_VAE/model.py:24).

Forward only, under no_grad: ``forward(wav [B, N]) -> [B, T_w, hidden]``, T_w = (N - 400) // 320 + 1
at the large-lv60 geometry.  The operations, in order:

1. ``normalize_wav``: ``F.layer_norm(wav, wav.shape)`` -- over the WHOLE padded batch tensor, zero
   padding and every utterance included, as SpeechBrain 0.5.x does.  The utterances of a batch are
   coupled by it.
2. seven conv layers, each conv -> LayerNorm over channels -> GELU
3. LayerNorm(conv_dim) -> Linear(conv_dim -> hidden)
4. ``h += GELU(pos_conv(h))``: grouped conv, padding K/2, the last frame dropped
5. the pre-LN transformer layers: ``h += out_proj(attn(LN(h)))``, ``h += W2 GELU(W1 LN(h))``
6. the final LayerNorm
7. ``output_norm``: ``F.layer_norm(out, out.shape)`` -- again over the WHOLE [B, T_w, hidden] tensor

There is no attention mask: padded samples are processed and attended to, as the reference's call
``self.modules['wav2vec2'](wavs)`` (no lengths) does.  SpeechBrain's behaviour is restated from its
documentation; parity with it is unpinned.  tests/w2v_ref.py restates this forward in plain torch
and tests/test_w2v_cpu.py pins that to a live ``transformers`` model.

Models are never fetched by name.  ``source`` is None (random weights from ``config``, drawn from
the torch RNG) or a local directory holding ``config.json`` and ``pytorch_model.bin`` or
``model.safetensors``.  The weights are frozen tensors kept under HuggingFace's state-dict key
names, so a checkpoint round-trips and a real HuggingFace state dict loads; the positional conv's
weight norm is accepted as ``weight_g`` / ``weight_v`` or ``parametrizations.weight.original0/1``.
Casting, permuting and regrouping the weights for the kernels (the weight norm folded, Q / K / V
fused with 1 / sqrt(d) in the Q rows, conv weights as [Cout][K][Cin], the positional conv as
[G][out][K][in]) happens once, on the first call after a load or a move.

``precision``: 'bf16' (bf16 GEMM and attention operands, fp32 accumulation; the residual stream,
the other GEMM outputs and every LayerNorm / GELU / softmax stay fp32) or 'fp32' (the parity mode:
exact-fp32 GEMMs and the fp32 MFMA in attention).
"""
import json
import math
import os
from collections import OrderedDict

import torch
from torch import nn

from mlvae_hip import ops

LARGE_LV60 = dict(
    conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_bias=True,
    feat_extract_norm="layer", feat_extract_activation="gelu", hidden_size=1024, num_hidden_layers=24,
    num_attention_heads=16, intermediate_size=4096, num_conv_pos_embeddings=128,
    num_conv_pos_embedding_groups=16, do_stable_layer_norm=True, hidden_act="gelu", layer_norm_eps=1e-5)

_POS = "encoder.pos_conv_embed.conv."
POS_G, POS_V = _POS + "parametrizations.weight.original0", _POS + "parametrizations.weight.original1"
_POS_OLD = {_POS + "weight_g": POS_G, _POS + "weight_v": POS_V}

_FETCH = ("models are never fetched by name: download the model yourself and point `source` at the local "
          "directory that holds its config.json and pytorch_model.bin (or model.safetensors), or use "
          "source: null for random weights from `config`")


def resolve_config(config):
    """The validated architecture mapping ('large_lv60' or a mapping with its keys)."""
    if isinstance(config, str):
        if config != "large_lv60":
            raise ValueError(f"Wav2Vec2: unknown config name {config!r} (only 'large_lv60'; or pass a mapping)")
        config = LARGE_LV60
    cfg = dict(LARGE_LV60)
    cfg.update({k: config[k] for k in config if k in LARGE_LV60})
    for k in ("conv_dim", "conv_kernel", "conv_stride"):
        cfg[k] = [int(v) for v in cfg[k]]
    if cfg["feat_extract_norm"] != "layer" or not cfg["do_stable_layer_norm"]:
        raise ValueError("Wav2Vec2: only the feat_extract_norm = 'layer' / do_stable_layer_norm = true family "
                         "(wav2vec2-large-lv60 and its kin) is built; the group-norm / post-LN family is not")
    if not cfg["conv_bias"]:
        raise ValueError("Wav2Vec2: conv_bias = false is not built")
    if cfg["hidden_act"] != "gelu" or cfg["feat_extract_activation"] != "gelu":
        raise ValueError("Wav2Vec2: only the exact-erf GELU activation is built")
    if not (len(cfg["conv_dim"]) == len(cfg["conv_kernel"]) == len(cfg["conv_stride"]) >= 1):
        raise ValueError("Wav2Vec2: conv_dim, conv_kernel and conv_stride must have one entry per layer")
    H, heads, G = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_conv_pos_embedding_groups"]
    if H % heads or H % G:
        raise ValueError(f"Wav2Vec2: hidden_size {H} must divide by the heads ({heads}) and the groups ({G})")
    if cfg["num_conv_pos_embeddings"] % 2:
        raise ValueError("Wav2Vec2: an odd positional-conv kernel is not built")
    # the bf16 GEMM's 16-byte operand chunks
    if any(c % 8 for c in cfg["conv_dim"]) or H % 8 or (H // G) % 8 or cfg["intermediate_size"] % 8:
        raise ValueError("Wav2Vec2: conv_dim, hidden_size, hidden_size / groups and intermediate_size must be "
                         "multiples of 8")
    return cfg


def state_shapes(cfg):
    """HuggingFace's Wav2Vec2Model state-dict keys -> shapes."""
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    K, G = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    out = OrderedDict(masked_spec_embed=(H,))
    cin = 1
    for i, (c, k) in enumerate(zip(cfg["conv_dim"], cfg["conv_kernel"])):
        p = f"feature_extractor.conv_layers.{i}."
        out[p + "conv.weight"], out[p + "conv.bias"] = (c, cin, k), (c,)
        out[p + "layer_norm.weight"], out[p + "layer_norm.bias"] = (c,), (c,)
        cin = c
    out["feature_projection.layer_norm.weight"], out["feature_projection.layer_norm.bias"] = (cin,), (cin,)
    out["feature_projection.projection.weight"], out["feature_projection.projection.bias"] = (H, cin), (H,)
    out[_POS + "bias"] = (H,)
    out[POS_G], out[POS_V] = (1, 1, K), (H, H // G, K)
    out["encoder.layer_norm.weight"], out["encoder.layer_norm.bias"] = (H,), (H,)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out[p + f"attention.{n}.weight"], out[p + f"attention.{n}.bias"] = (H, H), (H,)
        out[p + "layer_norm.weight"], out[p + "layer_norm.bias"] = (H,), (H,)
        out[p + "feed_forward.intermediate_dense.weight"] = (I, H)
        out[p + "feed_forward.intermediate_dense.bias"] = (I,)
        out[p + "feed_forward.output_dense.weight"] = (H, I)
        out[p + "feed_forward.output_dense.bias"] = (H,)
        out[p + "final_layer_norm.weight"], out[p + "final_layer_norm.bias"] = (H,), (H,)
    return out


def fold_pos_conv(g, v):
    """weight_norm(dim=2) folded: w[:, :, k] = g[k] v[:, :, k] / ||v[:, :, k]||."""
    return v * (g / v.norm(dim=(0, 1), keepdim=True))


def _read_state(source):
    bin_path, st_path = os.path.join(source, "pytorch_model.bin"), os.path.join(source, "model.safetensors")
    if os.path.isfile(bin_path):
        return torch.load(bin_path, map_location="cpu", weights_only=True)
    if os.path.isfile(st_path):
        try:
            from safetensors.torch import load_file
        except ImportError as e:
            raise ValueError(f"Wav2Vec2: {st_path} needs the safetensors package; save the weights as "
                             "pytorch_model.bin instead") from e
        return load_file(st_path)
    raise ValueError(f"Wav2Vec2: {source} holds neither pytorch_model.bin nor model.safetensors; " + _FETCH)


class Wav2Vec2(nn.Module):
    def __init__(self, source=None, config="large_lv60", output_norm=True, freeze=True, normalize_wav=True,
                 precision="bf16", save_path=None):
        super().__init__()
        del save_path  # SpeechBrain's download cache: nothing is downloaded here
        if not freeze:
            raise NotImplementedError("Wav2Vec2: freeze=False (fine-tuning) is not built: the encoder has no "
                                      "backward")
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"Wav2Vec2: precision must be 'bf16' or 'fp32', got {precision!r}")
        state = None
        if source is not None:
            if not (isinstance(source, (str, os.PathLike)) and os.path.isdir(source)):
                raise ValueError(f"Wav2Vec2: source {source!r} is not an existing directory; " + _FETCH)
            cfg_path = os.path.join(source, "config.json")
            if not os.path.isfile(cfg_path):
                raise ValueError(f"Wav2Vec2: {source} has no config.json; " + _FETCH)
            with open(cfg_path) as f:
                config = json.load(f)
            state = _read_state(os.fspath(source))
        self.config = resolve_config(config)
        self.output_norm, self.normalize_wav, self.precision = bool(output_norm), bool(normalize_wav), precision
        self.freeze = True
        self._w = OrderedDict()   # the frozen weights under HuggingFace's names (fp32, no grad)
        self._prep = None         # their kernel-side copies: built on the first call, dropped by a load / move
        if state is None:
            self._init_random()
        else:
            self._load_source(state, source)

    def _load_source(self, state, source):
        """A HuggingFace state dict from disk: the encoder's keys, bare or under the `wav2vec2.`
        prefix of a pre-training / CTC checkpoint (whose other heads are not read)."""
        if any(k.startswith("wav2vec2.") for k in state):
            state = {k[len("wav2vec2."):]: v for k, v in state.items() if k.startswith("wav2vec2.")}
        shapes = state_shapes(self.config)
        state = {k: v for k, v in state.items() if _POS_OLD.get(k, k) in shapes}
        if "masked_spec_embed" not in state:  # absent when the checkpoint's config masks nothing; unused here
            state["masked_spec_embed"] = torch.zeros(shapes["masked_spec_embed"])
        res = self.load_state_dict(state, strict=False)
        if res.missing_keys:
            raise ValueError(f"Wav2Vec2: {source} lacks {len(res.missing_keys)} of the encoder's tensors "
                             f"(first: {res.missing_keys[0]})")

    # ------------------------------------------------------------------ weights
    def _init_random(self):
        for key, shape in state_shapes(self.config).items():
            if key == POS_G:
                continue
            if key.endswith("layer_norm.weight"):
                t = torch.ones(shape)
            elif key.endswith(".bias"):
                t = torch.zeros(shape)
            elif key == "masked_spec_embed":
                t = torch.rand(shape)
            else:
                t = torch.randn(shape) / math.sqrt(math.prod(shape[1:]))
            self._w[key] = t
            if key == POS_V:  # weight_norm's initial g: the norms of v (the folded weight is v)
                self._w[POS_G] = t.norm(dim=(0, 1), keepdim=True)
        self._w = OrderedDict((k, self._w[k]) for k in state_shapes(self.config))

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        for k, t in self._w.items():
            t = fn(t)
            self._w[k] = t if t.is_floating_point() and t.dtype == torch.float32 else t.float()
        self._prep = None
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        for k, t in self._w.items():
            destination[prefix + k] = t

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        shapes = state_shapes(self.config)
        seen = set()
        dev = next(iter(self._w.values())).device if self._w else torch.device("cpu")
        new = OrderedDict()
        for full, t in state_dict.items():
            if not full.startswith(prefix):
                continue
            key = full[len(prefix):]
            key = _POS_OLD.get(key, key)
            if key not in shapes:
                unexpected_keys.append(full)
                continue
            if tuple(t.shape) != tuple(shapes[key]):
                error_msgs.append(f"size mismatch for {full}: {tuple(t.shape)} in the checkpoint, "
                                  f"{tuple(shapes[key])} in the model")
                continue
            new[key] = t.detach().to(dev, torch.float32).clone()
            seen.add(key)
        for key in shapes:
            if key in new:
                self._w[key] = new[key]
            elif key not in self._w or strict:
                missing_keys.append(prefix + key)
        self._w = OrderedDict((k, self._w[k]) for k in shapes if k in self._w)
        self._prep = None

    def _prepare(self, dev):
        """The kernel-side weights: cast, permuted and regrouped once."""
        cfg, w = self.config, self._w
        wd = torch.bfloat16 if self.precision == "bf16" else torch.float32
        f = lambda k: w[k].to(dev, torch.float32).contiguous()
        m = lambda t: t.to(dev, wd).contiguous()
        ln = lambda p: (f(p + ".weight"), f(p + ".bias"))
        P = {"conv": [], "layers": []}
        for i in range(len(cfg["conv_dim"])):
            p = f"feature_extractor.conv_layers.{i}."
            cw = f(p + "conv.weight")  # [Cout, Cin, K]
            W = cw[:, 0, :].contiguous() if i == 0 else m(cw.permute(0, 2, 1).reshape(cw.shape[0], -1))
            P["conv"].append((W, f(p + "conv.bias")) + ln(p + "layer_norm"))
        P["proj_ln"] = ln("feature_projection.layer_norm")
        P["proj"] = (m(f("feature_projection.projection.weight")), f("feature_projection.projection.bias"))
        H, G, K = cfg["hidden_size"], cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"]
        Cg = H // G
        pw = fold_pos_conv(f(POS_G), f(POS_V))  # [H, Cg, K], output channel o = g Cg + j
        P["pos"] = (m(pw.view(G, Cg, Cg, K).permute(0, 1, 3, 2).reshape(G, Cg, K * Cg)), f(_POS + "bias"))
        scale = (H // cfg["num_attention_heads"]) ** -0.5
        for i in range(cfg["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            a = p + "attention."
            wqkv = torch.cat([f(a + "q_proj.weight") * scale, f(a + "k_proj.weight"), f(a + "v_proj.weight")])
            bqkv = torch.cat([f(a + "q_proj.bias") * scale, f(a + "k_proj.bias"), f(a + "v_proj.bias")])
            P["layers"].append(dict(
                ln1=ln(p + "layer_norm"), qkv=(m(wqkv), bqkv.contiguous()),
                out=(m(f(a + "out_proj.weight")), f(a + "out_proj.bias")), ln2=ln(p + "final_layer_norm"),
                w1=(m(f(p + "feed_forward.intermediate_dense.weight")), f(p + "feed_forward.intermediate_dense.bias")),
                w2=(m(f(p + "feed_forward.output_dense.weight")), f(p + "feed_forward.output_dense.bias"))))
        P["final_ln"] = ln("encoder.layer_norm")
        P["dev"], P["dtype"] = dev, wd
        return P

    # ------------------------------------------------------------------ forward
    def n_frames(self, n):
        for k, s in zip(self.config["conv_kernel"], self.config["conv_stride"]):
            n = (n - k) // s + 1
        return n

    def supported(self, T):
        """Whether the attention kernel takes T frames at this model's heads and head width."""
        H, heads = self.config["hidden_size"], self.config["num_attention_heads"]
        return ops.w2v_attention_supported(T, heads, H // heads)

    @torch.no_grad()
    def forward(self, wav, stages=None):
        """wav [B, N] -> [B, T_w, hidden] fp32.  stages: a dict that receives every intermediate as
        fp32 (tests): conv0.., proj, pos, layer0.., final, out."""
        if wav.dim() != 2:
            raise ValueError(f"Wav2Vec2: wav must be [B, N], got {tuple(wav.shape)}")
        if not wav.is_cuda:
            raise TypeError("Wav2Vec2: the encoder runs on the HIP device only (there is no CPU fallback)")
        cfg = self.config
        B, N = wav.shape
        T = self.n_frames(N)
        if T < 1:
            raise ValueError(f"Wav2Vec2: {N} samples give no frame")
        H, heads = cfg["hidden_size"], cfg["num_attention_heads"]
        d = H // heads
        if not self.supported(T):
            raise ValueError(f"Wav2Vec2: attention over T = {T} frames with {heads} heads of width {d} is "
                             "unsupported by the HIP kernel (head width 32 or 64); there is no fallback")
        if self._prep is None or self._prep["dev"] != wav.device or self._prep["dtype"] != (
                torch.bfloat16 if self.precision == "bf16" else torch.float32):
            self._prep = self._prepare(wav.device)
        P, eps = self._prep, cfg["layer_norm_eps"]
        bf = self.precision == "bf16"
        ad = P["dtype"]
        keep = (lambda n, t: stages.__setitem__(n, t.float().clone())) if stages is not None else (lambda n, t: None)
        act = lambda pair: pair[1] if bf else pair[0]  # w2v_rows' (fp32, bf16) -> the GEMM operand

        wav = wav.detach().float().contiguous()
        stats = ops.w2v_tensor_stats(wav) if self.normalize_wav else None
        W, b, g, be = P["conv"][0]
        x = ops.w2v_conv0(wav, stats, W, b, g, be, cfg["conv_stride"][0], eps, out_dtype=ad)
        keep("conv0", x)
        n_conv = len(cfg["conv_dim"])
        xf = x if not bf else None  # the last conv layer's fp32 output feeds the projection's LN
        for i in range(1, n_conv):
            W, b, g, be = P["conv"][i]
            y = ops.w2v_conv_gemm(x, W, b, cfg["conv_kernel"][i], cfg["conv_stride"][i])
            last = i == n_conv - 1
            xf, xb = ops.w2v_rows(y, gamma=g, beta=be, eps=eps, gelu=True, out_f32=last or not bf,
                                  out_bf16=bf and not last)
            x = xb if xb is not None else xf
            keep(f"conv{i}", x)
        if xf is None:  # a one-layer conv stack in bf16: conv0 wrote bf16
            xf = x.float()
        x = act(ops.w2v_rows(xf.view(B * T, -1), gamma=P["proj_ln"][0], beta=P["proj_ln"][1], eps=eps,
                             out_f32=not bf, out_bf16=bf))
        h = ops.w2v_linear(x, *P["proj"])  # the fp32 residual stream [B T, H]
        keep("proj", h.view(B, T, H))

        G, K = cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"]
        hp = ops.w2v_regroup(h.view(B, T, H), G, K, out_dtype=ad)
        pc = ops.w2v_pos_conv(hp, P["pos"][0], T, H)
        ops.w2v_rows(pc.view(B * T, H), bias=P["pos"][1], gelu=True, res=h, out_f32=h)  # h += GELU(conv + b)
        keep("pos", h.view(B, T, H))

        for i, L in enumerate(P["layers"]):
            x = act(ops.w2v_rows(h, gamma=L["ln1"][0], beta=L["ln1"][1], eps=eps, out_f32=not bf, out_bf16=bf))
            qkv = ops.w2v_linear(x, *L["qkv"], out_dtype=ad)  # bf16 mode: what attention's MFMA reads
            a = ops.w2v_attention(qkv, B, T, heads, d, f32_math=not bf, out_dtype=ad)
            ops.w2v_linear(a, *L["out"], out=h, beta=1.0)
            x = act(ops.w2v_rows(h, gamma=L["ln2"][0], beta=L["ln2"][1], eps=eps, out_f32=not bf, out_bf16=bf))
            f1 = ops.w2v_linear(x, *L["w1"])
            x = act(ops.w2v_rows(f1, gelu=True, out_f32=not bf, out_bf16=bf))
            ops.w2v_linear(x, *L["w2"], out=h, beta=1.0)
            keep(f"layer{i}", h.view(B, T, H))
        out = ops.w2v_rows(h, gamma=P["final_ln"][0], beta=P["final_ln"][1], eps=eps, out_f32=True)[0]
        keep("final", out.view(B, T, H))
        if self.output_norm:
            out = ops.w2v_scale_shift(out, ops.w2v_tensor_stats(out))
        out = out.view(B, T, H)
        keep("out", out)
        return out
