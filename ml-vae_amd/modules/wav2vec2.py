"""The wav2vec2 encoder on the HIP kernels: the call surface of SpeechBrain's HuggingFaceWav2Vec2
with ``freeze: True`` that the w2v_MD_VAE recipes use (ref:src/models/w2v_MD_VAE/model.yaml:11-16,
called at ref:src/models/w2v_MD_VAE/model.py:24), and with ``freeze: False`` plus
``freeze_feature_extractor: True`` (fine-tuning above a frozen conv stack) as w2v_LSTM_FC uses it
(ref:src/models/w2v_LSTM_FC/model.yaml).

``forward(wav [B, N]) -> [B, T_w, hidden]``, T_w = (N - 400) // 320 + 1 at the large-lv60 geometry;
frozen: under no_grad.  The operations, in order:

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

Fine-tuning (``freeze=False, freeze_feature_extractor=True``): steps 1-2 run as above under no_grad
and save nothing; steps 3-7 run through ``ops.W2VHeadFn`` / ``W2VLayerFn`` / ``W2VTailFn`` (the same
kernels in the same order, so the output's bits equal the frozen module's) and their HIP backward.
``parameters()`` then yields the fp32 masters of everything from ``feature_projection`` upward
(``masked_spec_embed`` is unused without masking and stays a frozen tensor); the kernel-side copies
are rebuilt per tensor group when a master's version counter moved (an optimizer step, a load).
``freeze=False`` alone still raises as it always did (the wording is pinned); the whole model --
what SpeechBrain 0.5.x trains under ``freeze: False`` -- is ``freeze=False, train_feature_extractor=True``:
steps 1-2 then run through ``ops.W2VConvFn`` (the same kernels again, the same bits) and its HIP backward
(layer 0 fused and recomputed from the waveform, layers 1.. as residue GEMMs; DESIGN.md section 4, "The
conv stack"), and ``parameters()`` yields every tensor but ``masked_spec_embed``, the
``feature_extractor.conv_layers.*`` ones first, in HuggingFace's order.
Train-mode regularisation (the dropouts, layerdrop, SpecAugment masking) is not built: non-zero
values in a config are ignored with one logged warning, and ``train()`` / ``eval()`` compute the same.

``precision``: 'bf16' (bf16 GEMM and attention operands, fp32 accumulation; the residual stream,
the other GEMM outputs and every LayerNorm / GELU / softmax stay fp32) or 'fp32' (the parity mode:
exact-fp32 GEMMs and the fp32 MFMA in attention).
"""
import json
import logging
import math
import os
from collections import OrderedDict

import torch
from torch import nn

from mlvae_hip import ops

logger = logging.getLogger(__name__)

# the train-mode regularisation of a HuggingFace config: not built (see the module docstring)
REGULARISATION = ("hidden_dropout", "attention_dropout", "activation_dropout", "feat_proj_dropout", "layerdrop",
                  "mask_time_prob", "mask_feature_prob")

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
                 precision="bf16", save_path=None, freeze_feature_extractor=False, train_feature_extractor=False):
        super().__init__()
        del save_path  # SpeechBrain's download cache: nothing is downloaded here
        if train_feature_extractor and (freeze or freeze_feature_extractor):
            raise ValueError("Wav2Vec2: train_feature_extractor=True contradicts freeze=True / "
                             "freeze_feature_extractor=True")
        if not freeze and not freeze_feature_extractor and not train_feature_extractor:
            raise NotImplementedError("Wav2Vec2: freeze=False with freeze_feature_extractor=False is not built: "
                                      "the convolutional feature extractor has no backward; pass "
                                      "freeze_feature_extractor=True to fine-tune everything above it.  The "
                                      "whole model trains with train_feature_extractor=True")
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
        self.freeze, self.freeze_feature_extractor = bool(freeze), bool(freeze_feature_extractor)
        self.train_feature_extractor = bool(train_feature_extractor)
        # the weights under HuggingFace's names (fp32).  Frozen: plain tensors.  Fine-tuning: the trainable
        # ones are nn.Parameters, registered under the same names
        self._w = OrderedDict()
        self._prep = None         # their kernel-side copies: built on the first call, dropped by a load / move
        if not self.freeze and not isinstance(config, str):
            on = [k for k in REGULARISATION if config.get(k)]
            if on:
                logger.warning("Wav2Vec2: train-mode regularisation is not built; ignoring %s",
                               ", ".join(f"{k} = {config[k]}" for k in on))
        if state is None:
            self._init_random()
            self._make_trainable()
        else:
            self._make_trainable()
            self._load_source(state, source)

    @staticmethod
    def trainable_key(key):
        """Whether fine-tuning above a frozen conv stack trains this state-dict key: everything from
        the projection upward (train_feature_extractor adds the feature_extractor.* keys)."""
        return key.startswith(("feature_projection.", "encoder."))

    def _make_trainable(self):
        if self.freeze:
            return
        for key, shape in state_shapes(self.config).items():
            if self.trainable_key(key) or (self.train_feature_extractor and key.startswith("feature_extractor.")):
                t = self._w[key] if key in self._w else torch.zeros(shape)
                # HuggingFace's dotted names: what register_parameter refuses and state_dict needs
                self._parameters[key] = self._w[key] = nn.Parameter(t)

    def _load_source(self, state, source):
        """A HuggingFace state dict from disk: the encoder's keys, bare or under the `wav2vec2.`
        prefix of a pre-training / CTC checkpoint (whose other heads are not read)."""
        if any(k.startswith("wav2vec2.") for k in state):
            state = {k[len("wav2vec2."):]: v for k, v in state.items() if k.startswith("wav2vec2.")}
        shapes = state_shapes(self.config)
        state = {k: v for k, v in state.items() if _POS_OLD.get(k, k) in shapes}
        if "masked_spec_embed" not in state:  # absent when the checkpoint's config masks nothing; unused here
            state["masked_spec_embed"] = torch.zeros(shapes["masked_spec_embed"])
        have = {_POS_OLD.get(k, k) for k in state}
        missing = [k for k in shapes if k not in have]  # (a parameter's placeholder would hide a missing key)
        if missing:
            raise ValueError(f"Wav2Vec2: {source} lacks {len(missing)} of the encoder's tensors "
                             f"(first: {missing[0]})")
        self.load_state_dict(state, strict=False)

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
        super()._apply(fn, *args, **kwargs)  # the parameters
        for k, t in self._w.items():
            if k in self._parameters:
                self._w[k] = self._parameters[k]
                continue
            t = fn(t)
            self._w[k] = t if t.is_floating_point() and t.dtype == torch.float32 else t.float()
        self._prep = None
        return self

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for k, t in self._w.items():  # HuggingFace's order, parameters included
            destination[prefix + k] = t if keep_vars else t.detach()

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
            if key in new and key in self._parameters:
                with torch.no_grad():
                    self._parameters[key].copy_(new[key])
            elif key in new:
                self._w[key] = new[key]
            elif key not in self._w or strict:
                missing_keys.append(prefix + key)
        self._w = OrderedDict((k, self._w[k]) for k in shapes if k in self._w)
        self._prep = None

    def _groups(self):
        """The kernel-side weights by group: name -> (the state-dict keys it is built from, builder).
        A group is rebuilt when one of its keys' tensors was replaced or written (version counter)."""
        cfg = self.config
        wd = torch.bfloat16 if self.precision == "bf16" else torch.float32
        H, G, K = cfg["hidden_size"], cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"]
        Cg = H // G
        scale = (H // cfg["num_attention_heads"]) ** -0.5
        m = lambda t: t.to(wd).contiguous()
        ln = lambda p: ((p + ".weight", p + ".bias"), lambda w, b: (w, b))
        lin = lambda p: ((p + ".weight", p + ".bias"), lambda w, b: (m(w), b))
        out = OrderedDict()
        for i in range(len(cfg["conv_dim"])):
            p = f"feature_extractor.conv_layers.{i}."
            conv = (lambda cw, cb, g, be: (cw[:, 0, :].contiguous(), cb, g, be)) if i == 0 else (
                lambda cw, cb, g, be: (m(cw.permute(0, 2, 1).reshape(cw.shape[0], -1)), cb, g, be))  # [Cout][K][Cin]
            if i > 0 and self.train_feature_extractor:  # with the input gradient's weights: taps regrouped by residue
                conv = (lambda fwd, s: lambda cw, cb, g, be: fwd(cw, cb, g, be) + (
                    ops.w2v_conv_dx_weights(cw, s, wd),))(conv, cfg["conv_stride"][i])
            out[f"conv{i}"] = ((p + "conv.weight", p + "conv.bias", p + "layer_norm.weight", p + "layer_norm.bias"),
                               conv)
        out["proj_ln"] = ln("feature_projection.layer_norm")
        out["proj"] = lin("feature_projection.projection")

        def pos(g, v, b):  # the folded weight [H, Cg, K], output channel o = g Cg + j, regrouped [G][out][K][in]
            return m(fold_pos_conv(g, v).view(G, Cg, Cg, K).permute(0, 1, 3, 2).reshape(G, Cg, K * Cg)), b

        out["pos"] = ((POS_G, POS_V, _POS + "bias"), pos)
        if not self.freeze:  # the input gradient's weight: taps reversed, in / out swapped, [G][in][K][out]
            out["pos_rev"] = ((POS_G, POS_V), lambda g, v: m(
                fold_pos_conv(g, v).view(G, Cg, Cg, K).flip(-1).permute(0, 2, 3, 1).reshape(G, Cg, K * Cg)))
        for i in range(cfg["num_hidden_layers"]):
            p = f"encoder.layers.{i}."
            a = p + "attention."
            out[f"{i}.ln1"] = ln(p + "layer_norm")
            out[f"{i}.qkv"] = (tuple(a + n + s for s in (".weight", ".bias") for n in ("q_proj", "k_proj", "v_proj")),
                               lambda qw, kw, vw, qb, kb, vb: (m(torch.cat([qw * scale, kw, vw])),
                                                               torch.cat([qb * scale, kb, vb]).contiguous()))
            out[f"{i}.out"] = lin(a + "out_proj")
            out[f"{i}.ln2"] = ln(p + "final_layer_norm")
            out[f"{i}.w1"] = lin(p + "feed_forward.intermediate_dense")
            out[f"{i}.w2"] = lin(p + "feed_forward.output_dense")
        out["final_ln"] = ln("encoder.layer_norm")
        return out

    def _prepare(self, dev, P=None):
        """The kernel-side weights: cast, permuted and regrouped.  P: the previous ones, of which only
        the groups whose tensors changed are rebuilt."""
        w = self._w
        wd = torch.bfloat16 if self.precision == "bf16" else torch.float32
        f = lambda k: w[k].detach().to(dev, torch.float32).contiguous()
        if P is None:
            P = {"ver": {}, "conv": [None] * len(self.config["conv_dim"]),
                 "layers": [{} for _ in range(self.config["num_hidden_layers"])]}
        with torch.no_grad():
            for name, (keys, build) in self._groups().items():
                ver = tuple((id(w[k]), w[k]._version) for k in keys)
                if P["ver"].get(name) == ver:
                    continue
                entry = build(*[f(k) for k in keys])
                if name.startswith("conv"):
                    P["conv"][int(name[4:])] = entry
                elif name[0].isdigit():
                    i, part = name.split(".")
                    P["layers"][int(i)][part] = entry
                else:
                    P[name] = entry
                P["ver"][name] = ver
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

    def _conv_stack(self, wav, stages):
        """normalize_wav and the seven conv layers: the last layer's fp32 output [B, T, conv_dim]."""
        cfg, P, eps = self.config, self._prep, self.config["layer_norm_eps"]
        bf = self.precision == "bf16"
        ad = P["dtype"]
        keep = (lambda n, t: stages.__setitem__(n, t.float().clone())) if stages is not None else (lambda n, t: None)

        wav = wav.detach().float().contiguous()
        stats = ops.w2v_tensor_stats(wav) if self.normalize_wav else None
        W, b, g, be = P["conv"][0][:4]
        x = ops.w2v_conv0(wav, stats, W, b, g, be, cfg["conv_stride"][0], eps, out_dtype=ad)
        keep("conv0", x)
        n_conv = len(cfg["conv_dim"])
        xf = x if not bf else None  # the last conv layer's fp32 output feeds the projection's LN
        for i in range(1, n_conv):
            W, b, g, be = P["conv"][i][:4]
            y = ops.w2v_conv_gemm(x, W, b, cfg["conv_kernel"][i], cfg["conv_stride"][i])
            last = i == n_conv - 1
            xf, xb = ops.w2v_rows(y, gamma=g, beta=be, eps=eps, gelu=True, out_f32=last or not bf,
                                  out_bf16=bf and not last)
            x = xb if xb is not None else xf
            keep(f"conv{i}", x)
        if xf is None:  # a one-layer conv stack in bf16: conv0 wrote bf16
            xf = x.float()
        return xf

    def _trainable_tail(self, xf, stages):
        """Everything from the projection upward through the autograd pieces of mlvae_hip.ops."""
        cfg, P, w = self.config, self._prep, self._w
        eps, bf = cfg["layer_norm_eps"], self.precision == "bf16"
        B, T = xf.shape[0], xf.shape[1]
        H, heads = cfg["hidden_size"], cfg["num_attention_heads"]
        G, K = cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"]
        keep = (lambda n, t: stages.__setitem__(n, t.detach().float().clone())) if stages is not None else (
            lambda n, t: None)
        fp = "feature_projection."
        h = ops.W2VHeadFn.apply(xf, P, (B, T, H, G, K, eps, bf), w[fp + "layer_norm.weight"],
                                w[fp + "layer_norm.bias"], w[fp + "projection.weight"], w[fp + "projection.bias"],
                                w[_POS + "bias"], w[POS_G], w[POS_V])
        keep("pos", h.view(B, T, H))
        for i, L in enumerate(P["layers"]):
            p = f"encoder.layers.{i}."
            names = ["layer_norm"] + ["attention." + n for n in ("q_proj", "k_proj", "v_proj", "out_proj")] + [
                "final_layer_norm", "feed_forward.intermediate_dense", "feed_forward.output_dense"]
            masters = [w[p + n + s] for n in names for s in (".weight", ".bias")]
            h = ops.W2VLayerFn.apply(h, L, (B, T, H, heads, eps, bf), *masters)
            keep(f"layer{i}", h.view(B, T, H))
        out = ops.W2VTailFn.apply(h, P, eps, self.output_norm, w["encoder.layer_norm.weight"],
                                  w["encoder.layer_norm.bias"]).view(B, T, H)
        keep("out", out)
        return out

    def forward(self, wav, stages=None):
        """wav [B, N] -> [B, T_w, hidden] fp32.  stages: a dict that receives every intermediate as
        fp32 (tests): conv0.., proj, pos, layer0.., final, out (fine-tuning: no proj and no final)."""
        if self.freeze:
            with torch.no_grad():
                return self._forward(wav, stages)
        return self._forward(wav, stages)

    def _forward(self, wav, stages):
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
        elif not self.freeze:  # an optimizer step since: the changed tensors' copies only
            self._prepare(wav.device, self._prep)
        if self.train_feature_extractor:
            geo = (cfg["conv_kernel"], cfg["conv_stride"], cfg["layer_norm_eps"], self.precision == "bf16",
                   self.normalize_wav, stages)
            masters = [self._w[f"feature_extractor.conv_layers.{i}.{n}"] for i in range(len(cfg["conv_dim"]))
                       for n in ("conv.weight", "conv.bias", "layer_norm.weight", "layer_norm.bias")]
            return self._trainable_tail(ops.W2VConvFn.apply(wav, self._prep, geo, *masters), stages)
        if not self.freeze:
            with torch.no_grad():
                xf = self._conv_stack(wav, stages)
            return self._trainable_tail(xf, stages)
        xf = self._conv_stack(wav, stages)
        P, eps = self._prep, cfg["layer_norm_eps"]
        bf = self.precision == "bf16"
        ad = P["dtype"]
        keep = (lambda n, t: stages.__setitem__(n, t.float().clone())) if stages is not None else (lambda n, t: None)
        act = lambda pair: pair[1] if bf else pair[0]  # w2v_rows' (fp32, bf16) -> the GEMM operand
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
