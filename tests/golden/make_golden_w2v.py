"""Writes tests/golden/w2v_tiny.npz and w2v_tiny_d32.npz: a HuggingFace `transformers`
Wav2Vec2Model of a tiny stable-layer-norm config, filled by tests/w2v_ref.py's fill_state, run in
float64 on a ragged zero-padded [3, 4000] waveform batch with SpeechBrain's two whole-tensor
norms around it; every stage's output is stored rounded to float32 (stages of more than 24 frames
at w2v_ref.keep_frames' subset of frames).  Only the seed, the config, the waveforms and those
outputs are stored: the weights are redrawn from the seed by the tests.

Also prints the error floors the GPU tests' bounds come from (tests/test_gpu_w2v_encoder.py):
w2v_ref in float32 and under bf16 autocast against w2v_ref in float64, per stage.

Run by hand (needs `transformers`, which the tests do not):  python tests/golden/make_golden_w2v.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import w2v_ref as R  # noqa: E402

SEED = 20


def hf_model(cfg, state):
    from transformers import Wav2Vec2Config, Wav2Vec2Model
    model = Wav2Vec2Model(Wav2Vec2Config(**cfg)).eval()
    model.load_state_dict(state)
    return model


def hf_stages(cfg, state, wav):
    """Every stage of the live model in float64, SpeechBrain's two norms around it."""
    model = hf_model(cfg, state).double()
    got = {}
    hooks = []
    for i, layer in enumerate(model.feature_extractor.conv_layers):
        hooks.append(layer.register_forward_hook(
            lambda m, a, out, i=i: got.__setitem__(f"conv{i}", out.transpose(1, 2))))
    hooks.append(model.feature_projection.register_forward_hook(lambda m, a, out: got.__setitem__("proj", out[0])))
    hooks.append(model.encoder.layers[0].register_forward_pre_hook(lambda m, a: got.__setitem__("pos", a[0])))
    for i, layer in enumerate(model.encoder.layers):
        hooks.append(layer.register_forward_hook(lambda m, a, out, i=i: got.__setitem__(f"layer{i}", out[0])))
    with torch.no_grad():
        x = F.layer_norm(wav.double(), wav.shape)
        got["wav_norm"] = x
        got["final"] = model(x).last_hidden_state
        got["out"] = F.layer_norm(got["final"], got["final"].shape)
    for h in hooks:
        h.remove()
    return got


def floors(cfg, state, wav):
    """{stage: (max, relative RMS)} of w2v_ref in fp32 and under bf16 autocast against fp64."""
    with torch.no_grad():
        s64, s32, s16 = {}, {}, {}
        R.forward({k: v.double() for k, v in state.items()}, cfg, wav.double(), stages=s64)
        R.forward(state, cfg, wav, stages=s32)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            R.forward(state, cfg, wav, stages=s16)
    return ({n: R.errors(s32[n], s64[n]) for n in R.stage_names(cfg)},
            {n: R.errors(s16[n], s64[n]) for n in R.stage_names(cfg)})


def main():
    torch.manual_seed(0)
    wav = R.ragged_wav(SEED)
    for name, cfg in (("w2v_tiny", R.TINY), ("w2v_tiny_d32", R.TINY_D32)):
        state = R.fill_state(cfg, SEED)
        got = hf_stages(cfg, state, wav)
        names = R.stage_names(cfg) if name == "w2v_tiny" else ["out"]
        arrays = {"wav": wav.numpy(), "seed": np.int64(SEED), "config": np.array(json.dumps(cfg))}
        for n in names:
            t = got[n]
            if n != "wav_norm":
                t = t[:, R.keep_frames(t.shape[1])]
            arrays[n] = t.numpy().astype(np.float32)
        path = os.path.join(HERE, name + ".npz")
        np.savez(path, **arrays)
        print(f"{path}: {os.path.getsize(path)} bytes")
        f32, bf16 = floors(cfg, state, wav)
        print(f"floors of {name} (max, relative RMS against fp64):")
        for n in R.stage_names(cfg):
            print(f"    {n!r}: fp32 ({f32[n][0]:.2e}, {f32[n][1]:.2e})  bf16 ({bf16[n][0]:.2e}, {bf16[n][1]:.2e})")
    state = R.fill_state(R.TINY, SEED)
    for N in (400, 719, 720, 3520):
        f32, bf16 = floors(R.TINY, state, wav[:, :N].contiguous())
        print(f"    N = {N}: 'out' fp32 ({f32['out'][0]:.2e}, {f32['out'][1]:.2e})  "
              f"bf16 ({bf16['out'][0]:.2e}, {bf16['out'][1]:.2e})")


def yaml_keys(ref_src):
    """w2v_md_vae*_yaml_keys.json: the key names of the reference's two recipe yamls (top level,
    ``modules:``, ``recoverables:``), as make_golden_md_recipe.yaml_keys reads them."""
    import re
    for recipe in ("w2v_MD_VAE", "w2v_MD_VAE_sfl"):
        text = open(os.path.join(ref_src, "models", recipe, "model.yaml")).read()

        def block(name, indent):
            body = re.search(rf"^{indent}{name}:\n((?:{indent}    \S.*\n?)+)", text, flags=re.M).group(1)
            return re.findall(r"^\s+([A-Za-z_][A-Za-z0-9_]*):", body, flags=re.M)

        keys = {"top_level": re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", text, flags=re.M),
                "modules": block("modules", ""), "recoverables": block("recoverables", "    ")}
        with open(os.path.join(HERE, recipe.lower() + "_yaml_keys.json"), "w") as f:
            json.dump(keys, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--yaml-keys":  # needs a checkout of the reference's src/
        yaml_keys(sys.argv[2])
    else:
        main()
