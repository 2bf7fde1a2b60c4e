"""The wav2vec2 encoder's and the w2v_MD_VAE recipes' host-side parts (no GPU):

* tests/w2v_ref.py, the plain-torch restatement the GPU tests check the kernels against, matches
  every stage the HuggingFace fixture stores (tests/golden/w2v_tiny*.npz, make_golden_w2v.py) and,
  where `transformers` is importable, the live model at 400, 719, 720 and 3520 samples (1, 1, 2
  and 10 frames);
* modules.wav2vec2.Wav2Vec2: HuggingFace's state-dict key set, both spellings of the positional
  conv's weight norm, the local-directory load, and the three refusals (a model name as `source`,
  freeze=False, the group-norm family);
* models/w2v_MD_VAE*/model.yaml through load_hyperpyyaml against the reference yamls' key names,
  and the recipes' forward wiring with recording stand-in modules: the 1-or-2-frame padding, each
  FC to its own consumer, the un-normalised decoder target, one encoder pass per batch.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

import w2v_ref as R
from conftest import PKG

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    cfg = json.loads(str(z["config"]))
    return z, cfg, R.fill_state(cfg, int(z["seed"]))


def f64(state):
    return {k: v.double() for k, v in state.items()}


# --------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["w2v_tiny", "w2v_tiny_d32"])
def test_ref_matches_every_stored_stage(name):
    z, cfg, state = fixture(name)
    assert json.loads(str(z["config"])) == (R.TINY if name == "w2v_tiny" else R.TINY_D32)
    wav = torch.from_numpy(z["wav"])
    assert wav.shape == (3, 4000) and bool((wav[1, 3100:] == 0).all()) and bool((wav[2, 1700:] == 0).all())
    assert torch.equal(wav, R.ragged_wav(int(z["seed"])))
    stages = {}
    with torch.no_grad():
        out = R.forward(f64(state), cfg, wav.double(), stages=stages)
    assert out.shape == (3, 12, cfg["hidden_size"]) and R.n_frames(cfg, 4000) == 12
    names = R.stage_names(cfg) if name == "w2v_tiny" else ["out"]
    assert set(names) <= set(z.files)
    for n in names:
        got = stages[n] if n == "wav_norm" else stages[n][:, R.keep_frames(stages[n].shape[1])]
        stored = torch.from_numpy(z[n]).double()
        assert got.shape == stored.shape, n
        # the live model's float64 output rounded to float32: half an ulp, held to one
        err = (got - stored).abs()
        print(f"{name} {n}: max |ref - stored| {err.max().item():.2e}")
        assert bool((err <= 2.0 ** -23 * stored.abs() + 1e-12).all()), n


@pytest.mark.parametrize("N", [400, 719, 720, 3520])
def test_ref_matches_the_live_model(N):
    transformers = pytest.importorskip("transformers")
    z, cfg, state = fixture("w2v_tiny")
    model = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**cfg)).eval().double()
    model.load_state_dict(f64(state))  # strict: the key set is HuggingFace's
    wav = torch.from_numpy(z["wav"])[:, :N].double()
    with torch.no_grad():
        want = model(wav).last_hidden_state
        got = R.forward(f64(state), cfg, wav, normalize_wav=False, output_norm=False)
    assert got.shape == want.shape == (3, (N - 400) // 320 + 1, cfg["hidden_size"])
    err = (got - want).abs().max().item()
    print(f"N={N}: {got.shape[1]} frames, max |ref - live| {err:.2e}")
    assert err <= 1e-12 * want.abs().max().item()  # float64 on both sides: summation order only


# --------------------------------------------------------------------------- the module
def test_state_dict_keys_are_huggingfaces():
    from modules.wav2vec2 import Wav2Vec2
    m = Wav2Vec2(config=R.TINY)
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(R.state_shapes(R.TINY))
    assert list(m.parameters()) == [] and all(not v.requires_grad for v in sd.values())
    try:
        import transformers
    except ImportError:
        return
    live = transformers.Wav2Vec2Model(transformers.Wav2Vec2Config(**R.TINY)).state_dict()
    assert {k: tuple(v.shape) for k, v in live.items()} == {k: tuple(v.shape) for k, v in sd.items()}


def test_both_weight_norm_spellings_fold_to_the_same_weight():
    from modules.wav2vec2 import POS_G, POS_V, Wav2Vec2, fold_pos_conv
    state = R.fill_state(R.TINY, 4)
    old = {{R.POS_G: R.POS_G_OLD, R.POS_V: R.POS_V_OLD}.get(k, k): v for k, v in state.items()}
    assert R.POS_G_OLD in old and R.POS_G not in old
    a, b = Wav2Vec2(config=R.TINY), Wav2Vec2(config=R.TINY)
    a.load_state_dict(state)
    b.load_state_dict(old)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
    w = fold_pos_conv(sa[POS_G], sa[POS_V])
    assert torch.equal(w, fold_pos_conv(sb[POS_G], sb[POS_V]))
    # weight_norm(dim=2): every kernel tap's slice has norm g[k]
    assert torch.allclose(w.norm(dim=(0, 1)), state[R.POS_G].flatten(), rtol=1e-5)
    assert torch.allclose(w, R.fold_pos_conv(state[R.POS_G], state[R.POS_V]))
    with pytest.raises(RuntimeError, match="Unexpected key"):
        a.load_state_dict(dict(state, bogus=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="size mismatch"):
        a.load_state_dict(dict(state, masked_spec_embed=torch.zeros(3)))


def test_local_directory_load_round_trips(tmp_path):
    from modules.wav2vec2 import Wav2Vec2
    torch.manual_seed(1)
    a = Wav2Vec2(config=R.TINY_D32, precision="fp32")
    torch.manual_seed(1)
    again = Wav2Vec2(config=R.TINY_D32)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in a.state_dict().items())  # the torch RNG seeds it
    with open(tmp_path / "config.json", "w") as f:
        json.dump(dict(R.TINY_D32, model_type="wav2vec2", vocab_size=32), f)  # a real file's other keys pass
    torch.save(a.state_dict(), tmp_path / "pytorch_model.bin")
    b = Wav2Vec2(source=str(tmp_path), save_path="ignored")
    assert b.config == a.config and b.config["hidden_size"] == 64
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    # a pre-training / CTC checkpoint keeps the encoder under `wav2vec2.`, next to other heads
    torch.save({**{"wav2vec2." + k: v for k, v in sa.items()}, "lm_head.weight": torch.zeros(2, 2)},
               tmp_path / "pytorch_model.bin")
    c = Wav2Vec2(source=str(tmp_path)).state_dict()
    assert all(torch.equal(sa[k], c[k]) for k in sa)
    os.remove(tmp_path / "pytorch_model.bin")
    with pytest.raises(ValueError, match="neither pytorch_model.bin nor model.safetensors"):
        Wav2Vec2(source=str(tmp_path))


def test_refusals():
    from modules.wav2vec2 import Wav2Vec2
    with pytest.raises(ValueError, match="never fetched by name") as e:
        Wav2Vec2(source="facebook/wav2vec2-large-lv60")
    assert "local" in str(e.value) and "config.json" in str(e.value)
    with pytest.raises(NotImplementedError, match="no\\s+backward"):
        Wav2Vec2(config=R.TINY, freeze=False)
    with pytest.raises(ValueError, match="group-norm"):
        Wav2Vec2(config=dict(R.TINY, feat_extract_norm="group", do_stable_layer_norm=False))
    with pytest.raises(ValueError, match="group-norm"):
        Wav2Vec2(config=dict(R.TINY, do_stable_layer_norm=False))
    with pytest.raises(ValueError, match="precision"):
        Wav2Vec2(config=R.TINY, precision="fp16")
    with pytest.raises(TypeError, match="no CPU fallback"):
        Wav2Vec2(config=R.TINY)(torch.zeros(1, 4000))
    from modules.wav2vec2 import LARGE_LV60, resolve_config
    assert resolve_config("large_lv60") == LARGE_LV60 == R.LARGE_LV60
    m = Wav2Vec2(config=R.TINY)
    assert [m.n_frames(n) for n in (400, 719, 720, 3520, 80000)] == [1, 1, 2, 10, 249]


# --------------------------------------------------------------------------- the recipes' yaml
SMALL = {"model": {"wav2vec2_size": 128, "wav2vec2_config": {
    "conv_dim": [32] * 7, "num_hidden_layers": 2, "num_attention_heads": 2, "intermediate_size": 256,
    "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4}}}


@pytest.mark.parametrize("recipe", ["w2v_MD_VAE", "w2v_MD_VAE_sfl"])
def test_model_yaml_resolves_with_the_reference_keys(recipe):
    import functools
    from hyperpyyaml import load_hyperpyyaml
    from mlvae_hip import optim as hip_optim
    from modules.wav2vec2 import Wav2Vec2
    ov = (f"dataset: synthetic\nmodel_class: {recipe}\nmodel_name: x\n"
          f"model: !include:../models/{recipe}/model.yaml\n")
    with open(os.path.join(PKG, "config", "run.yaml")) as f:
        hp = load_hyperpyyaml(f, [SMALL, ov])  # the README's small encoder: the default is 315 M weights
    m = hp["model"]
    with open(os.path.join(GOLD, recipe.lower() + "_yaml_keys.json")) as f:
        ref = json.load(f)
    assert list(m["modules"].keys()) == ref["modules"]
    assert list(m["checkpointer"].recoverables.keys()) == ref["recoverables"]
    assert set(ref["top_level"]) <= set(m.keys())
    import re
    with open(os.path.join(PKG, "models", recipe, "model.yaml")) as f:
        own = re.findall(r"^([A-Za-z_][A-Za-z0-9_]*):", f.read(), flags=re.M)
    assert set(own) - set(ref["top_level"]) == {"wav2vec2_config", "wav2vec2_precision"}
    assert set(ref["top_level"]) - set(own) == set()
    enc = m["wav2vec2"]
    assert isinstance(enc, Wav2Vec2) and m["modules"]["wav2vec2"] is enc and enc.precision == "bf16"
    assert enc.output_norm and enc.normalize_wav and enc.config["hidden_size"] == 128
    assert enc.config["conv_kernel"] == [10, 3, 3, 3, 3, 2, 2] and enc.config["num_conv_pos_embeddings"] == 16
    # one optimizer group, the reference's module list; wav2vec_opt (frozen encoder) is dropped
    assert list(m["optimizers"]) == ["adam_opt"]
    opt = m["optimizers"]["adam_opt"]
    assert isinstance(opt["opt_class"], functools.partial) and opt["opt_class"].func is hip_optim.Adam
    assert opt["modules"] == ["w2v_feat_fc", "phn_recog_in_fc", "phoneme_recognizer", "phn_recog_out_fc",
                              "b_detector_in_fc", "boundary_detector", "concat_fc", "rnn", "pi_fc", "encoder",
                              "decoder"]
    for name in ("w2v_feat_fc", "phn_recog_in_fc", "b_detector_in_fc"):
        lin = [b for b in m[name].blocks if isinstance(b, torch.nn.Linear)]
        assert [(l.in_features, l.out_features) for l in lin] == [(128, 512), (512, 256)], name
    assert m["concat_fc"].blocks[0].in_features == 256 + 32
    assert m["max_key"] == "plvl_md.F1" and m["metric_keys"][-6:] == [
        "plvl_md.ACC", "plvl_md.PRE", "plvl_md.REC", "plvl_md.F1", "boundary.f1", "boundary.r_value"]
    if recipe.endswith("_sfl"):
        assert m["pi_mcmc_num"] == 5 and m["rif_weight"] == 1 and "baseline_fc" in m["modules"]
    else:
        assert (m["boundary_kld_weight"], m["vae_kld_weight"], m["pi_nll_weight"]) == (1e-5, 1e-5, 0.1)


def test_default_config_is_large_lv60():
    from hyperpyyaml import load_hyperpyyaml
    from modules.wav2vec2 import LARGE_LV60, resolve_config
    with open(os.path.join(PKG, "models", "w2v_MD_VAE", "model.yaml")) as f:
        text = f.read()
    # only the encoder's keys: the mapping resolves without building any module
    start = text.index("wav2vec2_size:")
    stop = text.index("wav2vec2_precision:")
    cfg = load_hyperpyyaml(text[start:stop])
    assert cfg["wav2vec2_size"] == 1024 and resolve_config(cfg["wav2vec2_config"]) == LARGE_LV60


# --------------------------------------------------------------------------- the recipes' wiring
class Rec(torch.nn.Module):
    """A stand-in module: records what it is called with and returns `out(*args)`."""

    def __init__(self, log, name, out):
        super().__init__()
        self.log, self.name, self.out = log, name, out

    def forward(self, *args, **kwargs):
        self.log.append((self.name, args, kwargs))
        return self.out(*args, **kwargs)


def _wired(recipe, T, Tw, monkeypatch):
    """The recipe's _upstream + _pi_logits on the CPU over recording modules."""
    import importlib
    from brain.dataio import PaddedBatch
    from models.MD_VAE.model import Target
    SBModel = importlib.import_module(f"models.{recipe}.model").SBModel
    B, F, C, n_ph = 2, 6, 5, 3
    log = []
    tag = lambda v: (lambda x, *a, **k: torch.full(x.shape[:2] + (2,), float(v)))
    mods = {
        "wav2vec2": Rec(log, "wav2vec2", lambda wav: torch.ones(B, Tw, C)),
        "phn_recog_in_fc": Rec(log, "phn_recog_in_fc", tag(1)),
        "b_detector_in_fc": Rec(log, "b_detector_in_fc", tag(2)),
        "w2v_feat_fc": Rec(log, "w2v_feat_fc", tag(3)),
        "phoneme_recognizer": Rec(log, "phoneme_recognizer", lambda x, *a, **k: {
            "out": torch.zeros(B, T, n_ph + 2), "losses": {"phn_recog_bce_loss": torch.zeros(B, T)}}),
        "boundary_detector": Rec(log, "boundary_detector", lambda x, *a, **k: {
            "boundary_v": torch.zeros(B, T), "losses": {"boundary_bce_loss": torch.zeros(B, T)}}),
        "phn_recog_out_fc": Rec(log, "phn_recog_out_fc", tag(4)),
        "concat_fc": Rec(log, "concat_fc", lambda x: x),
        "rnn": Rec(log, "rnn", lambda x: (x, None)),
        "pi_fc": Rec(log, "pi_fc", lambda x: x[..., :2]),
    }

    def never(*a, **k):
        raise AssertionError("the w2v recipes never call the normaliser")

    m = SBModel(modules=mods, hparams={"metric_keys": [], "output_dir": "", "normalizer": never,
                                       "epoch_counter": types.SimpleNamespace(current=1)},
                run_opts={"device": "cpu"})
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    ones = torch.ones(B)
    feat = torch.arange(B * T * F, dtype=torch.float32).view(B, T, F)
    b.update({"id": ["a", "b"], "feat": (feat, ones), "wav": (torch.zeros(B, 320 * T), ones),
              "gt_cnncl_seq": (torch.zeros(B, 3, dtype=torch.long), ones),
              "fa_boundary_seq": (torch.zeros(B, T), ones)})
    monkeypatch.setattr(PaddedBatch, "to", lambda self, dev: self, raising=False)
    m.target = Target.VAE
    m.modules.eval()
    pred, batch, feats, lens, _ = m._upstream(b)
    m._pi_logits(pred, feats, m._phn_out_fc if not recipe.endswith("_sfl") else "phn_recog_out_fc")
    return m, log, feat, feats


@pytest.mark.parametrize("recipe", ["w2v_MD_VAE", "w2v_MD_VAE_sfl"])
@pytest.mark.parametrize("short", [0, 1, 2])
def test_forward_wiring(recipe, short, monkeypatch):
    T, C = 9, 5
    m, log, feat, feats = _wired(recipe, T, T - short, monkeypatch)
    calls = [name for name, _, _ in log]
    assert calls.count("wav2vec2") == 1  # once per batch, shared
    by = {name: args for name, args, _ in log}
    assert by["wav2vec2"][0].shape == (2, 320 * T)
    padded = by["phn_recog_in_fc"][0]
    assert padded.shape == (2, T, C) and bool((padded[:, :T - short] == 1).all())
    assert not padded[:, T - short:].any()  # zero frames up to feat's T
    assert by["b_detector_in_fc"][0] is padded and by["w2v_feat_fc"][0] is padded
    # each FC to its own consumer
    assert bool((by["phoneme_recognizer"][0] == 1).all()) and bool((by["boundary_detector"][0] == 2).all())
    cat = by["concat_fc"][0]
    assert bool((cat[..., :2] == 3).all()) and bool((cat[..., 2:] == 4).all())
    # the decoder's target: batch['feat'] as it is (the normaliser would have raised)
    assert torch.equal(feats, feat)
    assert "feat_fc" not in calls


@pytest.mark.parametrize("recipe", ["w2v_MD_VAE", "w2v_MD_VAE_sfl"])
@pytest.mark.parametrize("short", [3, -1])
def test_a_frame_difference_of_three_raises(recipe, short, monkeypatch):
    with pytest.raises(ValueError, match="shape_diff"):
        _wired(recipe, 9, 9 - short, monkeypatch)


def test_recipes_subclass_their_parents_and_refuse_data_parallel(tmp_path):
    from brain import Stage
    from models.MD_VAE.model import SBModel as MD_VAE
    from models.MD_VAE_sfl.model import SBModel as MD_VAE_sfl
    from models.w2v_MD_VAE.model import SBModel as A
    from models.w2v_MD_VAE_sfl.model import SBModel as B
    assert issubclass(A, MD_VAE) and issubclass(B, MD_VAE_sfl)
    assert A.compute_forward is MD_VAE.compute_forward and B.compute_forward is MD_VAE_sfl.compute_forward
    assert not A.dp_exact and not B.dp_exact and A._phn_out_fc == "phn_recog_out_fc"
    for cls in (A, B):
        m = cls(modules={}, hparams={"metric_keys": [], "output_dir": str(tmp_path)}, run_opts={"device": "cpu"})
        m.on_stage_start(Stage.TRAIN, 1)
        m.world_size = 2
        with pytest.raises(RuntimeError, match="single-process"):
            m.on_stage_start(Stage.TRAIN, 1)
