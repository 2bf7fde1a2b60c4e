"""The w2v_MD_VAE and w2v_MD_VAE_sfl recipes (models/w2v_MD_VAE*) on the HIP path, with the tiny
wav2vec2 encoder of the fixtures on a tiny spoken synthetic corpus.

* one TRAIN step per target, then VALID: finite losses; the frozen encoder's tensors bit-identical
  after the steps; the normaliser never called;
* with injected noise, the VAE-target training step's mean losses equal the PARENT recipe's
  (MD_VAE / MD_VAE_sfl) fed phn_recog_in_fc / b_detector_in_fc / w2v_feat_fc outputs computed in
  plain torch from the same encoder features.  Bound 1e-4 relative: the two sides differ only by
  the fp32 rounding of the three FCs (torch's GEMM against the HIP one, ~1e-6 relative), carried
  through the recurrent stacks -- the bound the sibling recipe tests hold gradients to;
* an encoder checkpoint (state dict, and a local `source` directory) reproduces the forward bit
  for bit.
Reference ops: ref:src/models/w2v_MD_VAE/model.py:16-129, ref:src/models/w2v_MD_VAE_sfl/model.py:16-158."""
import importlib
import json
import types

import pytest
import torch

import w2v_ref as R
from gpu_utils import need_gpu, rel_err

pytestmark = pytest.mark.gpu

NPH, H, Z, NC, BS, W, K = 7, 32, 8, 3, 4, 128, 2
LOSS_KEYS = ["phn_recog_bce_loss", "boundary_bce_loss", "boundary_kld_loss", "pi_nll_loss", "vae_kld_loss",
             "recon_loss"]
SFL_KEYS = ["rif_loss", "entropy_loss", "baseline_loss"]
METRICS = ["plvl_md.ACC", "plvl_md.PRE", "plvl_md.REC", "plvl_md.F1", "boundary.f1", "boundary.r_value"]
RECIPES = ["w2v_MD_VAE", "w2v_MD_VAE_sfl"]


@pytest.fixture(scope="module")
def corpus():
    need_gpu()
    from brain.features import Fbank
    from utils.data_io import SyntheticSet
    cf = Fbank(deltas=True, sample_rate=16000, hop_length=20, n_fft=400, n_mels=40)
    return SyntheticSet(8, 120, 40, 60, 4242, md_labels=True, n_phonemes=NPH, waveforms=True, compute_features=cf)


def _encoder():
    from modules.wav2vec2 import Wav2Vec2
    m = Wav2Vec2(config=R.TINY, precision="bf16")
    m.load_state_dict(R.fill_state(R.TINY, 20))
    return m


def _modules(sfl):
    from modules.boundary_detector import BoundaryDetector
    from modules.decoder import Decoder
    from modules.fc_block import FCBlock
    from modules.h_vae import HierarchicalVAE
    from modules.lstm import LSTM
    from modules.phoneme_recognizer import PhonemeRecognizer
    torch.manual_seed(5)
    mods = {
        "wav2vec2": _encoder(),
        "w2v_feat_fc": FCBlock([W, 2 * H, H], end_activation=True),
        "phn_recog_in_fc": FCBlock([W, 2 * H, H], end_activation=True),
        "phoneme_recognizer": PhonemeRecognizer(H, H, 2, [H, H, H, NPH + 2], NPH),
        "phn_recog_out_fc": FCBlock([NPH + 2, H, H], end_activation=True),
        "b_detector_in_fc": FCBlock([W, 2 * H, H], end_activation=True),
        "boundary_detector": BoundaryDetector(H, H, 2, [H, H, H, 1]),
        "concat_fc": FCBlock([2 * H, H, H], end_activation=True),
        "rnn": LSTM(input_size=H, hidden_size=H, num_layers=2, batch_first=True, dropout=0.0),
        "pi_fc": FCBlock([H, H, H // 2, 2]),
        "encoder": HierarchicalVAE([H, H, H], Z, NC),
        "decoder": Decoder(Z, H, 2, 0.0, [2 * H, H, H, 120]),
    }
    if sfl:
        mods["baseline_fc"] = FCBlock([H, H, H, 1])
    return mods


def _never(*a, **k):
    raise AssertionError("the w2v recipes never call the normaliser")


def _hparams(tmp_path, sfl, normalizer):
    keys = LOSS_KEYS + (SFL_KEYS if sfl else []) + METRICS
    hp = dict(epoch_counter=types.SimpleNamespace(current=1), normalizer=normalizer, batch_size=BS,
              metric_keys=keys, max_key="plvl_md.F1", output_dir=str(tmp_path), dataset_name=str(tmp_path / "ds"),
              model_name="w2v_tiny", **{k[:-5] + "_weight": 0.5 for k in LOSS_KEYS + SFL_KEYS})
    if sfl:
        hp["pi_mcmc_num"] = K
    return hp


def _model(tmp_path, recipe):
    sfl = recipe.endswith("_sfl")
    SBModel = importlib.import_module(f"models.{recipe}.model").SBModel
    return SBModel(modules=_modules(sfl), hparams=_hparams(tmp_path, sfl, _never), run_opts={"device": "cuda:0"})


def _noise(B, T, sfl, seed=13):
    g = torch.Generator().manual_seed(seed)
    lead = (K, B, T) if sfl else (B, T)
    u = lambda *s: torch.rand(*s, generator=g).cuda()
    return {"boundary_u": u(10, B, T), "pi_u": u(*lead), "eps_v": torch.randn(*lead, Z, generator=g).cuda(),
            "eps_g": torch.randn(*lead, NC * Z, generator=g).cuda(),
            "expo": -torch.log(torch.rand(*lead, NC, generator=g).clamp_min(1e-6)).cuda()}


def _step(m, batch, stage):
    """(mean losses, total, predictions) of one forward + objectives."""
    means = {}
    orig = m.compute_and_save_losses
    m.compute_and_save_losses = lambda losses: (means.update(losses), orig(losses))[1]
    try:
        pred = m.compute_forward(batch, stage)
        total = m.compute_objectives(pred, batch, stage)
    finally:
        del m.compute_and_save_losses
    return means, total, pred


@pytest.mark.parametrize("recipe", RECIPES)
def test_a_train_step_per_target_then_valid(tmp_path, corpus, recipe):
    from brain import Stage
    from mlvae_hip.optim import Adam
    from models.MD_VAE.model import TRAIN_TARGETS
    m = _model(tmp_path, recipe)
    enc = m.modules["wav2vec2"]
    assert list(enc.parameters()) == []  # frozen: nothing for an optimizer
    before = {k: v.clone() for k, v in enc.state_dict().items()}
    assert len(before) == len(R.state_shapes(R.TINY))
    opt = Adam([p for n, mod in m.modules.items() if n != "wav2vec2" for p in mod.parameters()], lr=1e-3)
    batch = next(iter(corpus.batches(batch_size=BS)))
    T = batch["feat"][0].shape[1]
    assert T - enc.n_frames(batch["wav"][0].shape[1]) in (1, 2)  # the padding is exercised
    for epoch, target in enumerate(TRAIN_TARGETS, start=1):
        m.on_stage_start(Stage.TRAIN, epoch)
        assert m.target == target
        m.modules.train()
        torch.manual_seed(epoch)
        means, total, pred = _step(m, batch, Stage.TRAIN)
        print(f"{recipe} {target.name}: total {total.item():.5f} " + " ".join(f"{k} {v.item():.5f}" for k, v in means.items()))
        assert torch.isfinite(total) and all(torch.isfinite(v) for v in means.values())
        assert m._w2v_feats.shape == (BS, T, W) and bool((m._w2v_feats[:, -1] == 0).all())
        total.backward()
        assert m.check_gradients(total)
        opt.step()
        opt.zero_grad()
        m.on_stage_end(Stage.TRAIN, total.item(), epoch)
    want = set(LOSS_KEYS + (SFL_KEYS if recipe.endswith("_sfl") else []))
    assert set(means) == want  # the VAE target's step carries every loss
    m.on_stage_start(Stage.VALID, 3)
    m.modules.eval()
    with torch.no_grad():
        means, total, pred = _step(m, batch, Stage.VALID)
    m._raise_device_errors()
    assert torch.isfinite(total) and set(means) == want and all(torch.isfinite(v) for v in means.values())
    assert "F1" in m.stats_loggers["plvl_md_stats"].summarize()
    after = enc.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


class _Fed(torch.nn.Module):
    """`inner` on a fixed input instead of the frames it is called with."""

    def __init__(self, inner, fed):
        super().__init__()
        self.inner, self.fed = inner, fed

    def forward(self, x, *args, **kwargs):
        return self.inner(self.fed, *args, **kwargs)


class _Const(torch.nn.Module):
    def __init__(self, value):
        super().__init__()
        self.value = value

    def forward(self, x):
        return self.value


@pytest.mark.parametrize("recipe", RECIPES)
def test_losses_equal_the_parent_recipe_fed_the_fc_outputs(tmp_path, corpus, recipe):
    from brain import Stage
    from models.MD_VAE.model import Target
    from models.w2v_MD_VAE.model import pad_to_frames
    sfl = recipe.endswith("_sfl")
    m = _model(tmp_path, recipe)
    batch = next(iter(corpus.batches(batch_size=BS)))
    B, T = batch["feat"][0].shape[:2]
    m.noise = _noise(B, T, sfl)
    m.modules.train()
    m.target = Target.VAE
    m.stats_loggers = {}
    got, got_total, pred = _step(m, batch, Stage.TRAIN)
    m._raise_device_errors()

    # the parent recipe on the same modules, its three inputs computed in plain torch
    mods = dict(m.modules.items())
    with torch.no_grad():
        w2v = pad_to_frames(mods["wav2vec2"](batch["wav"][0].cuda()), T)
        assert torch.equal(w2v, m._w2v_feats)  # the encoder is deterministic
        fc = lambda name: mods[name].blocks(w2v)
        parent_mods = {k: v for k, v in mods.items()
                       if k not in ("wav2vec2", "w2v_feat_fc", "phn_recog_in_fc", "b_detector_in_fc")}
        parent_mods["feat_fc"] = _Const(fc("w2v_feat_fc"))
        parent_mods["phoneme_recognizer"] = _Fed(mods["phoneme_recognizer"], fc("phn_recog_in_fc"))
        parent_mods["boundary_detector"] = _Fed(mods["boundary_detector"], fc("b_detector_in_fc"))
    if not sfl:
        parent_mods["phn_recog_fc"] = parent_mods.pop("phn_recog_out_fc")
    Parent = importlib.import_module(f"models.{recipe[4:]}.model").SBModel
    identity = lambda feats, lens, epoch=None: feats  # the decoder's target is the raw feat on both sides
    p = Parent(modules=parent_mods, hparams=_hparams(tmp_path, sfl, identity), run_opts={"device": "cuda:0"})
    p.noise = m.noise
    p.modules.train()
    p.target = Target.VAE
    p.stats_loggers = {}
    want, want_total, ppred = _step(p, batch, Stage.TRAIN)
    p._raise_device_errors()
    assert set(got) == set(want) == set(LOSS_KEYS + (SFL_KEYS if sfl else []))
    for k in want:
        e = rel_err(got[k], want[k])
        print(f"{recipe} {k}: {got[k].item():.7f} parent {want[k].item():.7f} rel {e:.2e}")
        assert e < 1e-4, k
    assert rel_err(got_total, want_total) < 1e-4
    assert torch.equal(pred["sampled_pi"], ppred["sampled_pi"])
    # each FC reaches its own consumer: swapping two of them changes the losses
    m.modules["phn_recog_in_fc"], m.modules["b_detector_in_fc"] = mods["b_detector_in_fc"], mods["phn_recog_in_fc"]
    _, _, other = _step(m, batch, Stage.TRAIN)
    m._raise_device_errors()
    for key in ("phn_recog_out", "boundary_v"):
        matched, swapped = rel_err(pred[key], ppred[key]), rel_err(other[key], ppred[key])
        print(f"{recipe} {key}: against the parent rel {matched:.2e}, with the two FCs swapped {swapped:.2e}")
        assert swapped > 10 * matched and swapped > 1e-6, key  # untrained networks: the margin is self-calibrated


def test_pad_to_frames():
    need_gpu()
    from models.w2v_MD_VAE.model import pad_to_frames
    x = torch.ones(2, 10, 4, device="cuda")
    assert pad_to_frames(x, 10) is x
    for d in (1, 2):
        y = pad_to_frames(x, 10 + d)
        assert y.shape == (2, 10 + d, 4) and torch.equal(y[:, :10], x) and not y[:, 10:].any()
    for T in (13, 9):
        with pytest.raises(ValueError, match="shape_diff"):
            pad_to_frames(x, T)


def test_encoder_checkpoint_reproduces_the_forward(tmp_path):
    need_gpu()
    from modules.wav2vec2 import Wav2Vec2
    wav = R.ragged_wav(3).cuda()
    a = _encoder().cuda()
    out = a(wav)
    torch.save(a.state_dict(), tmp_path / "pytorch_model.bin")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(R.TINY, f)
    torch.manual_seed(99)
    b = Wav2Vec2(config=R.TINY).cuda()  # other random weights ...
    assert not torch.equal(b(wav), out)
    b.load_state_dict(torch.load(tmp_path / "pytorch_model.bin", weights_only=True))  # ... until the load
    assert torch.equal(b(wav), out)
    c = Wav2Vec2(source=str(tmp_path)).cuda()  # a local directory
    assert torch.equal(c(wav), out)
