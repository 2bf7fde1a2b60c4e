"""The Kaldi-compatible front end's HIP kernels (csrc/kaldi_fbank.hip through
mlvae_hip.ops.kaldi_fbank / cmvn_accumulate / cmvn_apply and brain.features.KaldiFbank /
SpeakerCMVN) against the float64 helper tests/kaldi_fbank_ref.py.

Tolerance: the yardstick is the same helper run in float32 on the same input (same float64-built
tables rounded to fp32, every product and sum in fp32); its worst absolute error against float64
is computed here, and the device's worst error must be at most 4 x that, separately for statics,
deltas and delta-deltas (4, as tests/test_gpu_fbank.py: a different summation order over the
window-long sums, and the device's log).  Frames per tile of the kernel: 32."""
import numpy as np
import pytest
import torch

import kaldi_fbank_ref as R
from conftest import PKG
from gpu_utils import need_gpu
from test_gpu_fbank import spoken_like

pytestmark = pytest.mark.gpu

FT = 32  # csrc/kaldi_fbank.hip
REF_GEO = dict(sample_rate=16000, hop_ms=20, win_ms=25, n_mels=40)
# T_b = 0, then 1 .. 5 (the delta-delta edges; 160 and 260 samples are shorter than the window and
# reflect more than once), one frame below, at and above a tile of 32 frames, and three tiles
PARITY_N = [0, 159, 160, 100 + 160, 479, 480, 4 * 320 + 7, 31 * 320 - 161, 31 * 320 - 160, 32 * 320 + 1,
            66 * 320 + 5, 3 * 320, 5 * 320 - 3]
PARITY_T = [0, 0, 1, 1, 1, 2, 4, 30, 31, 32, 66, 3, 5]
BLOCKS = ("static", "delta", "delta-delta")


def _ops_kw(geo):
    return dict(sample_rate=geo["sample_rate"], hop_length=geo["hop_ms"], win_length=geo["win_ms"],
                n_mels=geo["n_mels"])


def device_fbank(wav, n_samples, geo):
    from mlvae_hip import ops
    feats, frames = ops.kaldi_fbank(torch.from_numpy(wav).cuda(), torch.tensor(n_samples, dtype=torch.int32),
                                    **_ops_kw(geo))
    torch.cuda.synchronize()
    return feats.cpu().numpy(), frames.cpu().numpy()


def _block_errors(got, ref32, ref64, M, what, unit=""):
    for name, sl in zip(BLOCKS, (slice(0, M), slice(M, 2 * M), slice(2 * M, 3 * M))):
        e32 = np.abs(ref32[..., sl].astype(np.float64) - ref64[..., sl]).max()
        edev = np.abs(got[..., sl].astype(np.float64) - ref64[..., sl]).max()
        print(f"{what} {name}: device {edev:.3e}{unit}, float32 helper {e32:.3e}{unit}, ratio {edev / e32:.2f}")
        assert edev <= 4 * e32, (what, name, edev, e32)


def check_against_helper(wav, n_samples, geo, what):
    """Device vs float64 under the float32 yardstick; returns (device feats, float64 feats, frames)."""
    ref64, frames64 = R.kaldi_fbank_batch(wav.astype(np.float64), n_samples, dtype=np.float64, **geo)
    ref32, _ = R.kaldi_fbank_batch(wav, n_samples, dtype=np.float32, **geo)
    got, frames = device_fbank(wav, n_samples, geo)
    assert got.shape == ref64.shape and got.dtype == np.float32
    assert np.array_equal(frames, frames64)
    assert np.isfinite(got).all()
    for b, T in enumerate(frames64):
        assert not got[b, T:].any(), f"{what}: utterance {b} has non-zero rows past its {T} frames"
    _block_errors(got, ref32, ref64, geo["n_mels"], what)
    return got, ref64, frames64


@pytest.fixture(scope="module")
def parity_batch():
    return spoken_like(PARITY_N, 16000, seed=3)


def test_parity_with_the_float64_helper(parity_batch):
    need_gpu()
    assert np.isnan(parity_batch[0]).all() and np.isnan(parity_batch[3, 260:]).all()  # NaN past each length
    _, _, frames = check_against_helper(parity_batch, PARITY_N, REF_GEO, "parity")
    assert list(frames) == PARITY_T


@pytest.mark.parametrize("geo", [
    dict(sample_rate=8000, hop_ms=10, win_ms=25, n_mels=23),    # L 200, P 256
    dict(sample_rate=16000, hop_ms=10, win_ms=25, n_mels=64),   # the mel limit, a 160-sample shift
], ids=["8k-10ms-23", "16k-10ms-64"])
def test_other_geometries(geo):
    need_gpu()
    hop, L, _ = R.geometry(geo["sample_rate"], geo["hop_ms"], geo["win_ms"])
    ns = [0, hop // 2 - 1, hop // 2, L // 2 + 3, 3 * hop + 1, (FT - 1) * hop + hop // 2, FT * hop + 3,
          (2 * FT + 1) * hop + 7]
    check_against_helper(spoken_like(ns, geo["sample_rate"], seed=4), ns, geo, "geometry")


def test_independent_of_the_batch_and_deterministic(parity_batch):
    need_gpu()
    got, frames = device_fbank(parity_batch, PARITY_N, REF_GEO)
    again, _ = device_fbank(parity_batch, PARITY_N, REF_GEO)
    assert np.array_equal(got, again)
    for b, N in enumerate(PARITY_N):
        alone, f1 = device_fbank(parity_batch[b:b + 1, :max(N, 1)], [N], REF_GEO)
        assert f1[0] == frames[b] and alone.shape[1] == frames[b]
        assert np.array_equal(alone[0], got[b, :frames[b]]), f"utterance {b} differs alone and in the batch"
        assert not got[b, frames[b]:].any()


# --------------------------------------------------------------------------- CMVN
CMVN_N = [[9 * 320, 4 * 320 + 7, 7 * 320, 160], [12 * 320, 3 * 320, 320, 35 * 320]]
CMVN_SPK = [[0, 1, 0, 1], [2, 0, 2, 1]]  # speaker 2 appears in the second batch only


@pytest.fixture(scope="module")
def cmvn_case():
    """Two batches of four utterances, three speakers: (device raw feats, float64 raw, float32 raw,
    frames) per batch.  The device's own raw features feed both CMVNs, so the CMVN kernels are
    measured alone; the float32 / float64 helpers run on those same float32 numbers."""
    need_gpu()
    out = []
    for i, ns in enumerate(CMVN_N):
        wav = spoken_like(ns, 16000, seed=20 + i)
        got, frames = device_fbank(wav, ns, REF_GEO)
        out.append((got, frames))
    return out


def test_cmvn_against_the_helper(cmvn_case):
    need_gpu()
    from mlvae_hip import ops
    D, S = 120, 3
    stats = torch.zeros(S, 2 * D + 1, device="cuda", dtype=torch.float64)
    want = np.zeros((S, 2 * D + 1))
    dev = []
    for (raw, frames), spk in zip(cmvn_case, CMVN_SPK):
        x = torch.from_numpy(raw).cuda()
        ops.cmvn_accumulate(stats, x, torch.from_numpy(frames), spk)
        R.cmvn_accumulate(want, raw, frames, spk)
        dev.append(x)
    got_stats = stats.cpu().numpy()
    assert list(want[:, 2 * D]) == [9 + 7 + 3, 4 + 1 + 35, 12 + 1]
    rel = np.abs(got_stats - want) / np.abs(want)
    print(f"statistics: worst relative difference to the float64 sums {rel.max():.2e}")
    assert rel.max() <= 1e-12
    for (raw, frames), spk, x in zip(cmvn_case, CMVN_SPK, dev):
        y = ops.cmvn_apply(x, torch.from_numpy(frames), spk, stats)
        assert y is x
        got = y.cpu().numpy()
        ref64 = R.cmvn_apply(raw.astype(np.float64), frames, spk, want, dtype=np.float64)
        ref32 = R.cmvn_apply(raw, frames, spk, want, dtype=np.float32)
        assert np.isfinite(got).all()
        for b, T in enumerate(frames):
            assert not got[b, T:].any() and not raw[b, T:].any()
        _block_errors(got, ref32, ref64, 40, "cmvn", " sd")
    # per speaker: mean 0 and variance 1 over both batches
    rows = {s: [] for s in range(S)}
    for (raw, frames), spk, x in zip(cmvn_case, CMVN_SPK, dev):
        for b, T in enumerate(frames):
            rows[spk[b]].append(x[b, :T].double().cpu().numpy())
    for s in range(S):
        r = np.concatenate(rows[s])
        assert np.abs(r.mean(0)).max() < 1e-5 and np.abs(r.var(0) - 1).max() < 1e-4, s


def test_cmvn_rerun_is_bit_identical_and_module(cmvn_case):
    need_gpu()
    from brain.features import SpeakerCMVN
    runs = []
    for _ in range(2):
        c = SpeakerCMVN(3, 120)
        for (raw, frames), spk in zip(cmvn_case, CMVN_SPK):
            c.accumulate(torch.from_numpy(raw).cuda(), frames, spk)
        raw, frames = cmvn_case[1]
        y = c.apply(torch.from_numpy(raw).cuda(), frames, CMVN_SPK[1])
        runs.append((c.stats.clone(), y))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    c.reset()
    assert not c.stats.any()


def test_cmvn_reports_a_bad_speaker_id(cmvn_case):
    need_gpu()
    from mlvae_hip import ops
    raw, frames = cmvn_case[0]
    x = torch.from_numpy(raw).cuda()
    stats = torch.zeros(3, 241, device="cuda", dtype=torch.float64)
    for bad in ([0, 1, 3, 1], [0, -1, 0, 1]):
        with pytest.raises(ValueError, match="speaker id"):
            ops.cmvn_accumulate(stats, x, torch.from_numpy(frames), bad)
    ops.cmvn_accumulate(stats, x, torch.from_numpy(frames), [0, 1, 0, 1])
    with pytest.raises(ValueError, match="speaker id"):
        ops.cmvn_apply(x.clone(), torch.from_numpy(frames), [0, 1, 3, 1], stats)
    with pytest.raises(ValueError, match="no accumulated statistics"):
        ops.cmvn_apply(x.clone(), torch.from_numpy(frames), [0, 1, 2, 1], stats)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- limits
def test_status_errors():
    need_gpu()
    from mlvae_hip import _lib, ops
    from brain.features import KaldiFbank
    l = _lib.lib()
    wav = torch.zeros(1, 640, device="cuda")
    ns = torch.tensor([640], dtype=torch.int32, device="cuda")
    out = torch.zeros(1, 2, 120, device="cuda")
    frames = torch.zeros(1, dtype=torch.int32, device="cuda")
    buf = torch.zeros(1 << 18, device="cuda")  # stands in for table and workspace: never launched
    s = torch.cuda.current_stream().cuda_stream
    for B, hop, L, P, n_mels, word in ((1, 320, 400, 384, 40, "power of two"), (1, 320, 400, 1024, 40, "512"),
                                       (1, 320, 400, 256, 40, "window"), (1, 320, 400, 512, 65, "n_mels"),
                                       (1, 0, 400, 512, 40, "hop"), (65536, 320, 400, 512, 40, "65535")):
        rc = l.mlvae_kaldi_fbank(B, 640, wav.data_ptr(), 640, ns.data_ptr(), hop, L, P, n_mels, 1,
                                 buf.data_ptr(), out.data_ptr(), 120, frames.data_ptr(), buf.data_ptr(),
                                 buf.numel() * 4, s)
        assert rc == 1 and word in _lib.last_error(), (hop, L, P, n_mels, _lib.last_error())
    st = torch.zeros(3, 241, device="cuda", dtype=torch.float64)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    spk = torch.zeros(1, dtype=torch.int32, device="cuda")
    for fn in (l.mlvae_cmvn_accumulate, l.mlvae_cmvn_apply):
        for B, D, S, ld, word in ((65536, 120, 3, 120, "65535"), (1, 1025, 3, 1025, "1024"),
                                  (1, 120, 0, 120, "S"), (1, 120, 3, 119, "ld")):
            rc = fn(B, 2, D, S, out.data_ptr(), ld, frames.data_ptr(), spk.data_ptr(), st.data_ptr(),
                    err.data_ptr(), s)
            assert rc == 1 and word in _lib.last_error(), (B, D, S, ld, _lib.last_error())
    assert int(err.item()) == 0 and not st.any()
    with pytest.raises(_lib.MlvaeError, match="512"):
        KaldiFbank(n_fft=600)(wav)
    with pytest.raises(_lib.MlvaeError, match="n_mels"):
        KaldiFbank(n_mels=65)(wav)
    with pytest.raises(RuntimeError, match="backward"):
        ops.kaldi_fbank(wav.clone().requires_grad_(True))
    torch.cuda.synchronize()


def test_module_on_the_device(parity_batch):
    need_gpu()
    from brain.features import KaldiFbank
    wav = torch.from_numpy(np.nan_to_num(parity_batch[-3:, :4000])).cuda()
    full = KaldiFbank()
    a = full(wav)
    b = full(wav, torch.ones(3))
    assert a.shape == (3, (4000 + 160) // 320, 120) and torch.equal(a, b)
    st = KaldiFbank(deltas=False)(wav)
    assert st.shape == (3, 13, 40) and torch.equal(st, a[..., :40])
    # relative lengths: N_b = round(N len_b), the rows past (N_b + 160) // 320 are zeros
    c = full(wav, torch.tensor([1.0, 0.5, 0.25]))
    assert torch.equal(c[0], a[0]) and not c[1, 6:].any() and not c[2, 3:].any()
    want, _ = R.kaldi_fbank_batch(wav.cpu().numpy().astype(np.float64), [4000, 2000, 1000], **REF_GEO)
    assert np.abs(c.cpu().numpy() - want).max() < 1e-3


# --------------------------------------------------------------------------- the recipe
def _one_epoch(out_dir, kaldi):
    """One epoch of MD_VAE_sfl at tests/test_gpu_md_vae_sfl.py's tiny sizes on the spoken corpus
    through the recipe path: (the first batch's phn_recog_out, the batch losses, the normaliser)."""
    from prepare_experiment import prepare_experiment
    overrides = ("{synthetic: {md_labels: true, waveforms: true, kaldi_feats: true, n_train: 16, n_valid: 8, "
                 "n_test: 8, min_frames: 40, max_frames: 60}, model: {n_epochs: 1, pi_mcmc_num: 2, "
                 "phn_rnn_hidden_size: 64, boundary_rnn_hidden_size: 64, rnn_hidden_size: 64, "
                 "dec_rnn_hidden_size: 64, dataset_name: %s%s}}" % (out_dir / "ds", ", use_kaldi_feat: true"
                                                                    if kaldi else ""))
    args = ["config/run.yaml", "--model_class", "MD_VAE_sfl", "--model_name", "kaldi_ci",
            "--model", "!include:../models/MD_VAE_sfl/model.yaml", "--output_dir", str(out_dir),
            "--extra_overrides", overrides]
    prepared = prepare_experiment(args, prepare_exp_dir=True)
    hp, model = prepared["hparams"], prepared["model"]
    train_set, valid_set, _ = prepared["datasets"]
    e = train_set.items[0]
    assert e["kaldi_feat"].shape == e["feat"].shape and 0 <= e["spk"] < 4
    first, losses = [], []
    forward, fit_batch = model.compute_forward, model.fit_batch

    def spy_forward(batch, stage):
        pred = forward(batch, stage)
        if not first:
            first.append(pred["phn_recog_out"].detach().clone())
        return pred

    def spy_fit(batch):
        loss = fit_batch(batch)
        losses.append(loss.detach())
        return loss

    model.compute_forward, model.fit_batch = spy_forward, spy_fit
    model.fit(hp["model"]["epoch_counter"], train_set, valid_set,
              train_loader_kwargs=hp["train_dataloader_opts"], valid_loader_kwargs=hp["valid_dataloader_opts"])
    return first[0], torch.stack(losses), hp["model"]["normalizer"]


def test_md_vae_sfl_trains_on_kaldi_feat(tmp_path, monkeypatch):
    need_gpu()
    monkeypatch.chdir(PKG)  # the recipe's relative paths, as `python train.py` from the package
    out_k, loss_k, norm_k = _one_epoch(tmp_path / "kaldi", True)
    out_f, loss_f, norm_f = _one_epoch(tmp_path / "feat", False)
    assert loss_k.numel() == 2 and bool(torch.isfinite(loss_k).all()) and bool(torch.isfinite(loss_f).all())
    assert norm_k.glob_mean.numel() == 0   # the normaliser never ran
    assert norm_f.glob_mean.numel() == 120
    assert out_k.shape == out_f.shape and not torch.equal(out_k, out_f)
    print(f"first batch phn_recog_out: max |kaldi_feat run - feat run| {float((out_k - out_f).abs().max()):.3e}")
