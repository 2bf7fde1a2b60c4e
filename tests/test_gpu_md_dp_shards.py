"""The shard contract of the MD recipes' data-parallel step, in one process: the global batch of a
reference fixture (md_vae_tiny, md_vae_sfl_tiny, lstm_fc_tiny; three utterances) run as the shards
[0:2] and [2:3], one after the other, each under the ops.shard context the step builds from the
loader's fields.

* Injected noise (the fixture's, sliced per shard): the SUM of the shards' loss shares against the
  fixture's means at 1e-5, the summed gradients against the fixture's at 1e-4 relative-max, the
  same parameters without gradient, the decoded sequences exact -- the bounds
  tests/test_gpu_md_vae.py holds the whole batch to.
* Library noise (nothing injected, dropout 0.15 in ``rnn`` and the decoder): the summed shard
  gradients against ONE whole-batch call of the unchanged single-process path under the same
  torch seed, 1e-4 relative-max.  A stream left unmapped would draw other noise for utterance 2
  and shows as an order-one mismatch."""
import numpy as np
import pytest
import torch

import test_gpu_lstm_fc as FC
import test_gpu_md_vae as MD
import test_gpu_md_vae_sfl as SFL
from gpu_utils import need_gpu, rel_err

pytestmark = pytest.mark.gpu

SHARDS = [(0, 2), (2, 3)]


def _load(mod):
    d = np.load(mod.GOLD)
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def gold_md():
    return _load(MD)


@pytest.fixture(scope="module")
def gold_sfl():
    return _load(SFL)


@pytest.fixture(scope="module")
def gold_fc():
    return _load(FC)


def shard_batch(batch, lo, hi):
    """Rows [lo:hi) of a whole batch with the fields utils.data_io's loader attaches under
    world > 1 (same padded lengths: the relative lengths stay the global batch's)."""
    from brain.dataio import PaddedBatch
    b = PaddedBatch.__new__(PaddedBatch)
    dict.__init__(b)
    for k, v in batch.items():
        b[k] = (v[0][lo:hi].contiguous(), v[1][lo:hi].contiguous()) if isinstance(v, tuple) else v[lo:hi]
    b.global_lens = {k: v[1].clone() for k, v in batch.items() if isinstance(v, tuple)}
    b.utt_offset, b.global_size, b.global_index = lo, len(batch["id"]), 0
    return b


def shard_noise(noise, lo, hi, batch_dim):
    return {k: v.narrow(batch_dim[k], lo, hi - lo).contiguous() for k, v in (noise or {}).items()}


MD_DIMS = {"boundary_u": 1, "pi_u": 0, "eps_v": 0, "eps_g": 0, "expo": 0}
SFL_DIMS = {"boundary_u": 1, "pi_u": 1, "eps_v": 1, "eps_g": 1, "expo": 1}


def run_shards(m, batch, stage, noise, dims):
    """Forward + objectives (+ backward in train) of every shard under its context: (the summed
    loss shares per key, the summed total, the per-shard predictions).  Gradients accumulate in
    .grad: their sum."""
    shares, total, preds = {}, 0.0, []
    orig = m.compute_and_save_losses

    def keep(losses):
        for k, v in losses.items():
            shares[k] = shares.get(k, 0.0) + float(v.detach().double())
        return orig(losses)

    m.compute_and_save_losses = keep
    try:
        for lo, hi in SHARDS:
            b = shard_batch(batch, lo, hi)
            m.noise = shard_noise(noise, lo, hi, dims) if noise is not None else None
            with m._dp_shard(b, stage):
                pred = m.compute_forward(b, stage)
                loss = m.compute_objectives(pred, b, stage)
                if loss.requires_grad:
                    loss.backward()
            total += float(loss.detach().double())
            preds.append(pred)
    finally:
        del m.compute_and_save_losses
    return shares, total, preds


def check_losses(shares, total, gold, name):
    want = {k[len(name) + 6:]: v for k, v in gold.items() if k.startswith(name + "/loss/")}
    assert set(shares) == set(want)
    for k, v in want.items():
        e = abs(shares[k] - float(v)) / max(abs(float(v)), 1e-30)
        print(f"{name} {k}: shares sum {shares[k]:.7f} ref {float(v):.7f} rel {e:.2e}")
        assert e < 1e-5, k
    e = abs(total - float(gold[name + "/total"])) / abs(float(gold[name + "/total"]))
    print(f"{name} total rel {e:.2e}")
    assert e < 1e-5


def check_grads(m, gold, name, none):
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        if n in none:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        e = rel_err(p.grad, torch.from_numpy(gold[f"{name}/grad/{n}"]))
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (n, e)
    print(f"{name}: worst summed shard gradient {worst[0]} rel {worst[1]:.2e}")


def check_decoded(preds, gold, name, meta):
    from utils.decode_utils import decoded_lists
    bnd, flvl, plvl = [], [], []
    for p in preds:
        b, f, l = decoded_lists(*p["decoded_device"])
        bnd += b
        flvl += f
        plvl += l
    assert np.array_equal(MD._pad(bnd, meta["T"]), gold[name + "/decoded_boundary"])
    assert np.array_equal(MD._pad(flvl, meta["T"]), gold[name + "/decoded_flvl"])
    assert np.array_equal(MD._pad(plvl, meta["L"]), gold[name + "/decoded_plvl"])


# --------------------------------------------------------------------------- injected noise
@pytest.mark.parametrize("name", ["PHN_RECOG", "B_DETECTOR", "VAE"])
def test_md_vae_shards_match_reference(gold_md, tmp_path, name):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = MD._model(gold_md, tmp_path)
    m.modules.train()
    m.target = Target[name]
    m.stats_loggers = {}
    shares, total, preds = run_shards(m, MD._batch(gold_md, meta), Stage.TRAIN, m.noise, MD_DIMS)
    check_losses(shares, total, gold_md, name)
    check_grads(m, gold_md, name, set(meta["none_grads"][name]))
    if name == "VAE":
        check_decoded(preds, gold_md, name, meta)
        got = torch.cat([p["sampled_pi"] for p in preds]).cpu().numpy()
        assert np.array_equal(got, gold_md[name + "/sampled_pi"])
    m.on_stage_end(Stage.TRAIN, 0.0, 1)


def test_md_vae_test_target_shards(gold_md, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = MD._model(gold_md, tmp_path)
    m.modules.eval()
    m.on_stage_start(Stage.TEST, None)
    noise = m.noise
    with torch.no_grad():
        shares, total, preds = run_shards(m, MD._batch(gold_md, meta), Stage.TEST, noise, MD_DIMS)
    check_losses(shares, total, gold_md, "TEST")
    check_decoded(preds, gold_md, "TEST", meta)


def test_md_vae_sfl_shards_match_reference(gold_sfl, tmp_path):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = SFL._model(gold_sfl, tmp_path, train=True)
    m.modules.train()
    m.target = Target.VAE
    m.stats_loggers = {}
    shares, total, preds = run_shards(m, MD._batch(gold_sfl, meta), Stage.TRAIN, m.noise, SFL_DIMS)
    check_losses(shares, total, gold_sfl, "VAE")
    check_grads(m, gold_sfl, "VAE", set(meta["none_grads"]["VAE"]))
    check_decoded(preds, gold_sfl, "VAE", meta)
    draws = torch.cat([p["sampled_pi_draws"] for p in preds], dim=1).cpu()
    for k in range(meta["K"]):
        assert np.array_equal(draws[k, ..., 1].numpy(), gold_sfl["pi_labels"][k].astype(np.float32)), k
    m.on_stage_end(Stage.TRAIN, 0.0, 1)


def test_md_vae_sfl_test_target_shards(gold_sfl, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = SFL._model(gold_sfl, tmp_path, train=False)
    m.modules.eval()
    m.on_stage_start(Stage.TEST, None)
    with torch.no_grad():
        shares, total, preds = run_shards(m, MD._batch(gold_sfl, meta), Stage.TEST, m.noise, SFL_DIMS)
    check_losses(shares, total, gold_sfl, "TEST")
    check_decoded(preds, gold_sfl, "TEST", meta)


def test_lstm_fc_test_shards(gold_fc, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = FC._model(gold_fc, tmp_path)
    m.modules.eval()
    m.on_stage_start(Stage.TEST, None)
    with torch.no_grad():
        _, total, preds = run_shards(m, FC._batch(gold_fc, meta, aug=False), Stage.TEST, None, None)
    ref = float(gold_fc["TEST/loss"])
    assert abs(total - ref) / abs(ref) < 1e-5
    got = torch.cat([p["flvl_pred_md_lbl_seq"] for p in preds]).cpu().numpy()
    assert np.array_equal(got, gold_fc["TEST/pred_md_lbl_seqs"])


def test_lstm_fc_shards_match_reference(gold_fc, tmp_path):
    need_gpu()
    from brain import Stage
    m, meta = FC._model(gold_fc, tmp_path)
    m.modules.train()
    m.on_stage_start(Stage.TRAIN, 1)
    _, total, preds = run_shards(m, FC._batch(gold_fc, meta, aug=True), Stage.TRAIN, None, None)
    ref = float(gold_fc["TRAIN/loss"])
    e = abs(total - ref) / abs(ref)
    print(f"LSTM_FC: loss shares sum {total:.7f} ref {ref:.7f} rel {e:.2e}")
    assert e < 1e-5
    check_grads(m, gold_fc, "TRAIN", set())
    got = torch.cat([p["flvl_pred_md_lbl_seq"] for p in preds]).cpu().numpy()
    assert np.array_equal(got, gold_fc["TRAIN/pred_md_lbl_seqs"])
    from mlvae_hip import ops
    ops.raise_flvl_err()  # the stage's label error bit: clear


# --------------------------------------------------------------------------- library noise
def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.modules.named_parameters()}


def _library_noise_case(m, batch, stage, seed):
    """(whole-batch gradients of the single-process path, summed shard gradients), both under
    torch seed `seed`, with no injected noise and dropout 0.15 in rnn and the decoder."""
    m.noise = None
    m.modules["rnn"].dropout = 0.15
    m.modules["decoder"].rnn.dropout = 0.15
    m.modules.train()
    m.stats_loggers = {}
    torch.manual_seed(seed)
    loss = m.compute_objectives(m.compute_forward(batch, stage), batch, stage)
    loss.backward()
    whole, whole_loss = _grads(m), float(loss.detach())
    m.modules.zero_grad(set_to_none=True)
    total = 0.0
    for lo, hi in SHARDS:
        b = shard_batch(batch, lo, hi)
        torch.manual_seed(seed)  # ranks are seeded alike and make the same calls in the same order
        with m._dp_shard(b, stage):
            loss = m.compute_objectives(m.compute_forward(b, stage), b, stage)
            loss.backward()
        total += float(loss.detach())
    return whole, whole_loss, _grads(m), total


def _compare(whole, whole_loss, got, total, what):
    e = abs(total - whole_loss) / abs(whole_loss)
    print(f"{what}: loss whole {whole_loss:.7f} shards {total:.7f} rel {e:.2e}")
    assert e < 1e-5
    worst = ("", 0.0)
    for n, g in whole.items():
        assert (g is None) == (got[n] is None), n
        if g is None:
            continue
        e = rel_err(got[n], g)
        if e > worst[1]:
            worst = (n, e)
        assert e < 1e-4, (what, n, e)
    print(f"{what}: worst summed shard gradient {worst[0]} rel {worst[1]:.2e}")


@pytest.mark.parametrize("name", ["B_DETECTOR", "VAE"])
def test_md_vae_library_noise_shards_match_whole_batch(gold_md, tmp_path, name):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = MD._model(gold_md, tmp_path)
    m.target = Target[name]
    _compare(*_library_noise_case(m, MD._batch(gold_md, meta), Stage.TRAIN, 4321), f"MD_VAE {name}")
    m.on_stage_end(Stage.TRAIN, 0.0, 1)


def test_md_vae_sfl_library_noise_shards_match_whole_batch(gold_sfl, tmp_path):
    need_gpu()
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = SFL._model(gold_sfl, tmp_path, train=True)
    m.target = Target.VAE
    _compare(*_library_noise_case(m, MD._batch(gold_sfl, meta), Stage.TRAIN, 4321), "MD_VAE_sfl VAE")
    m.on_stage_end(Stage.TRAIN, 0.0, 1)
