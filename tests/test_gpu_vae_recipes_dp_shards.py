"""The shard contract of the single-encoder VAE recipes' data-parallel step, in one process (as
test_gpu_upstream_dp_shards.py): the global batch of each tiny fixture (three utterances) run as
the shards [0:2] and [2:3], one after the other, each under the ops.shard context the step builds
from the loader's fields, the fixture's draws sliced per shard, ``fused_latent`` off and on.

The SUM of the shards' loss shares against the fixture's loss and per-key losses at 1e-5, the
summed gradients against the fixture's at 1e-4 relative-max (the whole-batch bounds of
test_gpu_vae_recipes.py); pi_fc stays without gradient.  With library draws (nothing injected) the
fused shards choose the whole batch's components, row by row: an unmapped stream would draw
utterance 0's Gumbel noise for utterance 2."""
import pytest
import torch

import test_gpu_vae_recipes as VR
from gpu_utils import need_gpu, rel_err
from test_gpu_md_dp_shards import SHARDS, shard_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which,fused", VR.CASES)
def test_shards_match_reference(which, fused, tmp_path):
    need_gpu()
    from brain import Stage
    gold = VR.load_gold(which)
    m, meta = VR.make_model(which, gold, tmp_path, fused)
    m.modules.train()
    batch = VR.make_batch(gold, meta)
    noise = m.noise
    m.on_stage_start(Stage.TRAIN, 1)
    shares, total = {}, 0.0
    orig = m.compute_and_save_losses

    def keep(losses):
        for k, v in losses.items():
            shares[k] = shares.get(k, 0.0) + float(v.detach().double())
        return orig(losses)

    m.compute_and_save_losses = keep
    try:
        for lo, hi in SHARDS:
            b = shard_batch(batch, lo, hi)
            m.noise = {k: v[lo:hi].contiguous() for k, v in noise.items()}  # every draw is [B, ...]
            with m._dp_shard(b, Stage.TRAIN):
                loss = m.compute_objectives(m.compute_forward(b, Stage.TRAIN), b, Stage.TRAIN)
                loss.backward()
            total += float(loss.detach().double())
    finally:
        del m.compute_and_save_losses
    want = float(gold["TRAIN/loss"])
    e = abs(total - want) / abs(want)
    print(f"{which} fused={fused}: summed loss shares {total:.7f} ref {want:.7f} rel {e:.2e}")
    assert e < 1e-5
    assert set(shares) == set(VR.KEYS[which])
    for k, v in shares.items():
        ref = float(gold[f"TRAIN/loss/{k}"])
        assert abs(v - ref) / abs(ref) < 1e-5, (k, v, ref)
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        if n in meta["none_grads"]:
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        g = rel_err(p.grad, torch.from_numpy(gold[f"TRAIN/grad/{n}"]))
        if g > worst[1]:
            worst = (n, g)
        assert g < 1e-4, (n, g)
    print(f"{which} fused={fused}: worst summed shard gradient {worst[0]} rel {worst[1]:.2e}")


@pytest.mark.parametrize("which", ["gmm", "hvae"])
def test_library_draws_shards_are_the_whole_batch_s(which, tmp_path):
    need_gpu()
    from brain import Stage
    gold = VR.load_gold(which)
    m, meta = VR.make_model(which, gold, tmp_path, True)
    m.noise = None
    m.modules.train()
    batch = VR.make_batch(gold, meta)
    m.on_stage_start(Stage.TRAIN, 1)
    with torch.no_grad():
        torch.manual_seed(4321)
        whole = m.compute_forward(batch, Stage.TRAIN)["encoder_out"]["gmm_weight"]
        assert whole.argmax(-1).unique().numel() > 1
        for lo, hi in SHARDS:
            b = shard_batch(batch, lo, hi)
            torch.manual_seed(4321)  # ranks are seeded alike and make the same calls in the same order
            with m._dp_shard(b, Stage.TRAIN):
                got = m.compute_forward(b, Stage.TRAIN)["encoder_out"]["gmm_weight"]
            # the same component everywhere; its weight (1 - y) + y may round to the other side of 1
            # where the shard's GEMMs (another M) round the logits differently
            assert torch.equal(got.argmax(-1), whole[lo:hi].argmax(-1)), (lo, hi)
            assert float((got - whole[lo:hi]).abs().max()) < 1e-6, (lo, hi)
