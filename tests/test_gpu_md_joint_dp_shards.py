"""The shard contract of the data-parallel step (tests/test_gpu_md_dp_shards.py) for the joint
MD-VAE recipes with the paired upstream recurrence: the fixture's global batch of three utterances
run at TRAIN as the shards [0:2] and [2:3] under the ops.shard context the step builds, with the
fixture's noise sliced per shard and ``pair_upstream`` on.  The SUM of the shards' loss shares
against the fixture's means at 1e-5, the summed gradients at 1e-4 relative-max, the same parameters
without gradient.  The pair draws nothing and its rows are independent, so the contract holds
without change."""
import numpy as np
import pytest
import torch

import test_gpu_md_vae as MD
import test_gpu_md_vae_joint as J
from gpu_utils import need_gpu
from test_gpu_md_dp_shards import MD_DIMS, SHARDS, check_grads, check_losses, run_shards

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("recipe", list(J.RECIPES))
def test_joint_shards_match_reference(recipe, tmp_path):
    need_gpu()
    from brain import Stage
    from utils.decode_utils import decoded_lists
    assert SHARDS == [(0, 2), (2, 3)]
    gold = J.load_gold(recipe)
    m, meta = J.make_model(recipe, gold, tmp_path, pair=True)
    assert m.dp_exact
    m.modules.train()
    m.on_stage_start(Stage.TRAIN, 1)
    shares, total, preds = run_shards(m, MD._batch(gold, meta), Stage.TRAIN, m.noise, MD_DIMS)
    check_losses(shares, total, gold, "TRAIN")
    check_grads(m, gold, "TRAIN", set(meta["none_grads"]["TRAIN"]))
    got = torch.cat([p["sampled_pi"] for p in preds]).cpu().numpy()
    assert np.array_equal(got, gold["TRAIN/sampled_pi"])
    if recipe == "MD_VAE_joint_ll":  # the forward's decode, shard by shard
        flvl = [s for p in preds for s in decoded_lists(*p["decoded_device"])[1]]
        assert np.array_equal(MD._pad(flvl, meta["T"]), gold["TRAIN/decoded_flvl"])
    m.on_stage_end(Stage.TRAIN, 0.0, 1)
