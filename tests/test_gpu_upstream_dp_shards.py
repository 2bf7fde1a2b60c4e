"""The shard contract of the upstream-module recipes' data-parallel step, in one process (as
test_gpu_md_dp_shards.py): the global batch of each tiny fixture (three utterances) run as the
shards [0:2] and [2:3], one after the other, each under the ops.shard context the step builds
from the loader's fields; the boundary detector's recorded draws are sliced per shard.

* The SUM of the shards' loss shares against the fixture's loss at 1e-5, the summed gradients
  against the fixture's at 1e-4 relative-max (the whole-batch bounds of
  test_gpu_upstream_recipes.py).
* The per-utterance counts concatenated over the shards equal the whole batch's, exactly, and the
  merged stats give the reference's recorded summary."""
import json

import pytest
import torch

import test_gpu_upstream_recipes as UP
from gpu_utils import need_gpu, rel_err
from test_gpu_md_dp_shards import SHARDS, shard_batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which", ["phn", "bnd"])
def test_shards_match_reference(which, tmp_path):
    need_gpu()
    from brain import Stage
    r = UP.RECIPES[which]
    gold = UP.load_gold(which)
    m, meta = UP.make_model(which, gold, tmp_path)
    m.modules.train()
    batch = UP.make_batch(gold, meta)
    noise = getattr(m, "noise", None)  # the boundary recipe's injected draws
    # the whole batch's counts, for the exact comparison
    m.on_stage_start(Stage.TRAIN, 1)
    with torch.no_grad():
        m.compute_objectives(m.compute_forward(batch, Stage.TRAIN), batch, Stage.TRAIN)
    whole = torch.cat([c for _, c, _ in m.stats_loggers[r["stats"]]._pending]).cpu()
    # the shards
    m.modules.zero_grad()
    m.on_stage_start(Stage.TRAIN, 1)
    total = 0.0
    for lo, hi in SHARDS:
        b = shard_batch(batch, lo, hi)
        if noise is not None:
            m.noise = {"boundary_u": noise["boundary_u"][:, lo:hi].contiguous()}
        with m._dp_shard(b, Stage.TRAIN):
            loss = m.compute_objectives(m.compute_forward(b, Stage.TRAIN), b, Stage.TRAIN)
            loss.backward()
        total += float(loss.detach().double())
    want = float(gold["TRAIN/loss"])
    e = abs(total - want) / abs(want)
    print(f"{which}: summed loss shares {total:.7f} ref {want:.7f} rel {e:.2e}")
    assert e < 1e-5
    worst = ("", 0.0)
    for n, p in m.modules.named_parameters():
        assert p.grad is not None, n
        g = rel_err(p.grad, torch.from_numpy(gold[f"TRAIN/grad/{n}"]))
        if g > worst[1]:
            worst = (n, g)
        assert g < 1e-4, (n, g)
    print(f"{which}: worst summed shard gradient {worst[0]} rel {worst[1]:.2e}")
    st = m.stats_loggers[r["stats"]]
    assert len(st._pending) == len(SHARDS) and st.scores_list == []
    assert torch.equal(torch.cat([c for _, c, _ in st._pending]).cpu(), whole)
    assert st.summarize() == json.loads(str(gold["TRAIN/summary_json"]))
    from mlvae_hip import ops
    ops.raise_score_err()  # no error bit
