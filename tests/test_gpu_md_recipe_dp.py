"""MD_VAE_sfl and LSTM_FC end to end under data parallelism: ``python -m torch.distributed.run
--nproc-per-node 2 train.py ... --distributed_launch`` (gloo, both ranks on the one GPU), three
epochs at batch size 2 per rank on a synthetic corpus whose valid and test splits (5 utterances)
leave a remainder, so the last global batch gives rank 1 a filler row.  Then test.py on that
checkpoint twice -- two ranks at batch size 2, one process at batch size 4 (the same global
batches) -- must write the same test_metrics.txt and, for MD_VAE_sfl, the same saved MD results:
five ids, no ``__pad__``.  Only rank 0 writes.

Process start-up dominates these runs: each subprocess has its own timeout, and the test stops at
the first non-zero exit.  The recurrences' persistent workgroups of two ranks must be co-resident:
H = 16, at most 4 rows per launch, asserted against the device's compute units first."""
import glob
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import PKG
from gpu_utils import need_gpu

pytestmark = pytest.mark.gpu

SIZES = "md_labels: true, n_train: 8, n_valid: 5, n_test: 5, min_frames: 16, max_frames: 24"
RECIPES = {
    "MD_VAE_sfl": "n_epochs: 3, pi_mcmc_num: 2, phn_rnn_hidden_size: 16, boundary_rnn_hidden_size: 16, "
                  "rnn_hidden_size: 16, dec_rnn_hidden_size: 16",
    "LSTM_FC": "n_epochs: 3, lstm_hidden_size: 16, lstm_num_layers: 2, lr: 0.001",
}


def _run(script, recipe, out, batch, ds, ranks):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    ov = f"{{batch_size: {batch}, synthetic: {{{SIZES}}}, model: {{{RECIPES[recipe]}, dataset_name: {ds}}}}}"
    args = ["config/run.yaml", "--model_class", recipe, "--model_name", "dp_ci",
            "--model", f"!include:../models/{recipe}/model.yaml", "--output_dir", str(out),
            "--extra_overrides", ov]
    if ranks > 1:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks),
               "--master-addr", "127.0.0.1", "--master-port", str(port), script] + args + \
              ["--distributed_launch", "--distributed_backend", "gloo"]
    else:
        cmd = [script] + args
    r = subprocess.run([sys.executable] + cmd, cwd=PKG, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (script, ranks, r.stderr[-4000:])


@pytest.mark.parametrize("recipe", list(RECIPES))
def test_two_rank_recipe(tmp_path, recipe):
    need_gpu()
    from mlvae_hip._lib import device_cus, lib
    for fwd in (0, 1):
        assert 2 * lib().mlvae_lstm_launch_workgroups(4, 16, 0, fwd) <= device_cus()
    out = tmp_path / "out"
    _run("train.py", recipe, out, 2, tmp_path / "ds_train", 2)
    assert (out / "train_log.txt").is_file()
    ckpts = glob.glob(str(out / "checkpoints" / "CKPT+*"))
    assert len(ckpts) >= 1
    for ck in ckpts:  # one writer: a checkpoint directory is whole (its meta file is there)
        assert os.path.exists(os.path.join(ck, "CKPT.yaml")), os.listdir(ck)
    metrics = out / "test_output" / "test_metrics.txt"
    _run("test.py", recipe, out, 2, tmp_path / "ds_dp", 2)
    dp = metrics.read_text()
    metrics.unlink()
    _run("test.py", recipe, out, 4, tmp_path / "ds_one", 1)
    one = metrics.read_text()
    print(dp)
    assert dp == one
    if recipe == "MD_VAE_sfl":
        saved = [json.load(open(tmp_path / d / "saved_md_results" / "dp_ci.json")) for d in ("ds_dp", "ds_one")]
        assert saved[0] == saved[1]
        assert len(saved[0]) == 5 and "__pad__" not in saved[0]
        assert not (tmp_path / "ds_train" / "saved_md_results").exists()  # TRAIN / VALID save none
