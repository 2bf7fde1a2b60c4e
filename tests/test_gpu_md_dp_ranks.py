"""The MD-VAE recipe's shard-exact data-parallel step with two real ranks: two spawned workers,
gloo, one GPU (as tests/test_dist_gloo.py starts its workers), the weights of
tests/golden/md_vae_tiny.npz, library noise.

* Training: a global batch of four utterances (the fixture's three and utterance 0 under a second
  id), batch size 2 per rank.  Per target, after one fit_batch: the parameters are bit-identical
  on the two ranks, the reduced gradient equals the single-process gradient of the four
  utterances (this process, the unchanged single-process path, the same torch seed) at 1e-4
  relative-max -- test_gpu_md_vae.py's gradient bound -- with the same parameters left without
  one, and the step issued exactly ONE all_reduce (counted by wrapping
  torch.distributed.all_reduce; the fixture's normaliser is the identity and issues none).
  Rank 1 starts from other weights: init_optimizers' broadcast gives it rank 0's.
* Evaluation: the fixture's three utterances, so rank 1 holds one real row and one ``__pad__``
  filler; the merged plvl_md and boundary summaries equal the fixture's TEST summaries, and rank 0
  alone writes the saved MD results, three ids and no filler.

The recurrences are persistent kernels with co-resident workgroups: two ranks share the device, so
the test first asserts that twice a launch's workgroups fit the device's compute units."""
import functools
import json
import os
import queue

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import test_gpu_md_vae as MD
from gpu_utils import need_gpu, rel_err
from test_dist_gloo import _free_port

pytestmark = pytest.mark.gpu

TARGETS = ["PHN_RECOG", "B_DETECTOR", "VAE"]
SEED = 77
BS = 2  # per rank


def _gold():
    d = np.load(MD.GOLD)
    return {k: d[k] for k in d.files}


def _items(gold, meta, extra):
    """The fixture's utterances as the loader's per-utterance dicts (+ utterance 0 again under a
    second id when `extra`)."""
    T, L = meta["T"], meta["L"]
    items = []
    for i in list(range(meta["B"])) + ([0] if extra else []):
        Ti = int(round(float(gold["feat_lens"][i]) * T))
        Li = int(round(float(gold["seq_lens"][i]) * L))
        t = lambda k, n: torch.from_numpy(gold[k][i, :n].copy())
        items.append({"id": f"utt{i}" if len(items) < meta["B"] else f"utt{i}_again",
                      "feat": t("feat", Ti), "gt_cnncl_seq": t("gt_cnncl_seq", Li),
                      "fa_boundary_seq": t("fa_boundary_seq", Ti), "gt_boundary_seq": t("gt_boundary_seq", Ti),
                      "plvl_gt_md_lbl_seq": t("plvl_gt_md_lbl_seq", Li),
                      "prior": torch.from_numpy(gold["prior"][i].copy())})
    return items


def _first_batch(items, batch_size, rank, world, stage):
    from utils.data_io import BatchLoader
    return next(iter(BatchLoader(items, batch_size, rank, world, stage)))


def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().cpu().numpy().copy())
            for n, p in m.modules.named_parameters()}


def _worker(rank, world, port, q, tmp):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from brain import Stage
        from mlvae_hip.optim import Adam
        from models.MD_VAE.model import Target
        from pathlib import Path
        calls = {"n": 0}
        plain_all_reduce = dist.all_reduce

        def counted(*a, **k):
            calls["n"] += 1
            return plain_all_reduce(*a, **k)

        dist.all_reduce = counted
        gold = _gold()
        out = {"rank": rank}
        for name in TARGETS:
            m, meta = MD._model(gold, Path(tmp) / f"rank{rank}")
            m.rank, m.world_size = rank, world
            m.hparams.batch_size = BS
            m.noise = None
            if rank == 1:  # replicas start from rank 0's weights, whatever they held
                with torch.no_grad():
                    for p in m.modules.parameters():
                        p.add_(0.25)
            m.hparams.optimizer = functools.partial(Adam, lr=1e-3)
            m.init_optimizers()
            for n, p in m.modules.named_parameters():
                assert np.array_equal(p.detach().cpu().numpy(), gold["param/" + n]), n
            m.modules.train()
            m.target = Target[name]
            m.stats_loggers = {}
            batch = _first_batch(_items(gold, meta, True), BS, rank, world, Stage.TRAIN)
            seen = {}
            check = m.check_gradients

            def spy(loss, m=m, seen=seen, check=check):
                seen["grads"], seen["loss"] = _grads(m), float(loss)  # reduced, before the clip
                return check(loss)

            m.check_gradients = spy
            torch.manual_seed(SEED)
            calls["n"] = 0
            m.fit_batch(batch)
            torch.cuda.synchronize()
            out[name] = {"all_reduces": calls["n"], "grads": seen["grads"], "loss": seen["loss"],
                         "params": {n: p.detach().cpu().numpy().copy()
                                    for n, p in m.modules.named_parameters()}}
            m._raise_device_errors()
        # evaluation: three utterances over two ranks of two rows
        m, meta = MD._model(gold, Path(tmp) / f"rank{rank}")
        m.rank, m.world_size = rank, world
        m.hparams.batch_size = BS
        u = torch.from_numpy(gold["boundary_u"])  # the recorded boundary draws, this rank's rows
        mine = u[:, rank * BS:(rank + 1) * BS]
        fill = torch.full((u.shape[0], BS - mine.shape[1], u.shape[2]), 0.5)
        m.noise = {"boundary_u": torch.cat([mine, fill], dim=1).contiguous().cuda()}
        m.modules.eval()
        m.on_stage_start(Stage.TEST, None)
        batch = _first_batch(_items(gold, meta, False), BS, rank, world, Stage.TEST)
        with torch.no_grad():
            m.evaluate_batch(batch, Stage.TEST)
            m.on_stage_end(Stage.TEST, 0.0, None)
        saved = Path(tmp) / f"rank{rank}" / "ds" / "saved_md_results" / "md_vae_tiny.json"
        out["TEST"] = {"ids": list(batch["id"]),
                       "md": m.stats_loggers["plvl_md_stats"].summarize(),
                       "boundary": m.stats_loggers["boundary_stats"].summarize(),
                       "saved": json.load(open(saved)) if saved.exists() else None,
                       "metrics": (Path(tmp) / f"rank{rank}" / "test_output" / "test_metrics.txt").exists()}
        q.put(out)
    except BaseException as e:  # the parent fails with the worker's reason instead of waiting
        import traceback
        q.put({"rank": rank, "error": f"{e!r}\n{traceback.format_exc()}"})
    finally:
        dist.destroy_process_group()


def _single_process(gold, tmp_path, name):
    """Loss and gradients of the four utterances as one batch on the single-process path."""
    from brain import Stage
    from models.MD_VAE.model import Target
    m, meta = MD._model(gold, tmp_path / "one")
    m.hparams.batch_size = 2 * BS
    m.noise = None
    m.modules.train()
    m.target = Target[name]
    m.stats_loggers = {}
    batch = _first_batch(_items(gold, meta, True), 2 * BS, 0, 1, Stage.TRAIN)
    torch.manual_seed(SEED)
    loss = m.compute_objectives(m.compute_forward(batch, Stage.TRAIN), batch, Stage.TRAIN)
    loss.backward()
    m._raise_device_errors()
    return float(loss.detach()), _grads(m)


def test_two_ranks_take_the_single_process_step(tmp_path):
    need_gpu()
    from mlvae_hip._lib import device_cus, lib
    gold = _gold()
    meta = json.loads(str(gold["meta_json"]))
    assert meta["H"] <= 64 and BS <= 4
    for fwd in (0, 1):  # two ranks' persistent recurrences must be co-resident
        assert 2 * lib().mlvae_lstm_launch_workgroups(BS, meta["H"], 0, fwd) <= device_cus()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    for _ in range(360):  # ends as soon as both reported, or a worker died without reporting
        try:
            res.append(q.get(timeout=0.5))
        except queue.Empty:
            if not any(p.is_alive() for p in procs):
                break
        if len(res) == len(procs):
            break
    for p in procs:
        p.join(timeout=30)
    assert len(res) == 2, "a worker ended without a result"
    for r in res:
        assert "error" not in r, r["error"]
    res.sort(key=lambda r: r["rank"])
    for name in TARGETS:
        a, b = res[0][name], res[1][name]
        assert a["all_reduces"] == 1 and b["all_reduces"] == 1, (name, a["all_reduces"], b["all_reduces"])
        for n in a["params"]:
            assert np.array_equal(a["params"][n], b["params"][n]), (name, n)
        loss, grads = _single_process(gold, tmp_path, name)
        assert a["loss"] == b["loss"]
        e = abs(a["loss"] - loss) / abs(loss)
        print(f"{name}: reduced loss {a['loss']:.7f} single process {loss:.7f} rel {e:.2e}")
        assert e < 1e-5
        worst = ("", 0.0)
        for n, g in grads.items():
            assert (g is None) == (a["grads"][n] is None) == (b["grads"][n] is None), (name, n)
            if g is None:
                continue
            assert np.array_equal(a["grads"][n], b["grads"][n]), (name, n)
            e = rel_err(torch.from_numpy(a["grads"][n]), torch.from_numpy(g))
            if e > worst[1]:
                worst = (n, e)
            assert e < 1e-4, (name, n, e)
        print(f"{name}: worst reduced gradient {worst[0]} rel {worst[1]:.2e}")
    t0, t1 = res[0]["TEST"], res[1]["TEST"]
    assert t0["ids"] == ["utt0", "utt1"] and t1["ids"] == ["utt2", "__pad__"]
    for t in (t0, t1):  # merged on every rank
        assert t["md"] == json.loads(str(gold["TEST/md_summary_json"]))
        assert t["boundary"] == json.loads(str(gold["TEST/boundary_summary_json"]))
    assert t1["saved"] is None and not t1["metrics"]  # rank 0 alone writes
    assert t0["metrics"] and sorted(t0["saved"]) == ["utt0", "utt1", "utt2"]
    want = json.loads(str(gold["TEST/saved_md_result_json"]))
    for k in want:
        assert len(t0["saved"][k]) == len(want[k])
        for x, y in zip(t0["saved"][k], want[k]):
            assert x[0] == y[0] and x[1:] == pytest.approx(y[1:], rel=1e-6)
