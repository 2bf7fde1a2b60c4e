"""Data-parallel plumbing of the MD recipes that needs no GPU:

* utils.data_io's loader under world > 1: every rank's batch carries the global batch's relative
  lengths per sequence field, its utterance offset, the global batch's size and index; a short
  rank slice of an evaluation remainder is filled with ``__pad__`` rows;
* utils.metric_stats: ``__pad__`` rows are never scored, and the ranks' states merged in the
  order (global batch index, rank, position) summarise exactly as the single process's list."""
import torch

from utils.data_io import PAD_ID, SyntheticSet
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
from utils.metric_stats.md_metric_stats import MDMetricStats


def _set(n):
    return SyntheticSet(n, 4, 20, 40, seed=5, sorting="descending", md_labels=True, n_phonemes=5)


def _check_world(n_utts, bs, world, stage):
    ds = _set(n_utts)
    single = list(ds.batches(stage=stage, batch_size=bs * world))
    ranks = [list(ds.batches(stage=stage, batch_size=bs, rank=r, world=world)) for r in range(world)]
    train = stage == "TRAIN"
    n_glob = n_utts // (bs * world) if train else -(-n_utts // (bs * world))
    assert all(len(b) == n_glob for b in ranks)
    seen = []
    for i in range(n_glob):
        whole = single[i]
        G = len(whole["id"])
        for r in range(world):
            b = ranks[r][i]
            assert (b.utt_offset, b.global_size, b.global_index) == (r * bs, G, i)
            assert len(b["id"]) == bs
            for field, lens in b.global_lens.items():  # the single process's lengths, all of them
                assert torch.equal(lens, whole[field][1]), field
            assert {"feat", "gt_cnncl_seq", "fa_boundary_seq"} <= set(b.global_lens)
            for j, utt in enumerate(b["id"]):
                g = r * bs + j
                if g < G:
                    assert utt == whole["id"][g]
                    for field in b.global_lens:  # same padding, same relative length, same data
                        assert b[field][0].shape[1:] == whole[field][0].shape[1:]
                        assert b[field][1][j] == whole[field][1][g]
                        assert torch.equal(b[field][0][j], whole[field][0][g])
                    seen.append(utt)
                else:
                    assert utt == PAD_ID and not train
                    assert float(b["feat"][1][j]) == 0.0
    return seen, [u for b in single for u in b["id"]][:len(seen)]


def test_loader_global_fields_world_2_and_3():
    for world in (2, 3):
        seen, want = _check_world(12, 2, world, "TRAIN")
        assert seen == want and len(seen) == 12
        # a remainder: 11 utterances leave a last global batch of 11 % (2 world) rows
        seen, want = _check_world(11, 2, world, "TEST")
        assert seen == want and len(seen) == 11
        seen, _ = _check_world(11, 2, world, "TRAIN")  # TRAIN drops the incomplete global batch
        assert len(seen) == 11 // (2 * world) * (2 * world)


def test_single_process_batches_carry_no_dp_fields():
    b = next(iter(_set(4).batches(stage="TEST", batch_size=2)))
    assert not hasattr(b, "global_lens") and not hasattr(b, "utt_offset")


# ------------------------------------------------------------------------------------- metrics
def _utts(n, seed):
    """n utterances: (id, predicted / true phoneme labels, predicted / true boundary sequences)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        L = int(torch.randint(2, 6, (1,), generator=g))
        T = 5 * L
        starts = torch.arange(L) * 5
        gt_b, pr_b = torch.zeros(T), torch.zeros(T)
        gt_b[starts] = 1
        move = torch.randint(0, 3, (L,), generator=g)
        move[0] = 0
        pr_b[starts + move] = 1
        out.append((f"u{i}", torch.randint(0, 2, (L,), generator=g).tolist(),
                    torch.randint(0, 2, (L,), generator=g).tolist(), pr_b.numpy().astype("int64"),
                    gt_b.tolist()))
    return out


def _append(md, bnd, rows, batch_index=None):
    ids = [r[0] for r in rows]
    md.append(ids=ids, batch_index=batch_index, pred_md_lbl_seqs=[r[1] for r in rows],
              gt_md_lbl_seqs=[r[2] for r in rows], pred_boundary_seqs=[r[3] for r in rows],
              gt_boundary_seqs=[r[4] for r in rows])
    bnd.append(ids=ids, batch_index=batch_index, predictions=[r[3] for r in rows],
               targets=[r[4] for r in rows])


PAD_ROW = (PAD_ID, [], [], torch.zeros(0).numpy().astype("int64"), [])


def test_rank_states_merge_to_the_single_process_summary():
    utts = _utts(7, 3)  # global batches of 4: [0:4], then a remainder of 3
    md1, bnd1 = MDMetricStats(), BoundaryMetricStats()
    _append(md1, bnd1, utts[0:4])
    _append(md1, bnd1, utts[4:7])
    # two ranks, batch size 2: rank 1's slice of the remainder is one utterance and one filler
    slices = {0: [utts[0:2], utts[4:6]], 1: [utts[2:4], [utts[6], PAD_ROW]]}
    states_md, states_bnd = [], []
    for r in (0, 1):
        md, bnd = MDMetricStats(), BoundaryMetricStats()
        for i, rows in enumerate(slices[r]):
            _append(md, bnd, rows, batch_index=i)
        assert PAD_ID not in md.ids and PAD_ID not in bnd.ids
        assert PAD_ID not in md.saved_seqs["utt_ids"]
        states_md.append(md.state())
        states_bnd.append(bnd.state())
    md, bnd = MDMetricStats(), BoundaryMetricStats()
    md.merge(states_md)
    bnd.merge(states_bnd)
    assert md.ids == md1.ids == [u[0] for u in utts] and bnd.ids == bnd1.ids
    assert md.summarize() == md1.summarize()
    assert bnd.summarize() == bnd1.summarize()
    for k in md1.metric_keys:  # not only the rounded means: every score, in order
        assert [float(s[k]) for s in md.scores_list] == [float(s[k]) for s in md1.scores_list]
    assert md.saved_seqs == md1.saved_seqs
    # merged rank-major instead, the ids come out in another order (what the merge prevents)
    assert states_md[0]["ids"] + states_md[1]["ids"] != md1.ids


def test_counts_drop_fillers_and_merge():
    counts = torch.tensor([[5, 2, 1, 0], [3, 0, 2, 2], [0, 0, 0, 0], [4, 4, 0, 1]], dtype=torch.int32)
    one = MDMetricStats()
    one.append_counts(["a", "b", "c"], counts[[0, 1, 3]])
    r0, r1 = MDMetricStats(), MDMetricStats()
    r0.append_counts(["a", "b"], counts[0:2], batch_index=0)
    r1.append_counts([PAD_ID, "c"], counts[2:4], batch_index=0)
    assert r1.state()["ids"] == ["c"]
    m = MDMetricStats()
    m.merge([r0.state(), r1.state()])
    assert m.ids == ["a", "b", "c"]
    assert m.summarize() == one.summarize()
    # a rank that saw fillers only contributes nothing
    r2 = MDMetricStats()
    r2.append_counts([PAD_ID], counts[2:3], batch_index=0)
    m.merge([r0.state(), r1.state(), r2.state()])
    assert m.ids == ["a", "b", "c"] and m.summarize() == one.summarize()
