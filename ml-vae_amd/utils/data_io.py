"""Datasets of the recipe (ref:src/utils/data_io.py:24-146).

* ``PickledSet``: the reference's pre-computed corpora, ``<dataset_dir>/../computed_dataset/
  {train,valid,test}.pkl`` = {utt_id: {key: value}} over ``output_keys`` (written by the
  reference's prepare_datasets, ref:src/utils/data_io.py:40-104).  The Kaldi / librosa feature
  computation that produces them is out of scope; when the files exist they are read as is.
* ``SyntheticSet``: F-dim frames, lengths uniform in [min_frames, max_frames], values
  log(1e-6 + |N(0,1)|^2) standardised (log-mel-like), seeded.  ``md_labels=True``
  (``synthetic.md_labels`` in config/run.yaml) adds the fields the MD-VAE recipe reads --
  gt_cnncl_seq, fa_boundary_seq, gt_boundary_seq, plvl_gt_md_lbl_seq, prior -- drawn from a
  generator of their own per utterance, so the features are the same with and without them,
  and flvl_gt_md_lbl_seq (the LSTM_FC baseline's frame-level targets), derived from them.
  ``phn_labels=True`` (``synthetic.phn_labels``) with it adds flvl_gt_cnncl_seq, the canonical
  phoneme id of every frame (test_phn_classifier's frame-level targets), derived likewise: it
  takes no draw, so every other field is the same with and without it.  ``ali_labels=True``
  (``synthetic.ali_labels``) with md_labels adds gt_phn_end_seq, the exclusive end of every
  gt_boundary_seq segment in samples (the HMM_DNN_ALI aligner's ground truth), derived too.
  ``waveforms=True`` (``synthetic.waveforms``) with md_labels makes the corpus spoken: wav and
  gt_phn_seq from a third generator per utterance, feat = compute_features(wav) (the Fbank front
  end, brain.features.Fbank) -- see SyntheticSet.  ``kaldi_feats=True``
  (``synthetic.kaldi_feats``) with waveforms adds spk and kaldi_feat, the Kaldi-compatible front
  end with per-speaker CMVN (brain.features.KaldiFbank, SpeakerCMVN).

Batches follow SpeechBrain's PaddedBatch: batch['feat'] = (padded [B, Tmax, F], relative lengths
[B]).  Under data parallelism rank r of W reads utterances [r*bs, (r+1)*bs) of every global batch
of W*bs, padded to that global batch's longest utterance (so every rank sees the single-process
batch's T and relative lengths).  TRAIN drops an incomplete last global batch (every rank runs
the same number of optimizer steps); VALID / TEST keep it: ranks whose slice of the remainder is
short fill it with zero-length utterances (id ``__pad__``), which every masked mean and frame
count excludes.  Each data-parallel batch also carries, as attributes, what a rank needs to take
its share of the global batch without a collective: ``global_lens`` ({field: the relative
lengths of the whole global batch, fillers not among them}), ``utt_offset`` (the global index of
its first row), ``global_size`` (utterances of the global batch) and ``global_index`` (which
global batch of the split this is)."""
import io
import pickle
from pathlib import Path

import numpy as np
import torch

from brain.dataio import PaddedBatch

# the reference's keys (ref:src/utils/data_io.py:24-37)
output_keys = [
    'id', 'wav', 'aug_wav', 'duration', 'feat', 'aug_feat', 'kaldi_feat', 'aug_kaldi_feat',
    'gt_phn_seq', 'gt_cnncl_seq', 'flvl_gt_phn_seq', 'flvl_gt_cnncl_seq', 'aug_flvl_gt_cnncl_seq',
    'plvl_gt_md_lbl_seq', 'flvl_gt_md_lbl_seq', 'aug_flvl_gt_md_lbl_seq', 'gt_seg_seq',
    'gt_boundary_seq', 'gt_phn_end_seq', 'fa_seg_seq', 'fa_boundary_seq', 'fa_phn_end_seq', 'prior',
]


PAD_ID = "__pad__"  # the zero-length fillers of a short rank slice (never an utterance: no scores)


def _seq_max(items):
    """{field: longest sequence} over the given utterances (tensor fields with a time axis)."""
    out = {}
    for e in items:
        for k, v in e.items():
            if torch.is_tensor(v) and v.dim() >= 1:
                out[k] = max(out.get(k, 0), v.shape[0])
    return out


def _empty_like(e):
    """A zero-length utterance with the fields of e (fills a short rank slice in evaluation)."""
    d = {"id": PAD_ID}
    for k, v in e.items():
        if k == "id":
            continue
        d[k] = v.new_zeros((0,) + tuple(v.shape[1:])) if torch.is_tensor(v) and v.dim() >= 1 else v
    return d


def _global_lens(glob, pad_to):
    """{field: relative lengths [len(glob)]} of the global batch, as PaddedBatch computes them."""
    out = {}
    for k, tmax in pad_to.items():
        vals = [e[k] for e in glob]
        if all(torch.is_tensor(v) and v.dim() >= 1 for v in vals):
            out[k] = torch.tensor([v.shape[0] / tmax if tmax else 0.0 for v in vals],
                                  dtype=torch.float32)
    return out


def _batched(items, batch_size, rank=0, world=1, stage=None, skip=0):
    """skip: the first `skip` batches are passed over at the index level (not collated)."""
    if world <= 1:
        for i in range(skip * batch_size, len(items), batch_size):
            yield PaddedBatch(items[i:i + batch_size])
        return
    g = batch_size * world
    train = stage is None or getattr(stage, "name", str(stage)).upper() == "TRAIN"
    end = len(items) - g + 1 if train else len(items)
    for i in range(skip * g, max(end, 0), g):
        glob = items[i:i + g]
        mine = glob[rank * batch_size:(rank + 1) * batch_size]
        mine = mine + [_empty_like(glob[0])] * (batch_size - len(mine))
        pad_to = _seq_max(glob)
        batch = PaddedBatch(mine, pad_to=pad_to)
        batch.global_lens = _global_lens(glob, pad_to)
        batch.utt_offset = rank * batch_size
        batch.global_size = len(glob)
        batch.global_index = i // g
        yield batch


class BatchLoader:
    """The batches of one split, re-iterable: every pass (epoch) is a fresh walk over the items,
    as a DataLoader is (a bare generator would leave every epoch after the first empty).
    skip_next(n) makes the next pass start at batch n -- the resume point of an intra-epoch
    checkpoint -- without collating the batches it passes over.  `signature` is what must match
    for such a resume to skip the right utterances (batch size, world size, sorting, length)."""

    def __init__(self, items, batch_size, rank=0, world=1, stage=None, sorting=None):
        self.items, self.batch_size, self.rank, self.world = items, batch_size, rank, world
        self.stage, self.sorting = stage, sorting
        self._skip = 0

    def __len__(self):
        g = self.batch_size * self.world
        train = self.world > 1 and (self.stage is None or
                                    getattr(self.stage, "name", str(self.stage)).upper() == "TRAIN")
        return len(self.items) // g if train else (len(self.items) + g - 1) // g

    def skip_next(self, n):
        self._skip = int(n)

    def __iter__(self):
        skip, self._skip = self._skip, 0
        return _batched(self.items, self.batch_size, self.rank, self.world, self.stage, skip)

    def signature(self):
        return {"batch_size": self.batch_size, "world_size": self.world, "sorting": self.sorting,
                "n_batches": len(self)}


def _storage_from_bytes(b):
    """torch.storage._load_from_bytes without its weights_only=False: the tensor storages the
    reference's pickles hold load through torch's restricted (weights-only) unpickler."""
    return torch.load(io.BytesIO(b), weights_only=True)


class _CorpusUnpickler(pickle.Unpickler):
    """The reference's computed_dataset/*.pkl holds plain containers, numbers, strings, numpy
    arrays and torch tensors (SpeechBrain pipeline outputs); anything else (an arbitrary callable
    a crafted file could name) is refused."""
    _ALLOWED = {
        ("builtins", "dict"), ("builtins", "list"), ("builtins", "tuple"), ("builtins", "set"),
        ("builtins", "frozenset"), ("builtins", "int"), ("builtins", "float"), ("builtins", "str"),
        ("builtins", "bytes"), ("builtins", "bool"), ("builtins", "complex"),
        ("collections", "OrderedDict"),
        ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.multiarray", "_reconstruct"),
        ("numpy._core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"),
        ("numpy._core.multiarray", "scalar"), ("torch._utils", "_rebuild_tensor_v2"),
        ("torch", "Size"), ("torch", "float32"), ("torch", "float64"), ("torch", "int64"),
    }

    def find_class(self, module, name):
        if (module, name) == ("torch.storage", "_load_from_bytes"):
            return _storage_from_bytes
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"computed dataset pickle names {module}.{name}: refused "
                                     "(only containers, numbers, strings and numpy arrays load)")


def load_corpus_pickle(path):
    """Restricted load of a computed_dataset/*.pkl (no code from the file is executed)."""
    with open(path, "rb") as f:
        return _CorpusUnpickler(io.BytesIO(f.read())).load()


def _sort(items, sorting):
    if sorting == "descending":
        items.sort(key=lambda e: -e["feat"].shape[0])
    elif sorting == "ascending":
        items.sort(key=lambda e: e["feat"].shape[0])
    return items


class PickledSet:
    """One split of the reference's computed dataset (a dict of per-utterance dicts)."""

    def __init__(self, pkl_path, sorting="descending"):
        data = load_corpus_pickle(pkl_path)  # restricted: containers / numbers / numpy arrays
        self.items = []
        for utt_id, d in data.items():
            e = {"id": utt_id}
            for k, v in d.items():
                if isinstance(v, np.ndarray):
                    v = torch.from_numpy(v)
                elif isinstance(v, list) and v and isinstance(v[0], (int, float)):
                    v = torch.tensor(v)
                if k == "feat" and torch.is_tensor(v):
                    v = v.float()
                e[k] = v
            self.items.append(e)
        _sort(self.items, sorting)
        self.sorting = sorting

    def __len__(self):
        return len(self.items)

    def batches(self, stage=None, batch_size=8, rank=0, world=1, **_):
        return BatchLoader(self.items, batch_size, rank, world, stage, self.sorting)


MIN_SEG = 5   # frames of the shortest synthetic phoneme segment
JITTER = 2    # gt boundaries = forced-alignment boundaries moved by up to this many frames


def _label_generator(seed, index):
    """The label stream of one utterance (index -1: the set's prior): its own generator, so the
    feature stream `g` of SyntheticSet draws exactly what it draws without labels."""
    return torch.Generator().manual_seed((int(seed) * 1000003 + index + 1) % (2 ** 63 - 1) + 0x4D44)


def _synthetic_md_labels(T, n_phonemes, g, phn_labels=False):
    """The MD fields of one utterance of T frames (what phn_bce, the Viterbi decode and
    boundary_md_scoring assert: a boundary at frame 0, one boundary per phoneme, ids in range):
    L phonemes, L in [max(2, T // 12), max(2, T // 8)], each at least MIN_SEG frames long."""
    lo, hi = max(2, T // 12), max(2, T // 8)
    L = min(int(torch.randint(lo, hi + 1, (1,), generator=g)), max(T // MIN_SEG, 1))
    # durations: MIN_SEG each, the remaining frames dealt out at random
    extra = torch.randint(0, L, (max(T - MIN_SEG * L, 0),), generator=g)
    dur = torch.bincount(extra, minlength=L) + min(MIN_SEG, T // L)
    starts = torch.cumsum(dur, 0) - dur
    fa = torch.zeros(T)
    fa[starts] = 1.0
    # interior boundaries move by at most JITTER < MIN_SEG / 2 frames: order and count are kept
    move = torch.randint(-JITTER, JITTER + 1, (L,), generator=g)
    move[0] = 0
    if min(MIN_SEG, T // L) < MIN_SEG:
        move.zero_()
    gt = torch.zeros(T)
    gt[starts + move] = 1.0
    cnncl = torch.randint(0, n_phonemes, (L,), generator=g, dtype=torch.int64)
    plvl = (torch.rand(L, generator=g) < 0.2).to(torch.int64)
    # frame level: each phoneme's label over its gt_boundary_seq segment (no draw of its own)
    seg = torch.cumsum(gt, 0).to(torch.int64) - 1
    flvl = plvl[seg]
    out = {
        "gt_cnncl_seq": cnncl,
        "fa_boundary_seq": fa,
        "gt_boundary_seq": gt,
        "plvl_gt_md_lbl_seq": plvl,
        "flvl_gt_md_lbl_seq": flvl,
    }
    if phn_labels:  # each phoneme's canonical id over its gt_boundary_seq segment (no draw either)
        out["flvl_gt_cnncl_seq"] = cnncl[seg]
    return out


def _phn_end_seq(gt_boundary_seq, samples_per_frame):
    """Exclusive end of every gt_boundary_seq segment, in samples (int64 [L]): derived, no draw."""
    starts = torch.where(gt_boundary_seq == 1)[0]
    ends = torch.cat([starts[1:], starts.new_tensor([gt_boundary_seq.shape[0]])])
    return ends.to(torch.int64) * int(samples_per_frame)


F1_HZ = (300, 420, 560, 720, 900, 1100)                 # first tone of a spoken phoneme: id % 6
F2_HZ = (1400, 1700, 2050, 2450, 2900, 3400, 4000)      # second tone: (id // 6) % 7
MAX_SPOKEN_PHONEMES = len(F1_HZ) * len(F2_HZ)           # 42 distinct tone pairs
WAV_NOISE = 0.01                                        # white noise floor of the waveform
WAV_BATCH = 16                                          # utterances per front-end call


def _wave_generator(seed, index):
    """The waveform stream of one utterance (pronounced ids, phases, noise): its own generator,
    as _label_generator, so neither the features' nor the labels' draws move."""
    return torch.Generator().manual_seed((int(seed) * 1000003 + index + 1) % (2 ** 63 - 1) + 0x5756)


def _spoken_utterance(e, n_phonemes, samples_per_frame, sample_rate, g):
    """(gt_phn_seq int64 [L], wav float32 [T samples_per_frame]) of one labelled utterance: the
    pronounced id is the canonical one where plvl_gt_md_lbl_seq is 0 and another one where it is
    1; every gt_boundary_seq segment sounds the two tones of its pronounced id."""
    cnncl, plvl, gt = e["gt_cnncl_seq"], e["plvl_gt_md_lbl_seq"], e["gt_boundary_seq"]
    L, T = cnncl.shape[0], gt.shape[0]
    other = (cnncl + 1 + torch.randint(0, n_phonemes - 1, (L,), generator=g)) % n_phonemes
    phn = torch.where(plvl == 1, other, cnncl)
    ends = _phn_end_seq(gt, samples_per_frame).tolist()
    phase = 2 * np.pi * torch.rand(L, 2, generator=g, dtype=torch.float64).numpy()
    n = np.arange(T * samples_per_frame, dtype=np.float64)
    wav = np.empty_like(n)
    lo = 0
    for k, hi in enumerate(ends):
        p = int(phn[k])
        w1 = 2 * np.pi * F1_HZ[p % len(F1_HZ)] / sample_rate
        w2 = 2 * np.pi * F2_HZ[(p // len(F1_HZ)) % len(F2_HZ)] / sample_rate
        wav[lo:hi] = 0.5 * np.sin(w1 * n[lo:hi] + phase[k, 0]) + 0.3 * np.sin(w2 * n[lo:hi] + phase[k, 1])
        lo = hi
    noise = torch.randn(T * samples_per_frame, generator=g, dtype=torch.float64).numpy()
    return phn, torch.from_numpy((wav + WAV_NOISE * noise).astype(np.float32))


def _wav_batches(items):
    """(utterances, padded wav [B, N], relative lengths [B]) in batches of WAV_BATCH, on the device
    when there is one."""
    dev = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    for i in range(0, len(items), WAV_BATCH):
        part = items[i:i + WAV_BATCH]
        N = max(e["wav"].shape[0] for e in part)
        wav = torch.zeros(len(part), N)
        for j, e in enumerate(part):
            wav[j, :e["wav"].shape[0]] = e["wav"]
        lens = torch.tensor([e["wav"].shape[0] / N for e in part], dtype=torch.float32)
        yield part, wav.to(dev), lens.to(dev)


def _spoken_features(items, compute_features, feat_dim):
    """feat = compute_features(wav) of every utterance, in padded batches of WAV_BATCH, trimmed to
    the labels' T frames (the front end yields T + 1; ref:src/utils/data_io.py:199-201 trims the
    same way), kept on the host as the random features are."""
    for part, wav, lens in _wav_batches(items):
        feats = torch.as_tensor(compute_features(wav, lens)).detach().cpu().float()
        for j, e in enumerate(part):
            T = e["feat"].shape[0]
            if feats.dim() != 3 or feats.shape[1] < T:
                raise ValueError(f"synthetic corpus: compute_features gave {tuple(feats.shape)} for "
                                 f"an utterance of {T} frames")
            if feats.shape[2] != feat_dim:
                raise ValueError(f"synthetic corpus: compute_features gives {feats.shape[2]}-d frames, "
                                 f"the model's input_size is {feat_dim}")
            e["feat"] = feats[j, :T].clone()


def _kaldi_features(items, compute_kaldi_features, cmvn, n_speakers):
    """spk = utterance index % n_speakers and kaldi_feat = the Kaldi-compatible front end with
    per-speaker CMVN over the split (ref:src/utils/data_io_utils.py:150-206), in two passes of
    WAV_BATCH-sized batches: the raw features and the speakers' statistics, then the normalisation.
    `items` is in utterance order.  T samples_per_frame samples give exactly T frames."""
    for i, e in enumerate(items):
        e["spk"] = i % n_speakers
    cmvn.reset()
    raw = []
    for part, wav, lens in _wav_batches(items):
        feats = torch.as_tensor(compute_kaldi_features(wav, lens)).detach().float()
        frames = [e["feat"].shape[0] for e in part]
        if feats.dim() != 3 or feats.shape[1] != max(frames):
            raise ValueError(f"synthetic corpus: compute_kaldi_features gave {tuple(feats.shape)} for "
                             f"utterances of up to {max(frames)} frames (hop_length must be "
                             "samples_per_frame samples)")
        if feats.shape[2] != cmvn.dim:
            raise ValueError(f"synthetic corpus: compute_kaldi_features gives {feats.shape[2]}-d frames, "
                             f"the model's input_size is {cmvn.dim}")
        spk = [e["spk"] for e in part]
        cmvn.accumulate(feats, frames, spk)
        raw.append((part, feats.cpu(), frames, spk, feats.device))
    for part, feats, frames, spk, dev in raw:
        feats = torch.as_tensor(cmvn.apply(feats.to(dev), frames, spk)).detach().cpu().float()
        for j, e in enumerate(part):
            e["kaldi_feat"] = feats[j, :frames[j]].clone()


class SyntheticSet:
    """waveforms=True (``synthetic.waveforms``, with md_labels) makes the corpus *spoken*: every
    utterance gets gt_phn_seq (the pronounced ids: canonical where plvl_gt_md_lbl_seq is 0,
    another id where it is 1) and wav (T samples_per_frame float32 samples: two tones per
    pronounced phoneme over its gt_boundary_seq segment plus a noise floor), and feat becomes
    compute_features(wav) -- so the features carry the labels.  Every other field keeps the value
    it has without waveforms: the feature generator still takes its draws and the new fields come
    from a generator of their own per utterance.  Under data parallelism every rank builds the
    same corpus (nothing here depends on the rank) and reads its slice of each batch.

    kaldi_feats=True (``synthetic.kaldi_feats``, with waveforms) adds two fields and changes no
    other: spk = utterance index % n_speakers, and kaldi_feat [T, feat_dim] float32 =
    compute_kaldi_features(wav) (brain.features.KaldiFbank) normalised per speaker over the split
    (`speaker_cmvn`: an object with reset / accumulate / apply, brain.features.SpeakerCMVN when
    None) -- the reference's `kaldi_feat`, which MD_VAE_sfl reads under use_kaldi_feat."""

    def __init__(self, n_utts, feat_dim, min_frames, max_frames, seed, sorting="descending",
                 md_labels=False, n_phonemes=39, phn_labels=False, ali_labels=False,
                 samples_per_frame=320, waveforms=False, compute_features=None, sample_rate=16000,
                 kaldi_feats=False, n_speakers=4, compute_kaldi_features=None, speaker_cmvn=None):
        if ali_labels and not md_labels:
            raise ValueError("synthetic corpus: ali_labels needs md_labels")
        if kaldi_feats:
            if not waveforms:
                raise ValueError("synthetic corpus: kaldi_feats needs waveforms (kaldi_feat is computed "
                                 "from the synthesised waveform)")
            if compute_kaldi_features is None:
                raise ValueError("synthetic corpus: kaldi_feats needs compute_kaldi_features "
                                 "(config/run.yaml's compute_kaldi_features: the KaldiFbank front end)")
            if int(n_speakers) < 1:
                raise ValueError(f"synthetic corpus: n_speakers = {n_speakers} must be >= 1")
        if waveforms:
            if not md_labels:
                raise ValueError("synthetic corpus: waveforms needs md_labels (the waveform is "
                                 "synthesised from the phoneme and boundary labels)")
            if not 2 <= n_phonemes <= MAX_SPOKEN_PHONEMES:
                raise ValueError(f"synthetic corpus: waveforms has {MAX_SPOKEN_PHONEMES} distinct tone "
                                 f"pairs, n_phonemes = {n_phonemes} must be in [2, {MAX_SPOKEN_PHONEMES}]")
            if compute_features is None:
                raise ValueError("synthetic corpus: waveforms needs compute_features (config/run.yaml's "
                                 "compute_features: the Fbank front end)")
        g = torch.Generator().manual_seed(seed)
        lens = torch.randint(min_frames, max_frames + 1, (n_utts,), generator=g)
        self.items = []
        for i, L in enumerate(lens.tolist()):
            x = torch.log(1e-6 + torch.randn(L, feat_dim, generator=g) ** 2)
            x = (x - x.mean()) / x.std()
            self.items.append({"id": f"utt{i:05d}", "feat": x})
        if md_labels:
            # the decode's phoneme prior, in (0.05, 0.5): one per set, carried by every utterance
            prior = 0.06 + 0.43 * torch.rand(n_phonemes + 2, generator=_label_generator(seed, -1))
            for i, e in enumerate(self.items):
                e.update(_synthetic_md_labels(e["feat"].shape[0], n_phonemes, _label_generator(seed, i),
                                              phn_labels=phn_labels))
                e["prior"] = prior.clone()
                if ali_labels:
                    e["gt_phn_end_seq"] = _phn_end_seq(e["gt_boundary_seq"], samples_per_frame)
        if waveforms:
            for i, e in enumerate(self.items):
                e["gt_phn_seq"], e["wav"] = _spoken_utterance(e, n_phonemes, int(samples_per_frame),
                                                              int(sample_rate), _wave_generator(seed, i))
            _spoken_features(self.items, compute_features, feat_dim)
        if kaldi_feats:
            if speaker_cmvn is None:
                from brain.features import SpeakerCMVN
                speaker_cmvn = SpeakerCMVN(int(n_speakers), feat_dim)
            _kaldi_features(self.items, compute_kaldi_features, speaker_cmvn, int(n_speakers))
        _sort(self.items, sorting)
        self.sorting = sorting

    def __len__(self):
        return len(self.items)

    def batches(self, stage=None, batch_size=8, rank=0, world=1, **_):
        return BatchLoader(self.items, batch_size, rank, world, stage, self.sorting)


def computed_dataset_dir(hparams):
    return Path(hparams["prepare"]["dataset_dir"]).parent / "computed_dataset"


def prepare_datasets(hparams):
    cdir = computed_dataset_dir(hparams)
    if hparams.get("dataset") != "synthetic" or all((cdir / f"{s}.pkl").exists() for s in ("train", "valid", "test")):
        missing = [s for s in ("train", "valid", "test") if not (cdir / f"{s}.pkl").exists()]
        if missing:
            raise FileNotFoundError(
                f"computed dataset {cdir}/{{{','.join(missing)}}}.pkl not found: the Kaldi / librosa "
                "feature preparation of ref:src/utils/data_io.py:56-93 is not part of this build; "
                "point prepare.dataset_dir at a corpus the reference has already computed")
        return [PickledSet(cdir / f"{s}.pkl", hparams.get("sorting", "descending"))
                for s in ("train", "valid", "test")], None
    d = hparams.get("synthetic", {})
    F = hparams["model"]["input_size"]
    sets = []
    for j, split in enumerate(("train", "valid", "test")):
        sets.append(SyntheticSet(d.get(f"n_{split}", 32), F, d.get("min_frames", 50),
                                 d.get("max_frames", 200), hparams.get("seed", 123456) + j,
                                 hparams.get("sorting", "descending"),
                                 md_labels=bool(d.get("md_labels", False)),
                                 n_phonemes=int(hparams.get("n_phonemes", 39)),
                                 phn_labels=bool(d.get("phn_labels", False)),
                                 ali_labels=bool(d.get("ali_labels", False)),
                                 samples_per_frame=int(hparams.get("sample_rate", 16000)) *
                                 int(hparams.get("hop_length", 20)) // 1000,
                                 waveforms=bool(d.get("waveforms", False)),
                                 compute_features=hparams.get("compute_features"),
                                 sample_rate=int(hparams.get("sample_rate", 16000)),
                                 kaldi_feats=bool(d.get("kaldi_feats", False)),
                                 n_speakers=int(d.get("n_speakers", 4)),
                                 compute_kaldi_features=hparams.get("compute_kaldi_features")))
    return sets, None
