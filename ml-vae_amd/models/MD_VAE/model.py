"""The MD-VAE recipe (semantics of ref:src/models/MD_VAE/model.py:24-273).

Three training targets in a cycle -- the phoneme recogniser (epochs 1, 4, ...), the boundary
detector (2, 5, ...), the VAE (3, 6, ...) -- for TRAIN and for VALID; metrics, train_log lines
and checkpoints (max_key plvl_md.F1) come from VALID under the VAE target and from TEST only.

compute_forward, in the reference's order: normaliser; phoneme recogniser; boundary detector;
for the VAE / TEST targets feat_fc + phn_recog_fc -> concat_fc -> rnn -> pi_fc -> pi_logits,
sampled_pi (ops.pi_sample), the Viterbi MD decode, pi_nll_loss (ops.pi_nll on the decode's
device labels), H-VAE encoder, decoder.  Modules whose losses the reference detaches (every
upstream module outside its own target's epochs) run under torch.no_grad(): their parameters
get no gradient (.grad stays None; the optimizer and the clip skip them).

The decode stays on the device in TRAIN: its frame labels go to ops.pi_nll as the int32 tensor the
kernel wrote, and its error word (with the pi path's) is read in on_stage_end, or earlier where
the host lists are materialised (evaluation), raising the reference's AssertionError.

``self.noise`` (tests): None, or a dict with any of boundary_u [10,B,T], pi_u [B,T], eps_v,
eps_g, expo -- the draws injected into the modules instead of the library's Philox streams.
"""
import json
import logging
import warnings
from enum import Enum, auto
from pathlib import Path

import torch

from brain import Stage
from mlvae_hip import ops
from models.md_model import MDModel
from utils.data_io import PAD_ID
from utils.data_utils import apply_lens_to_loss, undo_padding
from utils.decode_utils import decode_md_device, decoded_lists, raise_decode_err
from utils.metric_stats.boundary_metric_stats import BoundaryMetricStats
from utils.metric_stats.md_metric_stats import MDMetricStats

logger = logging.getLogger(__name__)


class Target(Enum):
    PHN_RECOG = auto()
    B_DETECTOR = auto()
    VAE = auto()
    TEST = auto()


TRAIN_TARGETS = (Target.PHN_RECOG, Target.B_DETECTOR, Target.VAE)


class SBModel(MDModel):
    dp_exact = True  # data parallel: models/md_model.py's shard-exact step
    noise = None
    _decode_err = None  # the stage's decode error words, OR-ed on the device
    _phn_out_fc = "phn_recog_fc"  # the module over the recogniser's output in the pi path

    # ------------------------------------------------------------------ stages
    def on_stage_start(self, stage, epoch=None):
        super().on_stage_start(stage, epoch)
        if stage in (Stage.TRAIN, Stage.VALID):
            # VALID follows the epoch's training target (the reference's VALID -> TEST branch is
            # unreachable: kept that way)
            assert epoch is not None
            self.target = TRAIN_TARGETS[(epoch - 1) % 3]
        elif stage == Stage.TEST:
            self.target = Target.TEST
        else:
            raise ValueError(f"invalid stage {stage}")
        line = f"Epoch {epoch}, stage {stage.name}: target is {self.target.name}"
        logger.info(line)
        # train_log.txt gets lines from evaluated stages only: the schedule is recorded here
        log = Path(getattr(self.hparams, "output_dir", "")) / "train_log.txt"
        if stage != Stage.TEST and self.rank == 0 and log.is_file():
            with open(log, "a") as f:
                f.write(line + "\n")
        self._decode_err = None
        self._md_results = []  # data parallel: (global batch index, the batch's saved MD results)
        if self.to_run_evaluation(stage):  # the loss stats super() made, plus the MD metrics
            self.stats_loggers["plvl_md_stats"] = MDMetricStats()
            self.stats_loggers["boundary_stats"] = BoundaryMetricStats()
        else:
            self.stats_loggers = {}

    def to_run_evaluation(self, stage):
        return (stage == Stage.VALID and self.target == Target.VAE) or stage == Stage.TEST

    def on_stage_end(self, stage, stage_loss, epoch=None):
        self._raise_device_errors()
        if stage == Stage.TEST and self._dp():
            import torch.distributed as tdist
            parts = [None] * self.world_size
            tdist.all_gather_object(parts, self._md_results)
            if self.rank == 0:  # one writer, in the single-process order (batch, rank)
                results = {}
                for _, _, res in sorted(((b, r, res) for r, part in enumerate(parts) for b, res in part),
                                        key=lambda x: x[:2]):
                    results.update(res)
                self._write_md_results(results)
        if self.to_run_evaluation(stage):
            super().on_stage_end(stage, stage_loss, epoch)

    def _raise_device_errors(self):
        """The stage's device error words, read once (TRAIN reads none per batch)."""
        err, self._decode_err = self._decode_err, None
        if err is not None:
            raise_decode_err(err.item())
            ops.raise_pi_err()

    # ------------------------------------------------------------------ forward
    def compute_forward(self, batch, stage):
        predictions, batch, feats, feat_lens, noise = self._upstream(batch)
        if self.target in (Target.VAE, Target.TEST):
            rnn_out, pi_logits = self._pi_logits(predictions, feats, self._phn_out_fc)
            sampled_pi = ops.pi_sample(pi_logits, self.modules.training, u=noise.get("pi_u"))
            predictions["sampled_pi"] = sampled_pi
            self._decode_and_nll(predictions, batch, feat_lens, stage)

            enc = self.modules["encoder"](rnn_out, sampled_pi, eps_v=noise.get("eps_v"),
                                          eps_g=noise.get("eps_g"), expo=noise.get("expo"))
            predictions["losses"].update(enc["losses"])
            dec = self.modules["decoder"](enc["sampled_h"], feats)
            predictions["losses"].update(dec["losses"])
        return predictions

    def _upstream(self, batch):
        """Normaliser, phoneme recogniser and boundary detector for the stage's target:
        (predictions, batch on the device, feats, feat_lens, the injected noise)."""
        if not hasattr(self, "target"):
            raise ValueError("target is not defined")
        target = self.target
        noise = self.noise or {}
        batch = batch.to(self.device)
        feats, feat_lens = self._input_feats(batch)
        predictions = {"losses": {}}
        feats = feats.contiguous()

        def run(trained, fn):
            """fn() with autograd when this epoch trains the module, else without (the
            reference detaches its losses, and its output is only read detached)."""
            if trained:
                return fn()
            with torch.no_grad():
                return fn()

        fa_boundary_seqs = batch["fa_boundary_seq"][0]
        if target in (Target.PHN_RECOG, Target.VAE, Target.TEST):
            seqs, seq_lens = batch["gt_cnncl_seq"]
            phn = run(target == Target.PHN_RECOG, lambda: self.modules["phoneme_recognizer"](
                self._recog_input(feats), feat_lens, seqs, seq_lens, fa_boundary_seqs))
            predictions["phn_recog_out"] = phn["out"]
            predictions["losses"].update(phn["losses"])

        if target in (Target.B_DETECTOR, Target.VAE, Target.TEST):
            bnd = run(target == Target.B_DETECTOR, lambda: self.modules["boundary_detector"](
                self._detector_input(feats), feat_lens, fa_boundary_seqs, uniform_u=noise.get("boundary_u")))
            predictions["boundary_v"] = bnd["boundary_v"]
            predictions["losses"].update(bnd["losses"])
        return predictions, batch, feats, feat_lens, noise

    def _feat_field(self):
        """The batch field the recipe reads its input frames and their lengths from."""
        return "feat"

    def _input_feats(self, batch):
        """(input frames, relative lengths): batch['feat'] through the normaliser."""
        feats, feat_lens = batch["feat"]
        return self.hparams.normalizer(feats, feat_lens, epoch=self.hparams.epoch_counter.current), feat_lens

    # what the recogniser, the detector and the pi path read: the input frames themselves; the
    # wav2vec2 recipes (models/w2v_MD_VAE) put an FC over the encoder's features in each place
    def _recog_input(self, feats):
        return feats

    def _detector_input(self, feats):
        return feats

    def _pi_feats(self, feats):
        return self.modules["feat_fc"](feats)

    def _dp_lens_field(self, batch, stage):
        return self._feat_field()

    def _pi_logits(self, predictions, feats, phn_fc):
        """feat_fc + the recogniser output's FC (module name phn_fc) -> concat_fc -> rnn -> pi_fc:
        (rnn_out (B, T, C), pi_logits (B, T, 2))."""
        feat_fc_out = self._pi_feats(feats)
        phn_fc_out = self.modules[phn_fc](predictions["phn_recog_out"].detach())
        rnn_in = self.modules["concat_fc"](torch.cat([feat_fc_out, phn_fc_out], dim=-1))
        rnn_out = self.modules["rnn"](rnn_in)[0]          # (B, T, C)
        pi_logits = self.modules["pi_fc"](rnn_out)        # (B, T, 2)
        predictions["pi_logits"] = pi_logits
        return rnn_out, pi_logits

    def _decode_and_nll(self, predictions, batch, feat_lens, stage):
        """The Viterbi MD decode (its frame labels stay on the device) and pi_nll_loss on them."""
        seqs, seq_lens = batch["gt_cnncl_seq"]
        decoded = decode_md_device(predictions, feat_lens, seqs, seq_lens,
                                   prior=batch["prior"][0][0],
                                   weight=getattr(self.hparams, "dec_weight", 1.0),
                                   skip_empty=self._dp())  # a short rank slice's fillers
        predictions["decoded_device"] = decoded
        err = decoded[4]
        self._decode_err = err if self._decode_err is None else self._decode_err | err
        predictions["losses"]["pi_nll_loss"] = ops.pi_nll(predictions["pi_logits"], decoded[1], sync=False)
        if self.to_run_evaluation(stage):
            self._decoded_lists(predictions)

    def _decoded_lists(self, predictions):
        """The batch's decode as the reference's host lists (one sync; raises its
        AssertionError for a set error word), decoded once and kept in predictions."""
        if "decoded_lists" not in predictions:
            lists = decoded_lists(*predictions["decoded_device"])
            ops.raise_pi_err()
            predictions["decoded_lists"] = lists
            predictions["decoded_boundary_seq"] = [torch.as_tensor(s) for s in lists[0]]
            predictions["decoded_plvl_md_lbl_seq"] = [torch.tensor(s) for s in lists[2]]
        return predictions["decoded_lists"]

    # ------------------------------------------------------------------ objectives
    def compute_objectives(self, predictions, batch, stage):
        feats, feat_lens = batch[self._feat_field()]
        losses = {key: apply_lens_to_loss(value, feat_lens)
                  for key, value in predictions["losses"].items()}
        loss = self.compute_and_save_losses(losses)

        if self.to_run_evaluation(stage):
            # the forward's decode read pi_logits, boundary_v and phn_recog_out as they are
            # here: reused, not run again
            boundary_seqs, _, plvl_md_lbl_seqs = self._decoded_lists(predictions)
            gt_md_lbl_seqs = undo_padding(*batch["plvl_gt_md_lbl_seq"])
            gt_boundary_seqs = undo_padding(*batch["gt_boundary_seq"])
            bi = getattr(batch, "global_index", None)
            self.stats_loggers["plvl_md_stats"].append(
                ids=batch["id"], batch_index=bi, pred_md_lbl_seqs=plvl_md_lbl_seqs, gt_md_lbl_seqs=gt_md_lbl_seqs,
                pred_boundary_seqs=boundary_seqs, gt_boundary_seqs=gt_boundary_seqs)
            self.stats_loggers["boundary_stats"].append(
                ids=batch["id"], batch_index=bi, predictions=boundary_seqs, targets=gt_boundary_seqs)

        if stage == Stage.TEST:
            self.save_md_result(batch, predictions)
        return loss

    # ------------------------------------------------------------------ results
    def save_md_result(self, batch, predictions):
        """datasets/<dataset_name>/saved_md_results/<model_name>.json: per utterance the
        detected mispronunciations as [phoneme index, start, end], start / end relative to the
        utterance's length (merged into the file's earlier entries)."""
        self._decoded_lists(predictions)
        results = {}
        for i, utt_id in enumerate(batch["id"]):
            if utt_id == PAD_ID:  # the filler of a short rank slice: not an utterance
                continue
            boundary_seq = predictions["decoded_boundary_seq"][i]
            md_lbl_seq = predictions["decoded_plvl_md_lbl_seq"][i]
            n = len(boundary_seq)
            edges = torch.cat([torch.where(boundary_seq == 1)[0], torch.tensor([n])]) / n
            entries = []
            for k in torch.where(md_lbl_seq == 1)[0]:
                start, end = edges[k], edges[k + 1]
                if start * n == end * n:
                    warnings.warn(f"same start and end index: {int((start * n).item())}")
                    assert False
                entries.append([int(k.item()), start.item(), end.item()])
            results[utt_id] = entries
        if self._dp():  # gathered and written by rank 0 at the stage's end
            self._md_results.append((getattr(batch, "global_index", 0), results))
            return
        self._write_md_results(results)

    def _write_md_results(self, results):
        save_dir = Path("datasets") / self.hparams.dataset_name / "saved_md_results"
        save_dir.mkdir(parents=True, exist_ok=True)
        save_path = save_dir / f"{self.hparams.model_name}.json"
        if save_path.exists():
            with open(save_path) as f:
                merged = json.load(f)
            merged.update(results)
            results = merged
        with open(save_path, "w") as f:
            json.dump(results, f)
