"""Shared state and helpers of the operator layer: the matrix products' precision, the data-parallel
shard context, pointer / workspace helpers, the per-device int32 words and the GEMM / column-sum
launches.  _state and _ws are created here once and never rebound: every family module sees the
same objects."""
import ctypes

import torch

from .._lib import check, lib
from . import errors

PREC = {"fp32": 0, "bf16": 1}
_state = {"prec": "fp32"}
_ws = {}


def set_precision(prec):
    """Operand precision of the matrix products: "fp32" (exact f32 MFMA) or "bf16"."""
    if prec not in PREC:
        raise ValueError(f"precision must be one of {list(PREC)}")
    _state["prec"] = prec


def get_precision():
    return _state["prec"]


class precision:
    """Context: matrix-product operand precision inside the block (the mixed-precision region of
    MDModel.fit_batch's auto_mix_prec branch; backward runs inside it too, since the HIP ops read
    the precision when they launch)."""

    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        self.prev = get_precision()
        set_precision(self.prec)
        return self

    def __exit__(self, *exc):
        set_precision(self.prev)


def _prec():
    return PREC[_state["prec"]]


class shard:
    """Context: the batch inside the block is a data-parallel shard of a global batch of
    B_global utterances, its first utterance at utt_offset.  Every drawing op (randn, the LSTM's
    inter-layer dropout, boundary_heads, pi_sample, pi_sample_k, GmmLatentFn, HvaeLatentFn) then draws, for
    each of its utterances, bit for bit what the single process draws for that utterance of the
    global batch (include/mlvae.h, "the random streams over an utterance map"): the ops take the
    seeds from torch's CPU generator as they always do, so ranks seeded alike that make the same
    calls in the same order agree.  Backward passes that recompute a draw (dropout, the boundary
    draws) use the map of their forward.  global_lens = the relative lengths [B_global] of the
    global batch: masked_mean's default global denominator inside the block.  folded(K) is the
    context of MD_VAE_sfl's K-folded batch [K * B_local, T, .] (draw k of utterance b at row
    k * B_local + b).  Without a context the ops call what they always called."""

    def __init__(self, utt_offset, B_global, global_lens=None, K=1):
        if utt_offset < 0 or B_global < 1 or K < 1:
            raise ValueError(f"shard: utt_offset {utt_offset}, B_global {B_global}, K {K}")
        self.utt_offset, self.B_global, self.K = int(utt_offset), int(B_global), int(K)
        self.global_lens = global_lens

    def folded(self, K):
        return shard(self.utt_offset, self.B_global, self.global_lens, K)

    def map(self, B):
        """The ABI's (utt_offset, seg_utts, seg_stride, total_utts) for a batch of B rows."""
        if B % self.K:
            raise ValueError(f"shard: {B} rows are not {self.K} folds of a local batch")
        Bl = max(B // self.K, 1)
        # rows past B_global are the fillers of a short slice: masked out by their zero lengths
        return (ctypes.c_longlong * 4)(self.utt_offset, Bl, self.B_global, self.K * self.B_global)

    def global_frames(self, T):
        """Valid frames of the global batch padded to T (the masked means' global count)."""
        if self.global_lens is None:
            return None
        return valid_frames(self.global_lens, T)

    def __enter__(self):
        self.prev = _state.get("shard")
        _state["shard"] = self
        return self

    def __exit__(self, *exc):
        _state["shard"] = self.prev


def current_shard():
    return _state.get("shard")


def valid_frames(lens, T):
    """Frames the masked means count for relative lengths `lens` at padded length T: frame t is
    valid iff (float)t < fp32(len * T) (csrc/common.h valid_frames), summed over the utterances."""
    lim = torch.as_tensor(lens, dtype=torch.float32).cpu() * float(T)
    c = torch.where(lim > 0, torch.ceil(lim).clamp(max=float(T)), torch.zeros_like(lim))
    return int(c.sum().item())


def _bt(shape, what):
    """(B, T, C) of a [B, T, ...] batch: what the mapped streams index."""
    if len(shape) < 2:
        raise ValueError(f"{what}: a sharded draw needs a [B, T, ...] batch, got {tuple(shape)}")
    C = 1
    for d in shape[2:]:
        C *= int(d)
    return int(shape[0]), int(shape[1]), C


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t, off=0):
    return t.data_ptr() + 4 * off


def _need(t, name):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise TypeError(f"{name}: expected a float32 HIP tensor, got {t.dtype} on {t.device} "
                        "(the HIP path has no CPU fallback)")
    return t.contiguous()


def _ws_bytes(ws):
    return ws.numel() * ws.element_size()


def _workspace(nbytes, key="gemm"):
    dev = torch.cuda.current_device()
    w = _ws.get((dev, key))
    if w is None or _ws_bytes(w) < nbytes:
        w = torch.empty(max(nbytes // 4 + 1, 1024), device="cuda", dtype=torch.float32)
        _ws[(dev, key)] = w
    return w


def _dev_word(key):
    """One zeroed int32 word per device, kept for the process: what the kernels OR error bits into."""
    dev = torch.cuda.current_device()
    e = _ws.get((dev, key))
    if e is None:
        e = torch.zeros(1, device="cuda", dtype=torch.int32)
        _ws[(dev, key)] = e
    return e


def _md_err():
    """The shared device error word (errors.ERR names its bits)."""
    return _dev_word("md_err")


def raise_err(err, domain, who=None):
    """Read the word `err` as `domain` does (one host sync): raise what errors.read says, after
    clearing the domain's bits alone."""
    exc, clear = errors.read(int(err.item()), domain, who)
    if exc is not None:
        err.bitwise_and_(~clear)
        raise exc


def gemm(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias1=None, bias2=None, epi=0, aux=None,
         ldaux=0, beta=0.0, kshift_T=0, kshift=0):
    """C = epi(op(A) op(B) + bias1 + bias2 + beta*C) on raw device pointers (ints)."""
    l = lib()
    ws = _workspace(l.mlvae_gemm_workspace_size(M, N, K))
    check(l.mlvae_gemm(_prec(), ta, tb, M, N, K, 1.0, A, lda, B, ldb, beta, C, ldc, bias1, bias2,
                       epi, aux, ldaux, kshift_T, kshift, _p(ws), _ws_bytes(ws), _stream()),
          "mlvae_gemm")


def colsum(N, Cn, src, ld, out, out2=None, beta=0.0):
    l = lib()
    ws = _workspace(l.mlvae_colsum_workspace_size(N, Cn), "colsum")
    check(l.mlvae_colsum(N, Cn, src, ld, out, out2, beta, _p(ws), _ws_bytes(ws), _stream()),
          "mlvae_colsum")


def _rows(x):
    return x.numel() // x.shape[-1]


def _score_lens(lens, B, dev, what):
    if tuple(lens.shape) != (B,):
        raise ValueError(f"{what}: lengths must be [{B}], got {tuple(lens.shape)}")
    return _need(lens.to(dev, torch.float32), f"{what} lengths")
