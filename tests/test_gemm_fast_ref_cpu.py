"""The mlvae_gemm_bf16 test harness checks itself (no GPU): addr_gemm's explicit flat indexing over
place()d, NaN-poisoned buffers must equal ref_gemm on the logical operands exactly (integer-valued
operands: every sum is exact in fp64), so a wrong leading dimension, offset, batch stride or shift
rule in tests/gemm_fast_ref.py cannot hide behind the kernel tests that build on it."""
import numpy as np
import pytest
import torch

from gemm_fast_ref import SENTINEL, _shift_rows, addr_gemm, logical_index, logical_mask, place, ref_gemm

NAN = float("nan")
LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]


def _ints(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).float()


def _check(ta, tb, M, N, K, batch=1, pad_a=0, pad_b=0, pad_c=0, a_bs=None, shared_b=False, c_bs=None,
           guard=5, beta=0.0, epi=0, bias=False, T=0, kshift=0, kstep=0, seed=0):
    A = _ints(batch, *((K, M) if ta else (M, K)), seed=seed + 1)
    B = _ints(1 if shared_b else batch, *((N, K) if tb else (K, N)), seed=seed + 2)
    Cin = _ints(batch, M, N, seed=seed + 3)
    aux = _ints(M, N, seed=seed + 4)
    b1, b2 = (_ints(N, seed=seed + 5), _ints(N, seed=seed + 6)) if bias else (None, None)
    lda, ldb, ldc = A.shape[2] + pad_a, B.shape[2] + pad_b, N + pad_c
    a_bs = A.shape[1] * lda if a_bs is None else a_bs
    b_bs = 0 if shared_b else B.shape[1] * ldb
    c_bs = M * ldc if c_bs is None else c_bs
    Af, a0 = place(A, lda, guard, NAN, bstride=a_bs)
    Bf, b0 = place(B, ldb, guard, NAN, bstride=b_bs if not shared_b else None)
    Cf, c0 = place(Cin if beta != 0.0 else torch.full_like(Cin, SENTINEL), ldc, guard, SENTINEL, bstride=c_bs)
    auxf, aux0 = place(aux, N + 3, guard, NAN)
    b1f, b1_0 = place(b1, 0, guard, NAN) if bias else (None, 0)
    b2f, b2_0 = place(b2, 0, guard + 1, NAN) if bias else (None, 0)
    out = addr_gemm(ta, tb, M, N, K, batch, Af.numpy(), a0, lda, a_bs, Bf.numpy(), b0, ldb, b_bs, Cf.numpy(),
                    c0, ldc, c_bs, beta, None if b1f is None else b1f.numpy(), b1_0,
                    None if b2f is None else b2f.numpy(), b2_0, epi, auxf.numpy(), aux0, N + 3, T, kshift, kstep)
    ref = ref_gemm(ta, tb, A, B, b1, b2, beta, Cin, epi, aux, T, kshift, kstep)
    assert torch.isfinite(ref).all()
    out = torch.from_numpy(out)
    assert torch.isfinite(out).all(), "the emulation read a poisoned element"
    got = out[logical_index(c0, batch, M, N, ldc, c_bs)]
    assert torch.equal(got, ref)
    mask = logical_mask(out.numel(), c0, batch, M, N, ldc, c_bs)
    assert int(mask.sum()) == batch * M * N
    assert torch.equal(out[~mask], Cf.double()[~mask]), "the emulation wrote outside the logical C"


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("pad", [0, 3])
def test_layouts_and_padded_ld(ta, tb, pad):
    _check(ta, tb, 7, 5, 11, pad_a=pad, pad_b=2 * pad, pad_c=pad, seed=10 * ta + tb)
    _check(ta, tb, 24, 24, 24, batch=2, pad_a=pad, pad_b=pad, pad_c=1, bias=True, beta=0.5, epi=1, seed=3)
    _check(ta, tb, 3, 4, 6, batch=2, pad_a=pad, bias=True, beta=-2.0, epi=2, seed=4)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_batch_strides(ta, tb):
    rows, cols = (9, 6) if ta else (6, 9)                   # A entries: K = 9, M = 6
    one = rows * (cols + 2)
    _check(ta, tb, 6, 5, 9, batch=3, pad_a=2, shared_b=True, seed=5)           # b_bstride = 0
    _check(ta, tb, 6, 5, 9, batch=3, pad_a=2, a_bs=one + 7, seed=6)            # gaps between entries
    _check(ta, tb, 6, 5, 9, batch=3, pad_a=2, a_bs=-(one + 4), seed=7)         # entry 0 is the last matrix
    _check(ta, tb, 6, 5, 9, batch=3, pad_c=2, c_bs=6 * 7 + 5, seed=8)          # c_bstride > M * ldc


def test_negative_bstride_placement():
    A = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    flat, off = place(A, 5, 2, NAN, bstride=-20)
    assert off == 22 and flat.numel() == 2 * 2 + 20 + 2 * 5 + 4
    assert torch.equal(flat[off:off + 4], A[0, 0]) and torch.equal(flat[off - 20 + 5:off - 20 + 9], A[1, 1])
    assert int(torch.isnan(flat).sum()) == flat.numel() - A.numel()


@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("T", [3, 4, 5, 6])
@pytest.mark.parametrize("sh", [-2, -1, 1, 2])
def test_time_shift(ta, T, sh):
    _check(ta, 0, 5, 4, 4 * T, pad_b=2, T=T, kshift=sh, seed=T)
    _check(ta, 0, 5, 4, 3 * T, batch=2, pad_b=1, T=T, kshift=sh, kstep=-2 * sh, bias=True, seed=T + 1)


def test_shift_rule_by_hand():
    """T = 3, shift +1: rows 0 1 | 3 4 read rows 1 2 | 4 5; rows 2 and 5 (the last of a sequence) read
    zero -- never the first row of the next sequence."""
    b = torch.arange(1.0, 7.0).reshape(6, 1)
    assert _shift_rows(b, 3, 1).flatten().tolist() == [2, 3, 0, 5, 6, 0]
    assert _shift_rows(b, 3, -2).flatten().tolist() == [0, 0, 1, 0, 0, 4]


@pytest.mark.parametrize("side", ["a", "b"])
def test_overlapping_rows(side):
    """ld smaller than the row length: the flat data is the operand, the logical matrix its
    as_strided view (an overlapping window, as the wav2vec2 conv layers pass)."""
    M, N, K, ld, guard = 6, 8, 12, 4, 3
    if side == "a":    # A [M, K] k-contiguous, rows ld apart
        data = _ints((M - 1) * ld + K, seed=1)
        Af, a0 = place(data, 0, guard, NAN)
        A = torch.as_strided(data, (1, M, K), (0, ld, 1))
        B = _ints(1, K, N, seed=2)
        Bf, b0 = place(B, N, guard, NAN)
        args = (0, 0, M, N, K, 1, Af.numpy(), a0, ld, 0, Bf.numpy(), b0, N, 0)
        ref = ref_gemm(0, 0, A, B)
    else:              # B [K, N] n-contiguous, rows ld apart
        data = _ints((K - 1) * ld + N, seed=3)
        Bf, b0 = place(data, 0, guard, NAN)
        B = torch.as_strided(data, (1, K, N), (0, ld, 1))
        A = _ints(1, M, K, seed=4)
        Af, a0 = place(A, K, guard, NAN)
        args = (0, 0, M, N, K, 1, Af.numpy(), a0, K, 0, Bf.numpy(), b0, ld, 0)
        ref = ref_gemm(0, 0, A, B)
    Cf, c0 = place(torch.full((M, N), SENTINEL), N, guard, SENTINEL)
    out = torch.from_numpy(addr_gemm(*args, Cf.numpy(), c0, N, 0))
    assert torch.isfinite(out).all()
    assert torch.equal(out[c0:c0 + M * N].reshape(1, M, N), ref)


def test_k_zero_is_bias_plus_beta_c():
    _check(0, 1, 4, 5, 0, bias=True, beta=0.5, seed=9)


def test_poison_is_seen():
    """The finite-result assertion has teeth: an emulation that reads one element past a row of a
    padded operand picks the poison up."""
    A = _ints(1, 3, 4, seed=1)
    B = _ints(1, 4, 2, seed=2)
    Af, a0 = place(A, 6, 2, NAN)
    Bf, b0 = place(B, 2, 2, NAN)
    Cf, c0 = place(torch.zeros(3, 2), 2, 2, SENTINEL)
    out = addr_gemm(0, 0, 3, 2, 5, 1, Af.numpy(), a0, 6, 0, np.concatenate([Bf.numpy(), np.zeros(8)]), b0, 2, 0,
                    Cf.numpy(), c0, 2, 0)
    assert not np.isfinite(out[c0:c0 + 6]).all()
