"""Harness of the mlvae_gemm_bf16 edge tests (include/mlvae.h, csrc/gemm_fast.hip).

place()     embeds a logical matrix into a flat buffer with a leading dimension, batch stride,
            guards and poison, the way the production call sites hand slices of wider buffers over;
ref_gemm()  the fp64 result of the header's contract from the LOGICAL operands;
addr_gemm() the same contract by explicit flat indexing (NumPy) -- it checks the placement and
            stride arithmetic of this harness itself (tests/test_gemm_fast_ref_cpu.py);
run_gemm()  the ctypes launch with every leading dimension, offset and stride explicit.

Importing this module needs no GPU and no libmlvae.so (run_gemm binds the library when called).
"""
import numpy as np
import torch

SENTINEL = -24680.5  # finite prefill of every C element a launch must not write

EPI_NONE, EPI_LRELU, EPI_DLRELU, EPI_DROPOUT = 0, 1, 2, 3
EPI_OUT_F16, EPI_OUT_BF16 = 16, 32
SLOPE = float(np.float32(0.01))  # the kernels' fp32 LeakyReLU slope, as a double


def _shift_rows(b, T, shift):
    """rows k of B -> k + shift when 0 <= k % T + shift < T, else zero (the recurrent dW_hh)."""
    K = b.shape[0]
    t = torch.arange(K) % T + shift
    ok = (t >= 0) & (t < T)
    idx = torch.arange(K) + shift
    out = torch.zeros_like(b)
    out[ok] = b[idx[ok]]
    return out


def place(mat, ld, guard, poison, bstride=None):
    """Embed mat into a flat buffer of its dtype -> (flat, element offset of (0, 0) of entry 0).

    mat [rows, cols]: rows ld elements apart (ld >= cols); [batch, rows, cols]: entry z starts
    z * bstride elements after entry 0 (bstride may be negative: entry 0 is then the LAST matrix
    in memory; default one dense matrix, rows * ld).  A 1-D mat is flat data placed as it is: a
    bias, or an operand whose rows overlap (ld < cols), which the caller reads back by
    as_strided.  guard elements lie before and after; every element that belongs to no logical
    row is poison."""
    if mat.dim() == 1:
        flat = torch.full((2 * guard + mat.numel(),), poison, dtype=mat.dtype)
        flat[guard:guard + mat.numel()] = mat
        return flat, guard
    m3 = mat if mat.dim() == 3 else mat.unsqueeze(0)
    batch, rows, cols = m3.shape
    assert ld >= cols, "overlapping rows: pass the flat data as a 1-D tensor"
    one = (rows - 1) * ld + cols if rows else 0
    if bstride is None:
        bstride = rows * ld
    assert batch == 1 or abs(bstride) >= one, "batch entries would overlap"
    off = guard + (batch - 1) * max(-bstride, 0)
    flat = torch.full((2 * guard + (batch - 1) * abs(bstride) + one,), poison, dtype=mat.dtype)
    flat[logical_index(off, batch, rows, cols, ld, bstride)] = m3
    return flat, off


def logical_index(off, batch, rows, cols, ld, bstride):
    """int64 [batch, rows, cols]: the flat element index of every logical (z, row, col)."""
    z = torch.arange(batch).view(-1, 1, 1)
    r = torch.arange(rows).view(1, -1, 1)
    c = torch.arange(cols).view(1, 1, -1)
    return off + z * bstride + r * ld + c


def logical_mask(numel, off, batch, rows, cols, ld, bstride):
    """bool [numel]: the elements of a flat buffer that are logical (z, row, col) positions."""
    m = torch.zeros(numel, dtype=torch.bool)
    m[logical_index(off, batch, rows, cols, ld, bstride).reshape(-1)] = True
    return m


def ref_gemm(ta, tb, A, B, bias1=None, bias2=None, beta=0.0, Cin=None, epi=EPI_NONE, aux=None,
             T=0, kshift=0, kstep=0):
    """fp64 C [batch, M, N] of the header's contract from the logical operands.

    A [batch, K, M] if ta else [batch, M, K]; B [batch or 1, N, K] if tb else [batch or 1, K, N]
    (one entry: b_bstride = 0, shared by the batch).  Row k of B_z reads row k + sh_z when
    0 <= k % T + sh_z < T, else zero, sh_z = kshift + z * kstep.  aux [M, N] is shared by the
    batch.  Epilogues 1 (LeakyReLU 0.01) and 2 (times lrelu'(aux)); the dropout epilogue's mask is
    applied by the caller (tests/philox_np.py)."""
    batch = A.shape[0]
    out = []
    for z in range(batch):
        a = A[z].double().t() if ta else A[z].double()
        b = B[z if B.shape[0] > 1 else 0].double()
        b = b.t() if tb else b
        sh = kshift + z * kstep
        if sh != 0:
            assert not tb and T > 0
            b = _shift_rows(b, T, sh)
        r = a @ b
        if bias1 is not None:
            r = r + bias1.double()
        if bias2 is not None:
            r = r + bias2.double()
        if beta != 0.0:
            r = r + float(np.float32(beta)) * Cin[z].double()
        if epi == EPI_LRELU:
            r = torch.where(r > 0, r, SLOPE * r)
        elif epi == EPI_DLRELU:
            r = r * torch.where(aux > 0, 1.0, SLOPE).double()
        out.append(r)
    return torch.stack(out)


def addr_gemm(ta, tb, M, N, K, batch, A_flat, a0, lda, a_bs, B_flat, b0, ldb, b_bs, C_flat, c0, ldc,
              c_bs, beta=0.0, bias1=None, b1_0=0, bias2=None, b2_0=0, epi=EPI_NONE, aux=None, aux0=0,
              ldaux=0, T=0, kshift=0, kstep=0):
    """The contract by flat indexing: C_flat (float64 copy) with the logical elements replaced by
    C[z, m, n] = epi(sum_k A_flat[a0 + z a_bs + (k lda + m | m lda + k)] *
    B_flat[b0 + z b_bs + (n ldb + k | k' ldb + n)] + bias1[b1_0 + n] + bias2[b2_0 + n] +
    beta C_flat[c0 + z c_bs + m ldc + n]), k' = k + sh_z inside its length-T sequence (the product
    is dropped otherwise -- its B element is never read)."""
    Af = np.asarray(A_flat, dtype=np.float64)
    Bf = np.asarray(B_flat, dtype=np.float64)
    Cf = np.array(C_flat, dtype=np.float64)
    m = np.arange(M)[:, None, None]
    k = np.arange(K)[None, :, None]
    n = np.arange(N)[None, None, :]
    for z in range(batch):
        ia = a0 + z * a_bs + (k * lda + m if ta else m * lda + k)          # [M, K, 1]
        sh = kshift + z * kstep
        ok = np.ones((1, K, 1), dtype=bool)
        kb = k
        if sh != 0:
            t = k % T + sh
            ok = (t >= 0) & (t < T)
            kb = np.where(ok, k + sh, k)                                       # a row that exists
        ib = b0 + z * b_bs + (n * ldb + kb if tb else kb * ldb + n)         # [1, K, N]
        prod = np.where(ok, Af[ia] * Bf[ib], 0.0) if K else np.zeros((M, 0, N))
        r = prod.sum(axis=1)                                                  # [M, N]
        mm, nn = np.arange(M)[:, None], np.arange(N)[None, :]
        if bias1 is not None:
            r = r + np.asarray(bias1, dtype=np.float64)[b1_0 + nn]
        if bias2 is not None:
            r = r + np.asarray(bias2, dtype=np.float64)[b2_0 + nn]
        ic = c0 + z * c_bs + mm * ldc + nn
        if beta != 0.0:
            r = r + float(np.float32(beta)) * Cf[ic]
        if epi == EPI_LRELU:
            r = np.where(r > 0, r, SLOPE * r)
        elif epi == EPI_DLRELU:
            r = r * np.where(np.asarray(aux, dtype=np.float64)[aux0 + mm * ldaux + nn] > 0, 1.0, SLOPE)
        Cf[ic] = r
    return Cf


def _ptr(t, off=0):
    return t.data_ptr() + off * t.element_size() if t is not None else None


def run_gemm(ta, tb, M, N, K, batch, A, a0, lda, a_bs, B, b0, ldb, b_bs, C, c0, ldc, c_bs, beta=0.0,
             bias1=None, b1_0=0, bias2=None, b2_0=0, epi=EPI_NONE, aux=None, aux0=0, ldaux=0, T=0,
             kshift=0, kstep=0, seed=0, drop_offset=0, p=0.0, ws="auto", ws_bytes=None):
    """Launch mlvae_gemm_bf16 on flat device tensors (offsets in elements of each tensor) and
    return (rc, the whole flat C on the host, the workspace tensor or None).  ws "auto": a
    workspace of mlvae_gemm_bf16_workspace_size bytes prefilled with SENTINEL (a launch that must
    not split leaves it untouched); None: no workspace; a tensor: used as given, with ws_bytes
    (default its size)."""
    from mlvae_hip._lib import lib
    l = lib()
    if isinstance(ws, str):
        need = l.mlvae_gemm_bf16_workspace_size(M, N, K, batch)
        ws = torch.full((need // 4 + 4,), SENTINEL, device="cuda")
        if ws_bytes is None:
            ws_bytes = need
    elif ws is not None and ws_bytes is None:
        ws_bytes = ws.numel() * 4
    rc = l.mlvae_gemm_bf16(ta, tb, M, N, K, batch, _ptr(A, a0), lda, a_bs, _ptr(B, b0), ldb, b_bs,
                           _ptr(C, c0), ldc, c_bs, beta, _ptr(bias1, b1_0), _ptr(bias2, b2_0), epi,
                           _ptr(aux, aux0), ldaux, T, kshift, kstep, seed, drop_offset, p, _ptr(ws),
                           ws_bytes or 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, C.cpu(), ws
