"""mlvae_gemm_bf16 (csrc/gemm_fast.hip) where the production call sites differ from the plain unit
tests: leading dimensions and batch strides that are not the matrix extent, ragged and odd
extents, every K-tile count of every main-loop variant, the grouped tile walk's tail group, both
time-shift wraps, split-K through the reduce's epilogues, 16-bit C, the epilogue path selection
and the dropout mask index -- against tests/gemm_fast_ref.py's fp64 contract.

Every launch (case()): bf16 randn operands place()d between NaN poison with 4096-element guards
(an over-read makes the result non-finite), C prefilled with a sentinel that must survive
bit-identically outside the logical [M, N] region, result finite and rel_err < 1e-5 (the bound
of tests/test_gpu_gemm_fast.py, same kernel, K up to 8000).  Cases that must (not) split assert
the planner's workspace size first."""
import contextlib

import numpy as np
import pytest
import torch

from gemm_fast_ref import (EPI_DLRELU, EPI_DROPOUT, EPI_LRELU, EPI_NONE, EPI_OUT_BF16, EPI_OUT_F16, SENTINEL,
                           logical_index, logical_mask, place, ref_gemm, run_gemm)
from gpu_utils import need_gpu, rel_err
from philox_np import dropout_mask

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 4096                       # guard elements (a multiple of 8: 16-byte aligned bases)
LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]
M0, N0 = 264, 136              # 2 x 1 tiles, ragged in both dimensions
TOL = 1e-5
CDT = {0: torch.float32, EPI_OUT_F16: torch.float16, EPI_OUT_BF16: torch.bfloat16}


def _lib():
    from mlvae_hip._lib import lib
    return lib()


def _last_error():
    from mlvae_hip._lib import last_error
    return last_error()


@contextlib.contextmanager
def planner(variant=0, split_target=None):
    """Set the main-loop variant / split-K target for the launches inside; restore both after."""
    l = _lib()
    pv, pt = l.mlvae_gemm_bf16_set_variant(-1), l.mlvae_gemm_bf16_set_split_target(0)
    try:
        l.mlvae_gemm_bf16_set_variant(variant)
        if split_target is not None:
            l.mlvae_gemm_bf16_set_split_target(split_target)
        yield
    finally:
        l.mlvae_gemm_bf16_set_variant(pv)
        l.mlvae_gemm_bf16_set_split_target(pt)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Res:
    pass


def case(ta, tb, M, N, K, batch=1, pad_a=8, pad_b=8, lda_over=0, ldb_over=0, ldc=None, c_shift=0, a_gap=0,
         neg_a=False, shared_b=False, c_gap=0, bias=True, bias_shift=0, beta=0.0, epi=EPI_NONE, out=0,
         ldaux=None, T=0, kshift=0, kstep=0, drop=None, ws="auto", ws_short=False, split=None, ints=False,
         seed=0, expect_fail=False, check=True):
    """One launch under the file's rules -> Res (C logical, fp64 ref, rc, flat buffers).
    The operands depend only on (ta, tb, M, N, K, batch, shared_b, ints, seed, lda_over, ldb_over),
    so two calls that differ in the C layout, the epilogue or the bias alignment see the same data.
    drop = (seed, offset, p) with the dropout epilogue; expect_fail: the call must be refused and
    leave C untouched."""
    need_gpu()
    l = _lib()
    torch.manual_seed(1000003 * seed + M + 3 * N + 7 * K + 11 * ta + 13 * tb + 17 * batch)

    def gen(*shape):
        return (torch.randint(-3, 4, shape).float() if ints else torch.randn(*shape)).to(torch.bfloat16)

    def operand(nb, rows, cols, pad, over, gap, neg):
        if over:  # overlapping rows: the flat data is the operand
            data = gen((rows - 1) * over + cols)
            flat, off = place(data, 0, G, NAN)
            return torch.as_strided(data, (1, rows, cols), (0, over, 1)), flat, off, over, 0
        ld = cols + pad
        bs = (rows * ld + gap) * (-1 if neg else 1)
        logical = gen(nb, rows, cols)
        flat, off = place(logical, ld, G, NAN, bstride=bs)
        return logical, flat, off, ld, bs

    A, Af, a0, lda, a_bs = operand(batch, *((K, M) if ta else (M, K)), pad_a, lda_over, a_gap, neg_a)
    B, Bf, b0, ldb, b_bs = operand(1 if shared_b else batch, *((N, K) if tb else (K, N)), pad_b, ldb_over, 0, False)
    if shared_b or batch == 1:
        b_bs = 0
    if batch == 1:
        a_bs = 0
    b1, b2 = (gen(N).float(), gen(N).float()) if bias else (None, None)
    aux = torch.randn(M, N)
    Cin = gen(batch, M, N).float() if ints else torch.randn(batch, M, N)
    ldc = N if ldc is None else ldc
    c_bs = M * ldc + c_gap
    cdt = CDT[out]
    inside = Cin if beta != 0.0 else torch.full((batch, M, N), SENTINEL)
    Cf, c0 = place(inside.to(cdt), ldc, G + c_shift, SENTINEL, bstride=c_bs) if ldc >= N else (None, 0)
    if Cf is None:  # (refusal cases only) an ldc below N: a plain sentinel buffer
        Cf, c0 = torch.full((2 * G + batch * M * N,), SENTINEL, dtype=cdt), G + c_shift
    b1f, b1_0 = place(b1, 0, G + bias_shift, NAN) if bias else (None, 0)
    b2f, b2_0 = place(b2, 0, G, NAN) if bias else (None, 0)
    ldaux = N if ldaux is None else ldaux
    auxf, aux0 = place(aux, ldaux, G, NAN)

    need = l.mlvae_gemm_bf16_workspace_size(M, N, K, batch)
    if split is True:
        assert need > 0, "this case is meant to split K"
    elif split is False:
        assert need == 0, "this case is meant to run in one split"
    if ws_short:
        ws, ws_bytes = torch.full((need // 4 + 4,), SENTINEL, device="cuda"), need - 1
    else:
        ws_bytes = None
    dseed, doff, p = drop if drop else (0, 0, 0.0)
    dev = [t.cuda() if t is not None else None for t in (Af, Bf, Cf, b1f, b2f, auxf)]
    rc, flat, wsd = run_gemm(ta, tb, M, N, K, batch, dev[0], a0, lda, a_bs, dev[1], b0, ldb, b_bs, dev[2], c0, ldc,
                             c_bs, beta, dev[3], b1_0, dev[4], b2_0, epi | out, dev[5] if epi == EPI_DLRELU else None,
                             aux0, ldaux, T, kshift, kstep, dseed, doff, p, ws, ws_bytes)
    r = Res()
    r.rc, r.flat, r.prefill, r.ws, r.need, r.ldc = rc, flat, Cf, wsd, need, ldc
    if expect_fail:
        assert rc != 0, "the call must be refused"
        assert _last_error(), "a refusal sets mlvae_last_error()"
        assert torch.equal(_bits(flat), _bits(Cf)), "a refused call wrote to C"
        return r
    assert rc == 0, _last_error()
    mask = logical_mask(flat.numel(), c0, batch, M, N, ldc, c_bs)
    assert torch.equal(_bits(flat)[~mask], _bits(Cf)[~mask]), "C written outside its logical region"
    r.C = flat[logical_index(c0, batch, M, N, ldc, c_bs)]
    assert torch.isfinite(r.C).all(), "non-finite result: a poisoned (out-of-range) element was read"
    ref = ref_gemm(ta, tb, A, B, b1, b2, beta, Cin, epi, aux, T, kshift, kstep)
    if drop:  # the mask of element offset + row * ldc + col, the same for every batch entry
        mk = dropout_mask(dseed, doff + M * ldc, p)[doff:].reshape(M, ldc)[:, :N]
        r.mask = torch.from_numpy(mk.copy())
        ref = ref * r.mask.double()
    r.ref = ref
    if check and out == 0:
        if ints:
            assert torch.equal(r.C.double(), ref)
        else:
            err = rel_err(r.C, ref)
            assert err < TOL, err
    return r


def ws_untouched(r):
    return r.ws is None or bool((r.ws == SENTINEL).all())


# ---- a. strides and bounds

@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("K", [72, 200])
def test_padded_ld_and_c_layout(ta, tb, K):
    """lda / ldb = extent + 8 and + 24; ldc N (staged), N + 4 (staged), N + 1 (direct); C base on a
    16-byte boundary and one float off it (direct)."""
    for pad in (8, 24):
        for ldc in (N0, N0 + 4, N0 + 1):
            for c_shift in (0, 1):
                case(ta, tb, M0, N0, K, pad_a=pad, pad_b=pad, ldc=ldc, c_shift=c_shift, split=False)


def test_overlapping_rows():
    """ld below the row length (overlapping windows, as the wav2vec2 conv layers pass)."""
    case(0, 1, M0, N0, 48, lda_over=16, split=False)
    case(0, 0, M0, N0, 48, lda_over=16, split=False)
    case(0, 0, M0, N0, 72, ldb_over=N0 - 8, split=False)
    case(1, 0, M0, N0, 72, ldb_over=N0 - 8, split=False)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_batch_strides(ta, tb):
    case(ta, tb, M0, N0, 72, batch=3, shared_b=True, split=False)            # b_bstride = 0
    case(ta, tb, M0, N0, 72, batch=3, a_gap=1024 + 8, split=False)           # gaps between the A entries
    case(ta, tb, M0, N0, 72, batch=3, ldc=N0 + 4, c_gap=36, split=False)     # c_bstride > M * ldc
    case(ta, tb, M0, N0, 72, batch=3, neg_a=True, a_gap=40, split=False)     # A points at the last matrix


# ---- b. extents

@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("M", [1, 7, 257])
def test_any_m(tb, M):
    case(0, tb, M, N0, 72, split=False)


@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("N", [1, 129, 130, 134])
def test_any_n(ta, N):
    """N odd / not a multiple of 4: the direct epilogue's scalar tail."""
    case(ta, 1, M0, N, 72, split=False)
    case(ta, 1, M0, N, 72, ldc=N + 3, beta=0.5, epi=EPI_LRELU, split=False)


@pytest.mark.parametrize("K", [1, 63, 65, 203])
def test_any_k(K):
    case(1, 0, M0, N0, K, split=False)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_k_zero(ta, tb):
    """K = 0: C = bias1 + bias2 + beta C."""
    case(ta, tb, M0, N0, 0, split=False)
    r = case(ta, tb, M0, N0, 0, beta=0.5, ldc=N0 + 4, split=False)
    assert rel_err(r.C, r.ref) < TOL


def test_empty_output():
    """M = 0 or N = 0: status 0, nothing written."""
    need_gpu()
    l = _lib()
    C = torch.full((1024,), SENTINEL, device="cuda")
    A = torch.zeros(4096, dtype=torch.bfloat16, device="cuda")
    for M, N in ((0, 136), (264, 0), (0, 0)):
        rc = l.mlvae_gemm_bf16(0, 1, M, N, 72, 1, A.data_ptr(), 72, 0, A.data_ptr(), 72, 0, C.data_ptr(), 136, 0, 0.0,
                               None, None, 0, None, 0, 0, 0, 0, 0, 0, 0.0, None, 0,
                               torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        assert bool((C == SENTINEL).all())


# ---- c. K-tile counts of every main loop

KTILES = [8, 32, 40, 64, 72, 96, 128, 136, 192, 200, 264, 320, 328]


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("variant", [0, 4, 5, 12, 16, 18])
def test_k_tile_counts(ta, tb, variant):
    """1 to 6 K-tiles of 64 (2 to 11 steps of the 32-deep ring), whole and ragged, through the
    default main loop of the layout and the A/B variants the timing tools select."""
    with planner(variant=variant):
        for K in KTILES:
            try:
                case(ta, tb, M0, N0, K, split=False)
            except AssertionError as e:
                raise AssertionError(f"K = {K}: {e}") from e


# ---- d. tile walk

@pytest.mark.parametrize("M,N,K,batch", [(2312, 264, 64, 1), (4360, 520, 8, 1), (776, 264, 64, 3),
                                         (520, 264, 64, 3)])
def test_tile_walk_is_a_bijection(M, N, K, batch):
    """TM = 10 / 18 (groups of 8 M-panels with a tail group of 2) and the batched flat
    (batch, tile) walk of 24 and of 18 workgroups (18: not a multiple of the 8 XCDs): every tile
    written once.  Small-integer operands: the fp32 sums are exact, so the result equals the fp64
    reference bit for bit."""
    for ta, tb in ((0, 1), (1, 0)):
        case(ta, tb, M, N, K, batch=batch, ints=True, split=False)


# ---- e. time shift

def _lcm8(T):
    return T * 8 // np.gcd(T, 8)


def _shift_k(ta, T, long):
    """K = a multiple of T the layout accepts (trans_a = 0 needs K % 8 == 0).  Short: 5 T, or with
    trans_a = 0 the first multiple of lcm(T, 8) at or above it that stays below the split
    threshold (T = 130: 520 = 4 T); long: the smallest such multiple >= 2048."""
    step = T if ta else _lcm8(T)
    if long:
        return -(-2048 // step) * step
    k = -(-5 * T // step) * step
    return k if k < 1024 else step


@pytest.mark.parametrize("ta", [1, 0])
@pytest.mark.parametrize("T", [25, 40, 64, 100, 130])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("long", [False, True])
def test_time_shift(ta, T, batch, long):
    """T below and at / above the staged image depth (64 with m-contiguous A, 32 behind a
    k-contiguous A): the per-lane modulo and the single unsigned-min wrap; sequence boundaries
    inside K-tiles; unsplit and split; batch 2 shifts the second entry the other way."""
    K = _shift_k(ta, T, long)
    assert K % T == 0
    for sh in (-1, 1, -3, 3):
        try:
            case(ta, 0, M0, N0, K, batch=batch, bias=False, T=T, kshift=sh, kstep=-2 * sh if batch == 2 else 0,
                 split=long)
        except AssertionError as e:
            raise AssertionError(f"shift {sh}, K = {K}: {e}") from e


@pytest.mark.parametrize("ta", [1, 0])
@pytest.mark.parametrize("variant", [4, 5, 12, 16, 18])
def test_time_shift_variants(ta, variant):
    """The A/B variants on a shifted B: m-contiguous A and B under VAR 12 stage B through
    McLanes::stage_any at depth 32; 16 and 18 fall back to the layout's shifted default."""
    with planner(variant=variant):
        for T in (25, 40, 100):
            for sh in (-1, 3):
                try:
                    case(ta, 0, M0, N0, _shift_k(ta, T, False), batch=2, bias=False, T=T, kshift=sh, kstep=-2 * sh,
                         split=False)
                except AssertionError as e:
                    raise AssertionError(f"T = {T}, shift {sh}: {e}") from e


def test_time_shift_refusals():
    case(0, 1, M0, N0, 200, T=25, kshift=1, expect_fail=True)     # trans_b = 1
    case(1, 1, M0, N0, 200, T=25, kshift=0, kstep=1, batch=2, expect_fail=True)
    case(1, 0, M0, N0, 200, T=0, kshift=1, expect_fail=True)      # T <= 0
    case(1, 0, M0, N0, 200, T=-5, kshift=-1, expect_fail=True)


# ---- f. split-K

SPLIT_CFG = {
    "biases": dict(),
    "beta": dict(beta=0.5, ldc=N0 + 4),
    "lrelu": dict(epi=EPI_LRELU),
    "dlrelu": dict(epi=EPI_DLRELU, ldaux=N0 + 8, beta=0.5),
    "batch2": dict(batch=2, ldc=N0 + 4, c_gap=20),
    "odd_ldc": dict(ldc=N0 + 1, c_shift=1, epi=EPI_LRELU),
}


@pytest.mark.parametrize("K", [1032, 2056, 8000])
@pytest.mark.parametrize("cfg", sorted(SPLIT_CFG))
def test_split_k_reduce_epilogues(K, cfg):
    """splitk_reduce_fast applies both biases, beta, the epilogues and the C layout."""
    case(1, 0, M0, N0, K, split=True, **SPLIT_CFG[cfg])
    case(0, 1, M0, N0, K, split=True, **SPLIT_CFG[cfg])


@pytest.mark.parametrize("K", [1032, 2056, 8000])
def test_split_target(K):
    """The engine's lowered target still splits; a target of 1 workgroup does not."""
    with planner(split_target=128):
        case(1, 0, M0, N0, K, split=True)
    with planner(split_target=1):
        r = case(1, 0, M0, N0, K, split=False)
        assert ws_untouched(r)


@pytest.mark.parametrize("K", [1032, 2056, 8000])
def test_split_fallbacks(K):
    """One split when the partial slabs cannot be used: N % 4 != 0, no workspace, a workspace
    one byte short.  The workspace stays untouched."""
    r = case(0, 1, M0, 134, K)
    assert r.need > 0 and ws_untouched(r)
    case(1, 0, M0, N0, K, ws=None, split=True)
    r = case(1, 0, M0, N0, K, ws_short=True, split=True)
    assert ws_untouched(r)
    r = case(1, 0, M0, N0, K, split=True)                         # (and with it, the slabs are used)
    assert not ws_untouched(r)


# ---- g. 16-bit C

@pytest.mark.parametrize("N", [136, 132])
@pytest.mark.parametrize("out,epi", [(EPI_OUT_BF16, EPI_NONE), (EPI_OUT_BF16, EPI_LRELU), (EPI_OUT_BF16, EPI_DROPOUT),
                                     (EPI_OUT_F16, EPI_NONE), (EPI_OUT_F16, EPI_DROPOUT)])
def test_c16(N, out, epi):
    """bf16 / fp16 C = the fp32-C result of the same call (itself within 1e-5 of fp64) rounded
    once, through the 8-column (N and ldc % 8 == 0) and the 4-column stores, unsplit and split,
    single and batched; the padding of the 16-bit buffer untouched (case())."""
    drop = (977, 4096, 0.25) if epi == EPI_DROPOUT else None
    runs = [dict(K=K, ldc=ldc) for K in (200, 2056) for ldc in (N, N + 8, N + 4)]
    runs += [dict(K=K, ldc=N + 8, batch=2, c_gap=16) for K in (200, 2056)]
    for kw in runs:
        kw = dict(kw, split=kw["K"] > 1024, epi=epi, drop=drop)
        K = kw.pop("K")
        r32 = case(0, 1, M0, N, K, **kw)                              # pinned to fp64 inside
        r16 = case(0, 1, M0, N, K, out=out, **kw)
        assert torch.equal(_bits(r16.C), _bits(r32.C.to(CDT[out]))), (K, kw)


def test_c16_refusals():
    for out in (EPI_OUT_BF16, EPI_OUT_F16):
        case(0, 1, M0, N0, 200, out=out, beta=0.5, expect_fail=True)
        case(0, 1, M0, 134, 200, out=out, ldc=136, expect_fail=True)         # N % 4
        case(0, 1, M0, N0, 200, out=out, ldc=N0 + 2, expect_fail=True)       # ldc % 4
        case(0, 1, M0, N0, 200, out=out, c_shift=4, expect_fail=True)        # C 8 bytes off
        case(0, 1, M0, N0, 200, out=out, bias_shift=1, expect_fail=True)     # bias1 4 bytes off
        case(0, 1, M0, N0, 200, out=out, batch=2, c_gap=4, expect_fail=True)  # c_bstride % 8
    case(0, 1, M0, N0, 200, out=EPI_OUT_BF16, epi=EPI_DLRELU, expect_fail=True)
    case(0, 1, M0, N0, 200, out=EPI_OUT_F16, epi=EPI_LRELU, expect_fail=True)


# ---- h. epilogue path selection

@pytest.mark.parametrize("epi", [EPI_NONE, EPI_LRELU, EPI_DROPOUT])
@pytest.mark.parametrize("K", [200, 2056])
def test_direct_epilogue_equals_staged(epi, K):
    """An unaligned bias pointer or an odd ldc sends an unsplit launch down the direct epilogue
    (a split one through the scalar reduce either way): bit-identical to the staged run, each
    within 1e-5 of fp64.  (The dropout mask index depends on ldc: its odd-ldc run is pinned to
    the reference alone.)"""
    drop = (31337, 8192, 0.2) if epi == EPI_DROPOUT else None
    kw = dict(epi=epi, drop=drop, split=K > 1024)
    staged = case(0, 1, M0, N0, K, **kw)
    off_bias = case(0, 1, M0, N0, K, bias_shift=1, **kw)
    assert torch.equal(_bits(staged.C), _bits(off_bias.C))
    odd = case(0, 1, M0, N0, K, ldc=N0 + 1, **kw)
    if epi != EPI_DROPOUT:
        assert torch.equal(_bits(staged.C), _bits(odd.C))


# ---- i. dropout mask index

DROP_PATHS = {
    "f32_staged": dict(N=N0, ldc=N0 + 4),
    "f32_direct_quads": dict(N=N0, ldc=N0 + 4, bias_shift=1),
    "f32_direct_tail": dict(N=134, ldc=N0 + 4),
    "bf16_w8": dict(N=N0, ldc=N0 + 8, out=EPI_OUT_BF16),
    "bf16_4col": dict(N=N0, ldc=N0 + 4, out=EPI_OUT_BF16),
    "f16_4col": dict(N=132, ldc=N0 + 4, out=EPI_OUT_F16),
}


@pytest.mark.parametrize("path", sorted(DROP_PATHS))
@pytest.mark.parametrize("doff", [0, 4096])
def test_dropout_index(path, doff):
    """The mask element of C[row, col] is drop_offset + row * ldc + col (tests/philox_np.py), on
    every store path: the dropout run equals the plain run times the mask, exactly."""
    kw = dict(DROP_PATHS[path])
    N, out = kw.pop("N"), kw.pop("out", 0)
    plain = case(0, 1, M0, N, 200, split=False, **kw)
    dropped = case(0, 1, M0, N, 200, split=False, epi=EPI_DROPOUT, drop=(4242, doff, 0.15), out=out, **kw)
    kept = float((dropped.mask != 0).float().mean())
    assert 0.8 < kept < 0.9, kept
    want = (plain.C * dropped.mask).to(CDT[out])
    assert torch.equal(_bits(dropped.C), _bits(want))


def test_dropout_mask_matches_dropout_kernel():
    """philox_np's mask at an offset = mlvae_dropout_ex's on device."""
    need_gpu()
    from mlvae_hip._lib import check
    n, off, seed, p = 5000, 4096, 4242, 0.15
    x = torch.ones(n, device="cuda")
    y = torch.empty(n, device="cuda")
    check(_lib().mlvae_dropout_ex(n, x.data_ptr(), y.data_ptr(), None, None, seed, off, p,
                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy(), dropout_mask(seed, off + n, p)[off:])


@pytest.mark.parametrize("doff", [4098, 4099])
def test_dropout_offset_must_be_a_multiple_of_4(doff):
    """The vector epilogues take one mask quad per 4 columns: any other offset is refused."""
    for kw in DROP_PATHS.values():
        kw = dict(kw)
        N, out = kw.pop("N"), kw.pop("out", 0)
        case(0, 1, M0, N, 200, epi=EPI_DROPOUT, drop=(4242, doff, 0.15), out=out, expect_fail=True, **kw)
    case(0, 1, M0, N0, 200, epi=EPI_NONE, drop=(0, doff, 0.0), split=False)  # ignored without the epilogue


def test_fp8_gemm_refuses_unaligned_drop_offset():
    """mlvae_gemm_fp8_ex shares the epilogue: the same refusal, and an aligned offset is accepted."""
    need_gpu()
    l = _lib()
    M, N, K = 64, 64, 128
    A = torch.zeros(M * K, dtype=torch.uint8, device="cuda")      # e4m3 zeros
    alpha = torch.ones(1, device="cuda")
    C = torch.full((M * N,), SENTINEL, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for doff in (4098, 4099):
        rc = l.mlvae_gemm_fp8_ex(M, N, K, A.data_ptr(), K, A.data_ptr(), K, C.data_ptr(), N, alpha.data_ptr(), None,
                                 None, EPI_DROPOUT, 7, doff, 0.15, st)
        assert rc != 0 and "drop_offset" in _last_error()
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all())
    rc = l.mlvae_gemm_fp8_ex(M, N, K, A.data_ptr(), K, A.data_ptr(), K, C.data_ptr(), N, alpha.data_ptr(), None, None,
                             EPI_DROPOUT, 7, 4096, 0.15, st)
    torch.cuda.synchronize()
    assert rc == 0, _last_error()
    assert bool((C == 0).all())


# ---- j. argument refusals (before any launch)

def test_argument_refusals():
    need_gpu()
    l = _lib()
    A = torch.zeros(1 << 16, dtype=torch.bfloat16, device="cuda")
    C = torch.full((1 << 16,), SENTINEL, device="cuda")
    aux = torch.zeros(1 << 16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    a, c = A.data_ptr(), C.data_ptr()

    def call(ta=0, tb=1, M=64, N=64, K=64, batch=1, A=a, lda=64, a_bs=0, B=a, ldb=64, b_bs=0, ldc=64, epi=0,
             aux=None, p=0.0):
        return l.mlvae_gemm_bf16(ta, tb, M, N, K, batch, A, lda, a_bs, B, ldb, b_bs, c, ldc, 0, 0.0, None, None,
                                 epi, aux, 64, 0, 0, 0, 1, 0, p, None, 0, st)

    bad = {
        "lda % 8": dict(lda=68),
        "ldb % 8": dict(ldb=68),
        "A base off 16 bytes": dict(A=a + 2),
        "B base off 16 bytes": dict(B=a + 8),
        "contiguous K % 8": dict(K=60),
        "contiguous M % 8 (trans_a)": dict(ta=1, M=60),
        "contiguous N % 8 (trans_b = 0)": dict(tb=0, N=60),
        "a_bstride % 8": dict(batch=2, a_bs=4100),
        "b_bstride % 8": dict(batch=2, b_bs=4100),
        "A of 2 GB by shape": dict(M=1 << 20, lda=1024),
        "B of 2 GB by shape": dict(N=1 << 21, ldb=512),
        "epi out of range": dict(epi=4),
        "epi negative": dict(epi=-1),
        "DLRELU without aux": dict(epi=EPI_DLRELU),
        "drop_p = 1": dict(epi=EPI_DROPOUT, p=1.0),
        "batch 0": dict(batch=0),
    }
    assert call() == 0 and call(epi=EPI_DLRELU, aux=aux.data_ptr()) == 0   # the base call is accepted
    torch.cuda.synchronize()
    C.fill_(SENTINEL)
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        assert "gemm_bf16" in _last_error(), what
    torch.cuda.synchronize()
    assert bool((C == SENTINEL).all())
