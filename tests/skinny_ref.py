"""Harness of the skinny layer-0 product edge tests (include/mlvae.h, csrc/skinny.hip):
mlvae_skinny_nt, _nt_fp8, _proj, _proj_ex, _tn, _tn_fp8 and _dzw.

Operands  every operand value is a small integer, uniform in [-4, 4]: exact in bf16 and in e4m3.
          Each product of two of them is an integer of magnitude <= 16, so a sum over a reduction
          of length K is an integer with |sum| <= 16 K -- below 2^24 for every case here (the
          longest reduction is 2056 frames).  Any order of fp32 accumulation is then exact, and a
          kernel's result equals the fp64 reference cast to fp32 bit for bit: the GPU tests compare
          with torch.equal, no tolerance.  alpha of the fp8 entries is 2^-3 (an exact scaling);
          proj's biases are integers in [-4, 4], |result| <= 16 * 32 + 8 <= 2048, exact in fp16.
Placement place() / logical_mask() / SENTINEL of gemm_fast_ref: every operand lies in a flat buffer
          between guards with a leading dimension that may be wider than its logical width; every
          non-logical input element is NaN (bf16 NaN, byte 0x7F for e4m3), every output element is
          prefilled with SENTINEL and all non-logical ones must still hold it after a launch.
ref_*()   fp64 results of the header's contracts from the LOGICAL operands;
addr_*()  the same contracts by explicit flat indexing (NumPy, offset + row * ld + col on the
          placed buffers): they check the placement arithmetic of this harness itself
          (tests/test_skinny_ref_cpu.py);
nt_form(), tn_plan(), dzw_plan()  Python twins of the host-side dispatch of csrc/skinny.hip;
make_*()  one placed case (operands, prefilled outputs, fp64 references) per entry point;
run_*()   the ctypes launches with every leading dimension explicit.

Importing this module needs no GPU and no libmlvae.so (the run_* wrappers bind the library when
called).
"""
import numpy as np
import torch

from gemm_fast_ref import SENTINEL, logical_index, logical_mask, place

NAN = float("nan")
G = 4096            # guard elements (a multiple of 16: 16-byte aligned bases for every dtype here)
ALPHA8 = 0.125      # the fp8 entries' alpha: 2^-3
F8_NAN = 0x7F       # e4m3 NaN
DZW_Z, DZW_NB = 32, 48


# ------------------------------------------------------------------------------------------------
# operands and placement
def ints(*shape, seed, nonzero=False):
    """float32 integers uniform in [-4, 4] (nonzero: in [-4, -1] u [1, 4])."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-4, 5, shape, generator=g).float()
    if nonzero:
        s = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
        v = torch.where(v == 0, s, v)
    return v


def seed_of(args):
    """A case's operand seed from its argument tuple (the CPU and the GPU tests see the same data)."""
    return sum((i + 1) * int(a) for i, a in enumerate(args))


class Buf:
    """A matrix (or, 1-D, a vector) place()d into a flat buffer: flat, off, ld, rows, cols."""

    def __init__(self, mat, ld, poison, guard=G, fp8=False):
        self.fp8 = fp8
        if fp8:  # e4m3 bytes; the poison is the NaN byte
            mat = mat.to(torch.float8_e4m3fn).view(torch.uint8)
        if mat.dim() == 1:
            self.rows, self.cols, self.ld = 1, mat.numel(), mat.numel()
            self.flat, self.off = place(mat, 0, guard, poison)
        else:
            self.rows, self.cols, self.ld = mat.shape[0], mat.shape[1], ld
            self.flat, self.off = place(mat, ld, guard, poison)
        self.dev = None

    def f64(self):
        """The flat buffer as float64 NumPy (e4m3 bytes decoded; poison stays NaN)."""
        f = self.flat.view(torch.float8_e4m3fn).float() if self.fp8 else self.flat
        return f.double().numpy()

    def mask(self):
        return logical_mask(self.flat.numel(), self.off, 1, self.rows, self.cols, self.ld, 0)

    def logical(self, flat=None):
        """[rows, cols] (a vector: [1, n]) of a flat buffer laid out like this one."""
        flat = self.flat if flat is None else flat
        return flat[logical_index(self.off, 1, self.rows, self.cols, self.ld, 0)[0]]


def inp(mat, ld, fp8=False):
    """Input operand: bf16 (or e4m3) between NaN poison."""
    if fp8:
        return Buf(mat, ld, F8_NAN, fp8=True)
    return Buf(mat.to(torch.bfloat16), ld, NAN)


def inp32(vec):
    """fp32 input vector (a bias) between NaN poison."""
    return Buf(vec.float(), 0, NAN)


def out(rows, cols, ld, dtype=torch.float32):
    """Output: SENTINEL everywhere, logical region included."""
    shape = (rows, cols) if rows is not None else (cols,)
    return Buf(torch.full(shape, SENTINEL, dtype=dtype), ld, SENTINEL)


class Case:
    """One placed case: .ins / .outs (name -> Buf), .ref (name -> fp64 logical result) and the
    call's scalars as attributes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


# ------------------------------------------------------------------------------------------------
# fp64 references from the logical operands
def ref_nt(A, Bt, alpha=1.0):
    """C [M, N] = alpha A [M, K] Bt [N, K]^T."""
    return alpha * (A.double() @ Bt.double().t())


def ref_proj(A, B, b1=None, b2=None):
    """C [M, N] = A [M, K] B [N, K]^T + b1 + b2."""
    r = A.double() @ B.double().t()
    if b1 is not None:
        r = r + b1.double()
    if b2 is not None:
        r = r + b2.double()
    return r


def ref_tn(A, B, nw, alpha=1.0):
    """(W [M, nw], bias [M] or None) = alpha A [K, M]^T B [K, NB]: columns < nw and column nw (None
    when B has no such column).  Columns of B beyond nw + 1 reach neither."""
    p = alpha * (A.double().t() @ B.double())
    return p[:, :nw], (p[:, nw] if nw < B.shape[1] else None)


def ref_dzw(dG, Wt, zb):
    """(dZ [M, 32], W [K8, 32], bias [K8]) = (dG Wt^T, dG^T z, dG^T 1) with zb = [z | 1 | 0]."""
    dz = dG.double() @ Wt.double().t()
    p = dG.double().t() @ zb.double()
    return dz, p[:, :DZW_Z], p[:, DZW_Z]


# ------------------------------------------------------------------------------------------------
# the same contracts by explicit flat indexing on the placed buffers (float64 NumPy arrays)
def _rc(rows, cols):
    return np.arange(rows)[:, None], np.arange(cols)[None, :]


def addr_nt(M, N, K, Af, a0, lda, Bf, b0, ldb, Cf, c0, ldc, alpha=1.0):
    """Cf (copy) with C[m, n] = alpha sum_k Af[a0 + m lda + k] Bf[b0 + n ldb + k]."""
    Cf = np.array(Cf, dtype=np.float64)
    m, k = _rc(M, K)
    n, k2 = _rc(N, K)
    r = alpha * (Af[a0 + m * lda + k] @ Bf[b0 + n * ldb + k2].T) if K > 0 else np.zeros((M, N))
    mm, nn = _rc(M, N)
    Cf[c0 + mm * ldc + nn] = r
    return Cf


def addr_proj(M, N, K, Af, a0, lda, Bf, b0, ldb, b1f, b1_0, b2f, b2_0, Cf, c0, ldc):
    """Cf (copy) with C[m, n] = sum_k Af[a0 + m lda + k] Bf[b0 + n ldb + k] + b1f[b1_0 + n] +
    b2f[b2_0 + n] (a bias that is None adds nothing)."""
    Cf = addr_nt(M, N, K, Af, a0, lda, Bf, b0, ldb, Cf, c0, ldc)
    mm, nn = _rc(M, N)
    for bf, o in ((b1f, b1_0), (b2f, b2_0)):
        if bf is not None:
            Cf[c0 + mm * ldc + nn] += bf[o + nn]
    return Cf


def _addr_tn_product(M, ncol, K, Af, a0, lda, Bf, b0, ldb):
    """P [M, ncol] = sum_f Af[a0 + f lda + m] Bf[b0 + f ldb + n], frames in blocks of 256."""
    p = np.zeros((M, ncol))
    for f0 in range(0, K, 256):
        f, m = _rc(min(256, K - f0), M)
        f2, n = _rc(min(256, K - f0), ncol)
        p += Af[a0 + (f0 + f) * lda + m].T @ Bf[b0 + (f0 + f2) * ldb + n]
    return p


def addr_tn(M, NB, K, Af, a0, lda, Bf, b0, ldb, nw, Wf, w0, b1f, b1_0, b2f, b2_0, alpha=1.0):
    """(Wf, b1f, b2f) copies with W[m, n] = alpha sum_f Af[a0 + f lda + m] Bf[b0 + f ldb + n] at
    w0 + m nw + n for n < nw, and column nw at b1_0 + m / b2_0 + m of each bias given.  Only
    columns < nw (+ 1 with a bias) of B are read."""
    bias = b1f is not None or b2f is not None
    p = alpha * _addr_tn_product(M, nw + (1 if bias else 0), K, Af, a0, lda, Bf, b0, ldb)
    Wf = np.array(Wf, dtype=np.float64)
    mm, nn = _rc(M, nw)
    Wf[w0 + mm * nw + nn] = p[:, :nw]
    res = [Wf]
    for bf, o in ((b1f, b1_0), (b2f, b2_0)):
        if bf is not None:
            bf = np.array(bf, dtype=np.float64)
            bf[o + np.arange(M)] = p[:, nw]
        res.append(bf)
    return tuple(res)


def addr_dzw(M, K8, Af, a0, lda, Wtf, wt0, ldw, Zf, z0, ldz, dZf, dz0, lddz, Wf, w0, b1f, b1_0, b2f, b2_0):
    """(dZf, Wf, b1f, b2f) copies: dZ[m, j] = sum_k Af[a0 + m lda + k] Wtf[wt0 + j ldw + k] at
    dz0 + m lddz + j (j < 32); W and the biases as addr_tn over the M frames with B = the z block
    (nw = 32, the ones column at 32)."""
    dZf = addr_nt(M, DZW_Z, K8, Af, a0, lda, Wtf, wt0, ldw, dZf, dz0, lddz)
    Wf, b1f, b2f = addr_tn(K8, DZW_NB, M, Af, a0, lda, Zf, z0, ldz, DZW_Z, Wf, w0, b1f, b1_0, b2f, b2_0)
    return dZf, Wf, b1f, b2f


# ------------------------------------------------------------------------------------------------
# Python twins of the host-side dispatch in csrc/skinny.hip
def nt_form(M, N, K):
    """The kernel mlvae_skinny_nt launches: "lds" (Bt through LDS, 128-row workgroups) when K > 0,
    K % 256 == 0 and M >= 4096; else "ks" (K split over four waves) when K % 128 == 0; else
    "plain"."""
    if K > 0 and K % 256 == 0 and M >= 4096:
        return "lds"
    return "ks" if K % 128 == 0 else "plain"


def tn_plan(M, K):
    """(S, kc, empty): tn_splits(M, K), the frames per split rounded up to 64, and the splits
    whose first frame s * kc is >= K (they must store a zero slab)."""
    mb = (M + 63) // 64
    s = (2048 + mb - 1) // mb
    s = max(1, min(s, (K + 255) // 256))
    kc = ((K + s - 1) // s + 63) // 64 * 64
    return s, kc, [i for i in range(s) if i * kc >= K]


def dzw_plan(M, K8):
    """(G, nrb, ntl): workgroups, 128-row blocks per workgroup, tiles (chunks x row blocks) per
    workgroup of skinny_dzw_kernel."""
    nrb_all = (M + 127) // 128
    g = (nrb_all + 3) // 4
    nrb = [min(4, nrb_all - 4 * i) for i in range(g)]
    return g, nrb, [K8 // 256 * b for b in nrb]


# ------------------------------------------------------------------------------------------------
# case lists (tests/test_skinny_ref_cpu.py checks each list has the property it is named for)
NS = (16, 32, 48, 64)
NT_SHAPES = {"plain": [(77, 32), (77, 96), (77, 160)],
             "ks": [(300, 128), (300, 384), (300, 640), (4095, 256)],
             "lds": [(4096, 256), (4173, 256), (4173, 512), (4173, 768)]}
NT_ONE_CHUNK = [(4096, 256), (4173, 256)]       # the LDS form with one chunk: no prefetch
NT_ODD_CHUNKS = [(4173, 768)]                   # ... ending on sb[0] after using sb[1]
NT_KS_BOTH_LOOPS = [(300, 640)]                 # K / 4 = 160: the unrolled loop, then the tail
NT_TIGHT = [(77, 48, 96), (300, 48, 384), (4173, 48, 512)]   # (M, N, K), one per kernel form
NT_K0 = [(77, 32), (4173, 32)]                  # (M, N) at K == 0: zeros
NT8_SHAPES = [(4173, 256), (4173, 768)]

PROJ_KS, PROJ_NS, PROJ_MS = (8, 16, 24, 32), (16, 144, 528, 1040), (1, 15, 17, 64, 65, 77)


def proj_cases():
    """(f16, M, N, K, bias mask, padded): 14 padded cases per output type in which every K, N, M
    and bias combination (bit 0: bias1, bit 1: bias2) occurs, plus one tight case each."""
    cases = []
    for f16 in (0, 1):
        for i in range(14):
            j = i + 5 * f16
            cases.append((f16, PROJ_MS[j % 6], PROJ_NS[(j + j // 4) % 4], PROJ_KS[i % 4], (i // 2 + f16) % 4, True))
        cases.append((f16, 77, 528, 24, 3, False))
    return cases


TN_ROWS = [(64, 16, 15, 3), (64, 16, 16, 0), (128, 32, 20, 1), (192, 48, 32, 2), (64, 64, 63, 3),
           (256, 64, 40, 3)]                    # (M, NB, nw, bias mask)
TN_KS = (1, 63, 64, 65, 130, 1000)
TN_EMPTY_SPLIT = [(16384, 48, 32, 3, 2056)]     # (M, NB, nw, bias mask, K)
TN_TIGHT = [(192, 48, 32, 3, 130)]
TN8_ROWS = [(128, 32, 20, 1), (64, 64, 63, 3)]
TN8_KS = (65, 1000)

DZW_SHAPES = [(1, 256), (129, 256), (300, 768), (512, 256), (513, 512), (640, 768), (900, 1024)]
DZW_NTL_1 = [(1, 256)]
DZW_NRB_2 = [(129, 256)]
DZW_ODD_NTL = [(300, 768), (640, 768)]
DZW_BIAS = (3, 1, 0)
DZW_TIGHT = [(300, 768)]

# the argument tuples of make_nt / make_nt(fp8) / make_tn / make_tn(fp8) / make_dzw, in launch order
NT_CASES = ([(M, N, K, True) for f in ("plain", "ks", "lds") for M, K in NT_SHAPES[f] for N in NS] +
            [(M, N, K, False) for M, N, K in NT_TIGHT] + [(M, N, 0, True) for M, N in NT_K0])
NT8_CASES = [(M, N, K, True) for M, K in NT8_SHAPES for N in NS] + [(4173, 48, 512, False)]
TN_CASES = ([r + (K, True) for r in TN_ROWS for K in TN_KS] + [r + (True,) for r in TN_EMPTY_SPLIT] +
            [r + (False,) for r in TN_TIGHT])
TN8_CASES = [r + (K, True) for r in TN8_ROWS for K in TN8_KS] + [(128, 32, 20, 1, 130, False)]
DZW_CASES = [(M, K8, b, True) for M, K8 in DZW_SHAPES for b in DZW_BIAS] + [(M, K8, 3, False) for M, K8 in DZW_TIGHT]


# ------------------------------------------------------------------------------------------------
# placed cases
def make_nt(M, N, K, padded=True, fp8=False, seed=0):
    """nt / nt_fp8: lda = K + 8 (fp8: K + 16 bytes), ldb = K + 24, ldc = N + 4 when padded."""
    A, Bt = ints(M, K, seed=seed + 1), ints(N, K, seed=seed + 2)
    lda = K + ((16 if fp8 else 8) if padded else 0)
    ldb, ldc = K + (24 if padded else 0), N + (4 if padded else 0)
    alpha = ALPHA8 if fp8 else 1.0
    return Case(M=M, N=N, K=K, fp8=fp8, alpha=alpha, ins=dict(A=inp(A, lda, fp8), Bt=inp(Bt, ldb)),
                outs=dict(C=out(M, N, ldc)), ref=dict(C=ref_nt(A, Bt, alpha)))


def make_proj(f16, M, N, K, bias, padded=True, seed=0):
    """proj / proj_ex: lda = ldb = K + 8, ldc = N + 8 when padded; bias bit 0: bias1, bit 1: bias2."""
    A, B = ints(M, K, seed=seed + 1), ints(N, K, seed=seed + 2)
    b1, b2 = ints(N, seed=seed + 3), ints(N, seed=seed + 4)
    pad = 8 if padded else 0
    r = ref_proj(A, B, b1 if bias & 1 else None, b2 if bias & 2 else None)
    return Case(M=M, N=N, K=K, f16=f16, bias=bias, ins=dict(A=inp(A, K + pad), B=inp(B, K + pad), b1=inp32(b1), b2=inp32(b2)),
                outs=dict(C=out(M, N, N + pad, torch.float16 if f16 else torch.float32)), ref=dict(C=r))


def make_tn(M, NB, nw, bias, K, padded=True, fp8=False, seed=0):
    """tn / tn_fp8: A [K, M] with lda = M + 8 (fp8: M + 16 bytes), B [K, NB] with ldb = NB + 8 when
    padded.  B: integers in columns < nw, ones in column nw when a bias is wanted, NON-ZERO
    integers in every other column -- they must reach neither W nor a bias."""
    A = ints(K, M, seed=seed + 1)
    B = ints(K, NB, seed=seed + 2)
    B[:, nw:] = ints(K, NB - nw, seed=seed + 3, nonzero=True)
    if bias and nw < NB:
        B[:, nw] = 1.0
    lda = M + ((16 if fp8 else 8) if padded else 0)
    alpha = ALPHA8 if fp8 else 1.0
    W, b = ref_tn(A, B, nw, alpha)
    return Case(M=M, NB=NB, nw=nw, bias=bias, K=K, fp8=fp8, alpha=alpha,
                ins=dict(A=inp(A, lda, fp8), B=inp(B, NB + (8 if padded else 0))),
                outs=dict(W=out(M, nw, nw), b1=out(None, M, 0), b2=out(None, M, 0)), ref=dict(W=W, b=b))


def make_dzw(M, K8, bias, padded=True, seed=0):
    """dzw: lda = K8 + 8, ldw = K8 + 16, ldz = 56, lddz = 36 when padded; zb = [z | 1 | 0]."""
    dG, Wt = ints(M, K8, seed=seed + 1), ints(DZW_Z, K8, seed=seed + 2)
    zb = torch.zeros(M, DZW_NB)
    zb[:, :DZW_Z] = ints(M, DZW_Z, seed=seed + 3)
    zb[:, DZW_Z] = 1.0
    p = padded
    dz, W, b = ref_dzw(dG, Wt, zb)
    return Case(M=M, K8=K8, bias=bias,
                ins=dict(A=inp(dG, K8 + (8 if p else 0)), Wt=inp(Wt, K8 + (16 if p else 0)),
                         zb=inp(zb, 56 if p else DZW_NB)),
                outs=dict(dZ=out(M, DZW_Z, 36 if p else DZW_Z), W=out(K8, DZW_Z, DZW_Z), b1=out(None, K8, 0),
                          b2=out(None, K8, 0)), ref=dict(dZ=dz, W=W, b=b))


def addr_case(kind, c):
    """The addr_* twin of a placed case -> name -> flat float64 output (None: not an output of
    this call)."""
    i, o = c.ins, c.outs
    A = i["A"]
    if kind == "nt":
        Bt, C = i["Bt"], o["C"]
        return dict(C=addr_nt(c.M, c.N, c.K, A.f64(), A.off, A.ld, Bt.f64(), Bt.off, Bt.ld, C.f64(), C.off, C.ld, c.alpha))
    if kind == "proj":
        B, C, b1, b2 = i["B"], o["C"], i["b1"], i["b2"]
        return dict(C=addr_proj(c.M, c.N, c.K, A.f64(), A.off, A.ld, B.f64(), B.off, B.ld,
                                b1.f64() if c.bias & 1 else None, b1.off, b2.f64() if c.bias & 2 else None, b2.off,
                                C.f64(), C.off, C.ld))
    b1, b2 = o["b1"], o["b2"]
    b1f, b2f = (b1.f64() if c.bias & 1 else None), (b2.f64() if c.bias & 2 else None)
    if kind == "tn":
        B, W = i["B"], o["W"]
        r = addr_tn(c.M, c.NB, c.K, A.f64(), A.off, A.ld, B.f64(), B.off, B.ld, c.nw, W.f64(), W.off, b1f, b1.off,
                    b2f, b2.off, c.alpha)
        return dict(W=r[0], b1=r[1], b2=r[2])
    Wt, zb, dZ, W = i["Wt"], i["zb"], o["dZ"], o["W"]
    r = addr_dzw(c.M, c.K8, A.f64(), A.off, A.ld, Wt.f64(), Wt.off, Wt.ld, zb.f64(), zb.off, zb.ld, dZ.f64(), dZ.off,
                 dZ.ld, W.f64(), W.off, b1f, b1.off, b2f, b2.off)
    return dict(dZ=r[0], W=r[1], b1=r[2], b2=r[3])


def expected(kind, c):
    """name -> the fp64 reference of every output this call writes (a bias not passed is absent)."""
    e = {k: v for k, v in c.ref.items() if k != "b"}
    if kind in ("tn", "dzw"):
        for bit, name in ((1, "b1"), (2, "b2")):
            if c.bias & bit:
                e[name] = c.ref["b"].reshape(1, -1)
    return e


# ------------------------------------------------------------------------------------------------
# launches
def _ptr(t, off=0):
    return t.data_ptr() + off * t.element_size() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lib():
    from mlvae_hip._lib import lib
    return lib()


def make_ws(need):
    """A workspace of need bytes (+ 4 floats), all SENTINEL: the float just past need must survive."""
    return torch.full((need // 4 + 4,), SENTINEL, device="cuda")


def run_nt(M, N, K, A, a0, lda, Bt, b0, ldb, C, c0, ldc):
    rc = _lib().mlvae_skinny_nt(M, N, K, _ptr(A, a0), lda, _ptr(Bt, b0), ldb, _ptr(C, c0), ldc, _stream())
    torch.cuda.synchronize()
    return rc


def run_nt_fp8(M, N, K, A8, a0, lda, Bt, b0, ldb, C, c0, ldc, alpha):
    rc = _lib().mlvae_skinny_nt_fp8(M, N, K, _ptr(A8, a0), lda, _ptr(Bt, b0), ldb, _ptr(C, c0), ldc, _ptr(alpha),
                                    _stream())
    torch.cuda.synchronize()
    return rc


def run_proj(M, N, K, A, a0, lda, B, b0, ldb, b1, b1_0, b2, b2_0, C, c0, ldc, c_fp16=None):
    """c_fp16 None: mlvae_skinny_proj (fp32 C); 0 / 1: mlvae_skinny_proj_ex."""
    l = _lib()
    if c_fp16 is None:
        rc = l.mlvae_skinny_proj(M, N, K, _ptr(A, a0), lda, _ptr(B, b0), ldb, _ptr(b1, b1_0), _ptr(b2, b2_0),
                                 _ptr(C, c0), ldc, _stream())
    else:
        rc = l.mlvae_skinny_proj_ex(M, N, K, _ptr(A, a0), lda, _ptr(B, b0), ldb, _ptr(b1, b1_0), _ptr(b2, b2_0),
                                    _ptr(C, c0), ldc, c_fp16, _stream())
    torch.cuda.synchronize()
    return rc


def run_tn(M, NB, K, A, a0, lda, B, b0, ldb, nw, W, w0, b1, b1_0, b2, b2_0, ws, ws_bytes, alpha=None):
    """alpha None: mlvae_skinny_tn; a device float: mlvae_skinny_tn_fp8 (A e4m3, lda in bytes)."""
    l = _lib()
    if alpha is None:
        rc = l.mlvae_skinny_tn(M, NB, K, _ptr(A, a0), lda, _ptr(B, b0), ldb, nw, _ptr(W, w0), _ptr(b1, b1_0),
                               _ptr(b2, b2_0), _ptr(ws), ws_bytes, _stream())
    else:
        rc = l.mlvae_skinny_tn_fp8(M, NB, K, _ptr(A, a0), lda, _ptr(B, b0), ldb, nw, _ptr(W, w0), _ptr(b1, b1_0),
                                   _ptr(b2, b2_0), _ptr(alpha), _ptr(ws), ws_bytes, _stream())
    torch.cuda.synchronize()
    return rc


def run_dzw(M, K8, A, a0, lda, Wt, wt0, ldw, zb, z0, ldz, Z, dZ, dz0, lddz, W, w0, b1, b1_0, b2, b2_0, ws, ws_bytes):
    rc = _lib().mlvae_skinny_dzw(M, K8, _ptr(A, a0), lda, _ptr(Wt, wt0), ldw, _ptr(zb, z0), ldz, Z, _ptr(dZ, dz0),
                                 lddz, _ptr(W, w0), _ptr(b1, b1_0), _ptr(b2, b2_0), _ptr(ws), ws_bytes, _stream())
    torch.cuda.synchronize()
    return rc
