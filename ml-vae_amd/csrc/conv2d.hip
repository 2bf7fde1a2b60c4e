// The CRDNN's convolutional front end (SpeechBrain's CRDNN lobe as the CRDNN_CTC recipes' yaml
// builds it, ref:src/models/CRDNN_CTC/model.yaml:23-35; the lobe itself is not vendored: parity
// with it is unpinned, the semantics below are torch's).  Activations are channels-last
// [B, T, F, C], contiguous fp32 at the ABI; the convolution runs over the padded batch (no
// utterance lengths), reflection at the batch's own T and F borders.
//
// Conv2d 3x3, stride 1, "same", reflect padding 1 (x[-1] = x[1], x[T] = x[T-2]; likewise on F),
// weight [Cout][Cin][3 (time)][3 (freq)]:
//   * pad_bf16_kernel writes a padded bf16 copy xp [B, T+2, F+2, Cin].  In it the three frequency
//     taps of one position are 3 Cin contiguous elements, so for each time tap kt the A operand of
//     the implicit GEMM (M = B T F positions, N = Cout, K = 9 Cin) is a row of "overlapping rows":
//     conv2d_mfma_kernel reads its fragments straight from xp -- no im2col buffer -- and the
//     packed bf16 weights Wp[Cout][3][roundup(3 Cin, 32)] (zero past 3 Cin) on
//     v_mfma_f32_16x16x32_bf16 with swapped operands (a lane ends with 4 consecutive output
//     channels of one position: 16-byte stores).  Two forms: for N % 128 == 0 (the recipe's widths)
//     conv2d_mfma_lds_kernel stages a 128-position x 128-channel tile's operands in LDS, K chunk by
//     K chunk; otherwise conv2d_mfma_kernel (4 waves x (32 or 64 positions x 16 NT channels)) reads
//     its fragments straight from global memory and leaves the reuse between waves to L1 / L2.
//   * input gradient = the same kernel: the full correlation of a zero-padded (2) bf16 copy of dy
//     with the flipped, transposed weights over the padded extent [T+2, F+2], then
//     fold_kernel adds the four border rows / columns onto their mirror sources (T = 2: both
//     borders fold onto interior elements).
//   * weight gradient: dW[co][ci][kt][kf] = sum_p dy[p][co] xp[p + (kt, kf)][ci]: per (kt, 64 x 64
//     tile of [Cout] x [3 Cin]) and position split, 32 positions at a time staged in LDS as bf16
//     and read transposed (ds_read_b64_tr_b16); one slab per split, summed in split order
//     (deterministic, no float atomics).  Bias gradient: fp32 column sums of dy, two fixed-order
//     stages.
// First layer (Cin = 1, x [B, T, F]): K = 9, bandwidth-bound direct fp32 kernels (forward, weight
// + bias gradient; the features carry no gradient).
//
// LayerNorm over (F, C) + LeakyReLU(0.01) [+ frequency max-pool 2 (floor; a tie keeps the lower
// bin) + Dropout2d keep mask [B, F/2]]: one workgroup per (b, t) row, two-pass mean / biased
// variance, mean and rstd saved; the backward recomputes the pre-activation and the pool's
// argmax from the saved input.  d gamma / d beta: rows summed per row split in row order, the
// splits in split order.  Time max-pool 2 (floor), forward and backward.
#include "common.h"

namespace {

constexpr int CT = 256;
constexpr int LDT = 72;  // shorts per row of the weight gradient's LDS images (64 + 8 skew)
// deterministic workgroup sum (4 waves): butterfly per wave, the waves in order
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// ------------------------------------------------------------------ padded bf16 copies
// xp [B][T + 2P][F + 2P][C] (bf16) of x [B][T][F][C] (fp32): reflect (P = 1) or zeros
__global__ __launch_bounds__(CT) void pad_bf16_kernel(int T, int F, int C, int P, int reflect, size_t nq,
                                                      const float* __restrict__ x, short* __restrict__ xp) {
  const int C4 = C / 4, Fp = F + 2 * P, Tp = T + 2 * P;
  for (size_t i = (size_t)blockIdx.x * CT + threadIdx.x; i < nq; i += (size_t)gridDim.x * CT) {
    const int c = (int)(i % C4) * 4;
    size_t r = i / C4;
    const int fp = (int)(r % Fp);
    r /= Fp;
    const int tp = (int)(r % Tp);
    const size_t b = r / Tp;
    int t = tp - P, f = fp - P;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (reflect) { t = reflect1(t, T); f = reflect1(f, F); }
    if (t >= 0 && t < T && f >= 0 && f < F) v = *(const f32x4*)(x + ((b * T + t) * F + f) * C + c);
    *(bf16x4*)(xp + i * 4) = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
  }
}

// Wp[n][kt][k], k = kf C + c < 3 C (zero up to Rp).  Forward: n = co, c = ci, w[co][ci][kt][kf].
// Input gradient (flip): n = ci, c = co (C = the layer's Cout, N = its Cin), w[co][ci][2-kt][2-kf].
__global__ __launch_bounds__(CT) void pack_w_kernel(int N, int C, int Rp, int flip, const float* __restrict__ w,
                                                    short* __restrict__ wp) {
  const size_t n_el = (size_t)N * 3 * Rp;
  for (size_t i = (size_t)blockIdx.x * CT + threadIdx.x; i < n_el; i += (size_t)gridDim.x * CT) {
    const int k = (int)(i % Rp);
    const size_t r = i / Rp;
    const int kt = (int)(r % 3), n = (int)(r / 3);
    float v = 0.f;
    if (k < 3 * C) {
      const int kf = k / C, c = k - kf * C;
      v = flip ? w[(((size_t)c * N + n) * 3 + (2 - kt)) * 3 + (2 - kf)] : w[(((size_t)n * C + c) * 3 + kt) * 3 + kf];
    }
    wp[i] = f2bf(v);
  }
}

// ------------------------------------------------------------------ the implicit GEMM
// "valid" 3x3 correlation of the padded xp [B][Tp][Fp][C] with Wp -> y [B][To = Tp-2][Fo = Fp-2][N]
struct C2Args {
  int Tp, Fp, C, N, To, Fo, Rp;
  long long M;  // B To Fo
  const short* xp;
  const short* wp;
  const float* bias;
  float* y;
};

template <int MF, int NT>
__global__ __launch_bounds__(CT) void conv2d_mfma_kernel(C2Args a) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long m0 = (long long)blockIdx.x * (64 * MF) + wave * (16 * MF);
  if (m0 >= a.M) return;  // whole wave; the kernel has no barrier
  const int n0 = blockIdx.y * 16 * NT;
  const int R = 3 * a.C;
  size_t rb[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    long long m = m0 + 16 * mf + l15;
    if (m >= a.M) m = a.M - 1;  // loads stay in bounds; the store is skipped
    const long long pf = (long long)a.To * a.Fo;
    const long long b = m / pf;
    const int r = (int)(m - b * pf), t = r / a.Fo, f = r - t * a.Fo;
    rb[mf] = (((size_t)b * a.Tp + t) * a.Fp + f) * a.C;
  }
  f32x4 acc[MF][NT];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mf][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < 3; ++kt) {
    const size_t xo = (size_t)kt * a.Fp * a.C;
    const short* wrow = a.wp + ((size_t)(n0 + l15) * 3 + kt) * a.Rp;
    for (int kk = 0; kk < a.Rp; kk += 32) {
      const int k = kk + 8 * q;
      bf16x8 xb[MF];
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        xb[mf] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (k < R) xb[mf] = *(const bf16x8*)(a.xp + rb[mf] + xo + k);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x8 wa = *(const bf16x8*)(wrow + (size_t)nt * 16 * 3 * a.Rp + k);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) acc[mf][nt] = mfma16(wa, xb[mf], acc[mf][nt]);
      }
    }
  }
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    const long long m = m0 + 16 * mf + l15;
    if (m < a.M) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + 16 * nt + 4 * q;
        f32x4 v = acc[mf][nt];
        if (a.bias) v += *(const f32x4*)(a.bias + n);
        *(f32x4*)(a.y + (size_t)m * a.N + n) = v;
      }
    }
  }
}

// The same product for N % 128 == 0 (the recipe's 128 and 256 channels) with both operands staged
// in LDS: a workgroup owns 128 positions x 128 channels, each of its 2 x 2 waves 64 x 64 (16
// MFMAs per 8 fragment reads).  K runs per time tap in chunks of KS = 64 of the tap's 3 C
// contiguous elements (zero past 3 C); the next chunk's 16-byte global loads (4 + 4 per thread) are
// issued before the current chunk's MFMAs.  Row stride KS + 8 shorts = 36 dwords: the 16 rows of a
// fragment read fall on distinct banks.
constexpr int KS = 64, LDK = KS + 8;

__global__ __launch_bounds__(CT) void conv2d_mfma_lds_kernel(C2Args a) {
  __shared__ __attribute__((aligned(16))) short Xl[128 * LDK];
  __shared__ __attribute__((aligned(16))) short Wl[128 * LDK];
  const int lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const long long mblk = (long long)blockIdx.x * 128;
  const int n0 = blockIdx.y * 128;
  const int g8 = (threadIdx.x & 7) * 8, sr = threadIdx.x >> 3;  // staging: k group, first row
  const int R = 3 * a.C, nks = (R + KS - 1) / KS, steps = 3 * nks;
  const long long pf = (long long)a.To * a.Fo;
  size_t rbx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    long long m = mblk + sr + 32 * j;
    if (m >= a.M) m = a.M - 1;  // loads stay in bounds; the store is skipped
    const long long b = m / pf;
    const int r = (int)(m - b * pf), t = r / a.Fo, f = r - t * a.Fo;
    rbx[j] = (((size_t)b * a.Tp + t) * a.Fp + f) * a.C;
  }
  bf16x8 px[4], pw[4];
  auto load = [&](int s) {
    const int kt = s / nks, k = (s - kt * nks) * KS + g8;
    const size_t xo = (size_t)kt * a.Fp * a.C + k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      px[j] = pw[j] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (k < R) {
        px[j] = *(const bf16x8*)(a.xp + rbx[j] + xo);
        pw[j] = *(const bf16x8*)(a.wp + ((size_t)(n0 + sr + 32 * j) * 3 + kt) * a.Rp + k);
      }
    }
  };
  f32x4 acc[4][4];
#pragma unroll
  for (int mf = 0; mf < 4; ++mf)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mf][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int s = 0; s < steps; ++s) {
    lds_barrier();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *(bf16x8*)(Xl + (sr + 32 * j) * LDK + g8) = px[j];
      *(bf16x8*)(Wl + (sr + 32 * j) * LDK + g8) = pw[j];
    }
    lds_barrier();
    if (s + 1 < steps) load(s + 1);
#pragma unroll
    for (int kk = 0; kk < KS; kk += 32) {
      bf16x8 xb[4], wa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xb[i] = *(const bf16x8*)(Xl + (64 * wm + 16 * i + l15) * LDK + kk + 8 * q);
        wa[i] = *(const bf16x8*)(Wl + (64 * wn + 16 * i + l15) * LDK + kk + 8 * q);
      }
#pragma unroll
      for (int mf = 0; mf < 4; ++mf)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mf][nt] = mfma16(wa[nt], xb[mf], acc[mf][nt]);
    }
  }
#pragma unroll
  for (int mf = 0; mf < 4; ++mf) {
    const long long m = mblk + 64 * wm + 16 * mf + l15;
    if (m < a.M) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + 64 * wn + 16 * nt + 4 * q;
        f32x4 v = acc[mf][nt];
        if (a.bias) v += *(const f32x4*)(a.bias + n);
        *(f32x4*)(a.y + (size_t)m * a.N + n) = v;
      }
    }
  }
}

// dx [B][T][F][C] = dxp [B][T+2][F+2][C] folded: padded row 0 onto t = 1, row T+1 onto t = T-2
// (and the columns likewise), each sum in a fixed order
__global__ __launch_bounds__(CT) void fold_kernel(int T, int F, int C, size_t nq, const float* __restrict__ dxp,
                                                  float* __restrict__ dx) {
  const int C4 = C / 4, Fp = F + 2, Tp = T + 2;
  for (size_t i = (size_t)blockIdx.x * CT + threadIdx.x; i < nq; i += (size_t)gridDim.x * CT) {
    const int c = (int)(i % C4) * 4;
    size_t r = i / C4;
    const int f = (int)(r % F);
    r /= F;
    const int t = (int)(r % T);
    const size_t b = r / T;
    int ts[3], fs[3], nt = 0, nf = 0;
    if (t == 1) ts[nt++] = 0;
    ts[nt++] = t + 1;
    if (t == T - 2) ts[nt++] = T + 1;
    if (f == 1) fs[nf++] = 0;
    fs[nf++] = f + 1;
    if (f == F - 2) fs[nf++] = F + 1;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int u = 0; u < nt; ++u)
      for (int v = 0; v < nf; ++v) s += *(const f32x4*)(dxp + ((b * Tp + ts[u]) * Fp + fs[v]) * C + c);
    *(f32x4*)(dx + i * 4) = s;
  }
}

// ------------------------------------------------------------------ weight gradient
struct WgArgs {
  int T, F, C, N, Tp, Fp, nCo, nJ, steps, sps;
  long long M;
  const float* dy;   // [M][N]
  const short* xp;   // [B][Tp][Fp][C]
  float* slabs;      // [splits][3][N][3 C]
  size_t S;          // 9 C N
};

__global__ __launch_bounds__(CT) void conv2d_wgrad_kernel(WgArgs a) {
  __shared__ __attribute__((aligned(16))) short DYl[32 * LDT];
  __shared__ __attribute__((aligned(16))) short Xl[32 * LDT];
  const int lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int tile = blockIdx.x;
  const int jt = tile % a.nJ;
  tile /= a.nJ;
  const int cot = tile % a.nCo, kt = tile / a.nCo;
  const int co0 = 64 * cot, j0 = 64 * jt, R = 3 * a.C;
  const int s0 = blockIdx.y * a.sps, s1 = s0 + a.sps < a.steps ? s0 + a.sps : a.steps;
  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long long pf = (long long)a.T * a.F;
  for (int s = s0; s < s1; ++s) {
    const long long p0 = (long long)s * 32;
#pragma unroll
    for (int j = 0; j < 2; ++j) {  // dy: 32 rows x 16 quads
      const int e = threadIdx.x + j * CT, r = e >> 4, c = (e & 15) * 4;
      const long long m = p0 + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < a.M && co0 + c < a.N) v = *(const f32x4*)(a.dy + (size_t)m * a.N + co0 + c);
      *(bf16x4*)(DYl + r * LDT + c) = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    }
    {  // x: 32 rows x 8 groups of 8 (the kt-th time tap's 3 C contiguous elements, columns j0 ..)
      const int r = threadIdx.x >> 3, j = (threadIdx.x & 7) * 8;
      const long long m = p0 + r;
      bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (m < a.M && j0 + j < R) {
        const long long b = m / pf;
        const int rr = (int)(m - b * pf), t = rr / a.F, f = rr - t * a.F;
        v = *(const bf16x8*)(a.xp + (((size_t)b * a.Tp + t + kt) * a.Fp + f) * a.C + j0 + j);
      }
      *(bf16x8*)(Xl + r * LDT + j) = v;
    }
    __syncthreads();
    const bf16x8 af = trfrag(Xl, LDT, 16 * wave, 0, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = mfma16(af, trfrag(DYl, LDT, 16 * nt, 0, lane), acc[nt]);
    __syncthreads();
  }
  float* slab = a.slabs + (size_t)blockIdx.y * a.S;
  const int j = j0 + 16 * wave + 4 * q;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int co = co0 + 16 * nt + l15;
    if (co < a.N && j < R) *(f32x4*)(slab + ((size_t)kt * a.N + co) * R + j) = acc[nt];
  }
}

// dw (torch layout) = the slabs summed in split order
__global__ __launch_bounds__(CT) void wgrad_reduce_kernel(int C, int N, int splits, size_t S,
                                                          const float* __restrict__ slabs, float* __restrict__ dw) {
  const size_t e = (size_t)blockIdx.x * CT + threadIdx.x;
  if (e >= S) return;
  float s = 0.f;
  for (int z = 0; z < splits; ++z) s += slabs[(size_t)z * S + e];
  const int R = 3 * C;
  const int j = (int)(e % R);
  const size_t r = e / R;
  const int co = (int)(r % N), kt = (int)(r / N), kf = j / C, ci = j - kf * C;
  dw[(((size_t)co * C + ci) * 3 + kt) * 3 + kf] = s;
}

// column sums of dy [M][N] (fp32): block g sums rows [g rpb, (g + 1) rpb) -> part[g][N]
__global__ __launch_bounds__(CT) void colsum_part_kernel(long long M, int N, long long rpb,
                                                         const float* __restrict__ dy, float* __restrict__ part) {
  __shared__ float red[CT];
  const int RL = CT / N, co = threadIdx.x % N, rl = threadIdx.x / N;
  const long long r0 = (long long)blockIdx.x * rpb, r1 = r0 + rpb < M ? r0 + rpb : M;
  float s = 0.f;
  if (rl < RL)
    for (long long r = r0 + rl; r < r1; r += RL) s += dy[(size_t)r * N + co];
  red[threadIdx.x] = s;
  __syncthreads();
  if (rl == 0) {
    float t = red[co];
    for (int i = 1; i < RL; ++i) t += red[co + i * N];
    part[(size_t)blockIdx.x * N + co] = t;
  }
}

__global__ __launch_bounds__(CT) void colsum_final_kernel(int G, int N, const float* __restrict__ part,
                                                          float* __restrict__ out) {
  const int c = blockIdx.x * CT + threadIdx.x;
  if (c >= N) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[(size_t)g * N + c];
  out[c] = s;
}

// ------------------------------------------------------------------ first layer (Cin = 1)
// y[b][t][f][co] = bias[co] + sum_{kt, kf} w[co][kt][kf] x[b][refl(t + kt - 1)][refl(f + kf - 1)]
__global__ __launch_bounds__(CT) void conv2d_first_fwd_kernel(int T, int F, int N, size_t nq,
                                                              const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y) {
  const int N4 = N / 4;
  for (size_t i = (size_t)blockIdx.x * CT + threadIdx.x; i < nq; i += (size_t)gridDim.x * CT) {
    const int n = (int)(i % N4) * 4;
    size_t r = i / N4;
    const int f = (int)(r % F);
    r /= F;
    const int t = (int)(r % T);
    const size_t b = r / T;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (bias) s = *(const f32x4*)(bias + n);
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
      const float* xr = x + (b * T + reflect1(t + kt - 1, T)) * F;
#pragma unroll
      for (int kf = 0; kf < 3; ++kf) {
        const float xv = xr[reflect1(f + kf - 1, F)];
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += w[(size_t)(n + u) * 9 + kt * 3 + kf] * xv;
      }
    }
    *(f32x4*)(y + i * 4) = s;
  }
}

// part[g][co][10]: the nine taps' sums and the bias sum over positions [g ppb, (g + 1) ppb)
__global__ __launch_bounds__(CT) void conv2d_first_wgrad_kernel(int T, int F, int N, long long M, long long ppb,
                                                                const float* __restrict__ dy,
                                                                const float* __restrict__ x, float* __restrict__ part) {
  extern __shared__ float red[];  // [CT][10]
  const int RL = CT / N, co = threadIdx.x % N, rl = threadIdx.x / N;
  const long long p0 = (long long)blockIdx.x * ppb, p1 = p0 + ppb < M ? p0 + ppb : M;
  float s[10];
#pragma unroll
  for (int u = 0; u < 10; ++u) s[u] = 0.f;
  const long long pf = (long long)T * F;
  if (rl < RL)
    for (long long m = p0 + rl; m < p1; m += RL) {
      const long long b = m / pf;
      const int rr = (int)(m - b * pf), t = rr / F, f = rr - t * F;
      const float g = dy[(size_t)m * N + co];
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) {
        const float* xr = x + ((size_t)b * T + reflect1(t + kt - 1, T)) * F;
#pragma unroll
        for (int kf = 0; kf < 3; ++kf) s[kt * 3 + kf] += g * xr[reflect1(f + kf - 1, F)];
      }
      s[9] += g;
    }
#pragma unroll
  for (int u = 0; u < 10; ++u) red[threadIdx.x * 10 + u] = s[u];
  __syncthreads();
  if (rl == 0) {
    for (int u = 0; u < 10; ++u) {
      float t = red[co * 10 + u];
      for (int i = 1; i < RL; ++i) t += red[(co + i * N) * 10 + u];
      part[((size_t)blockIdx.x * N + co) * 10 + u] = t;
    }
  }
}

__global__ __launch_bounds__(CT) void conv2d_first_wgrad_final_kernel(int G, int N, const float* __restrict__ part,
                                                                      float* __restrict__ dw, float* __restrict__ db) {
  const int e = blockIdx.x * CT + threadIdx.x;
  if (e >= N * 10) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[(size_t)g * N * 10 + e];
  const int co = e / 10, u = e - co * 10;
  if (u < 9) dw[co * 9 + u] = s;
  else if (db) db[co] = s;
}

// ------------------------------------------------------------------ LayerNorm(F, C) + LeakyReLU [+ pool + keep]
__global__ __launch_bounds__(CT) void ln_fwd_kernel(int T, int F, int C, int pool, float eps,
                                                    const float* __restrict__ x, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const float* __restrict__ keep,
                                                    float* __restrict__ y, float* __restrict__ mean_o,
                                                    float* __restrict__ rstd_o) {
  __shared__ float sh[4];
  const size_t row = blockIdx.x;
  const int D = F * C;
  const float* xr = x + row * D;
  float s = 0.f;
  for (int e = threadIdx.x * 4; e < D; e += CT * 4) {
    const f32x4 v = *(const f32x4*)(xr + e);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = block_sum(s, sh) / (float)D;
  s = 0.f;
  for (int e = threadIdx.x * 4; e < D; e += CT * 4) {
    const f32x4 v = *(const f32x4*)(xr + e) - mean;
    s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  }
  const float rstd = 1.f / sqrtf(block_sum(s, sh) / (float)D + eps);
  if (threadIdx.x == 0) { mean_o[row] = mean; rstd_o[row] = rstd; }
  if (!pool) {
    for (int e = threadIdx.x * 4; e < D; e += CT * 4) {
      const f32x4 v = (*(const f32x4*)(xr + e) - mean) * rstd * *(const f32x4*)(gamma + e) + *(const f32x4*)(beta + e);
      *(f32x4*)(y + row * D + e) = f32x4{lrelu(v[0]), lrelu(v[1]), lrelu(v[2]), lrelu(v[3])};
    }
  } else {
    const int Fo = F / 2, Do = Fo * C;
    const size_t b = row / T;
    for (int u = threadIdx.x * 4; u < Do; u += CT * 4) {
      const int fo = u / C, c = u - fo * C, e0 = 2 * fo * C + c, e1 = e0 + C;
      const f32x4 v0 = (*(const f32x4*)(xr + e0) - mean) * rstd * *(const f32x4*)(gamma + e0) + *(const f32x4*)(beta + e0);
      const f32x4 v1 = (*(const f32x4*)(xr + e1) - mean) * rstd * *(const f32x4*)(gamma + e1) + *(const f32x4*)(beta + e1);
      const float k = keep ? keep[b * Fo + fo] : 1.f;
      f32x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float y0 = lrelu(v0[i]), y1 = lrelu(v1[i]);
        o[i] = (y1 > y0 ? y1 : y0) * k;
      }
      *(f32x4*)(y + row * Do + u) = o;
    }
  }
}

struct LnBwd {
  int T, F, C, pool;
  const float* dy;     // [rows][F (or F / 2)][C]
  const float* x;      // [rows][F][C]
  const float* gamma;
  const float* beta;
  const float* keep;   // [B][F / 2] or null
  const float* mean;
  const float* rstd;
};

// d loss / d (pre-activation) of element e of a row, and its normalised input xh
__device__ __forceinline__ float ln_dz(const LnBwd& a, size_t row, int e, float mean, float rstd, float* xh_o) {
  const int D = a.F * a.C;
  const float* xr = a.x + row * D;
  const float xh = (xr[e] - mean) * rstd;
  *xh_o = xh;
  const float z = xh * a.gamma[e] + a.beta[e];
  float g;
  if (a.pool) {
    const int f = e / a.C, c = e - f * a.C, fo = f >> 1, Fo = a.F / 2;
    if (fo >= Fo) return 0.f;  // the odd last bin: dropped by the pool
    const int ep = (f & 1) ? e - a.C : e + a.C;
    const float zp = (xr[ep] - mean) * rstd * a.gamma[ep] + a.beta[ep];
    const float y = lrelu(z), yp = lrelu(zp);
    const bool win = (f & 1) ? (y > yp) : (y >= yp);  // a tie keeps the lower bin
    if (!win) return 0.f;
    g = a.dy[(row * Fo + fo) * a.C + c];
    if (a.keep) g *= a.keep[(row / a.T) * Fo + fo];
  } else {
    g = a.dy[row * D + e];
  }
  return g * (z > 0.f ? 1.f : MLVAE_NEG_SLOPE);
}

__global__ __launch_bounds__(CT) void ln_bwd_dx_kernel(LnBwd a, float* __restrict__ dx) {
  __shared__ float sh[4];
  const size_t row = blockIdx.x;
  const int D = a.F * a.C;
  const float mean = a.mean[row], rstd = a.rstd[row];
  float s1 = 0.f, s2 = 0.f;
  for (int e = threadIdx.x; e < D; e += CT) {
    float xh;
    const float dxh = ln_dz(a, row, e, mean, rstd, &xh) * a.gamma[e];
    dx[row * D + e] = dxh;  // read back by this thread below
    s1 += dxh;
    s2 += dxh * xh;
  }
  const float m1 = block_sum(s1, sh) / (float)D;
  const float m2 = block_sum(s2, sh) / (float)D;
  for (int e = threadIdx.x; e < D; e += CT) {
    const float xh = (a.x[row * D + e] - mean) * rstd;
    dx[row * D + e] = rstd * (dx[row * D + e] - m1 - xh * m2);
  }
}

// part[z][0][e] = sum over the split's rows (in row order) of dz xh, part[z][1][e] of dz
__global__ __launch_bounds__(CT) void ln_bwd_param_kernel(LnBwd a, size_t rows, size_t rps, float* __restrict__ part) {
  const int D = a.F * a.C, e = blockIdx.x * CT + threadIdx.x;
  if (e >= D) return;
  const size_t r0 = blockIdx.y * rps, r1 = r0 + rps < rows ? r0 + rps : rows;
  float dg = 0.f, db = 0.f;
  for (size_t r = r0; r < r1; ++r) {
    float xh;
    const float dz = ln_dz(a, r, e, a.mean[r], a.rstd[r], &xh);
    dg += dz * xh;
    db += dz;
  }
  part[((size_t)blockIdx.y * 2) * D + e] = dg;
  part[((size_t)blockIdx.y * 2 + 1) * D + e] = db;
}

__global__ __launch_bounds__(CT) void ln_bwd_param_final_kernel(int D, int Z, const float* __restrict__ part,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int e = blockIdx.x * CT + threadIdx.x;
  if (e >= D) return;
  float dg = 0.f, db = 0.f;
  for (int z = 0; z < Z; ++z) {
    dg += part[((size_t)z * 2) * D + e];
    db += part[((size_t)z * 2 + 1) * D + e];
  }
  dgamma[e] = dg;
  dbeta[e] = db;
}

// ------------------------------------------------------------------ time max-pool 2 (floor)
__global__ __launch_bounds__(CT) void time_pool_fwd_kernel(int T, int D4, size_t nq, const f32x4* __restrict__ x,
                                                           f32x4* __restrict__ y) {
  const int To = T / 2;
  for (size_t i = (size_t)blockIdx.x * CT + threadIdx.x; i < nq; i += (size_t)gridDim.x * CT) {
    const int d = (int)(i % D4);
    const size_t r = i / D4, b = r / To, to = r - b * To;
    const f32x4 v0 = x[(b * T + 2 * to) * D4 + d], v1 = x[(b * T + 2 * to + 1) * D4 + d];
    f32x4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = v1[u] > v0[u] ? v1[u] : v0[u];
    y[i] = o;
  }
}

__global__ __launch_bounds__(CT) void time_pool_bwd_kernel(int T, int D4, size_t nq, const f32x4* __restrict__ dy,
                                                           const f32x4* __restrict__ x, f32x4* __restrict__ dx) {
  const int To = T / 2;
  for (size_t i = (size_t)blockIdx.x * CT + threadIdx.x; i < nq; i += (size_t)gridDim.x * CT) {
    const int d = (int)(i % D4);
    const size_t r = i / D4, b = r / T, t = r - b * T, to = t >> 1;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if ((int)to < To) {  // the odd last frame is dropped
      const f32x4 v = x[i], vp = x[(b * T + (t ^ 1)) * D4 + d], g = dy[(b * To + to) * D4 + d];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool win = (t & 1) ? (v[u] > vp[u]) : (v[u] >= vp[u]);  // a tie keeps the earlier frame
        o[u] = win ? g[u] : 0.f;
      }
    }
    dx[i] = o;
  }
}

// ------------------------------------------------------------------ host side
int round_up(int v, int m) { return (v + m - 1) / m * m; }
size_t align256(size_t v) { return (v + 255) / 256 * 256; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
unsigned grid_for(size_t n) {
  size_t g = (n + CT - 1) / CT;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

bool chan_ok(int Cin, int Cout) {
  return Cin >= 16 && Cin <= 256 && Cin % 16 == 0 && Cout >= 16 && Cout <= 256 && Cout % 16 == 0;
}
bool dims_ok(int B, int T, int F) {
  return B > 0 && T >= 2 && F >= 2 && (long long)B * (T + 4) * (F + 4) < (1ll << 40);
}

size_t padded_bytes(int B, int T, int F, int C, int P) {
  return align256((size_t)B * (T + 2 * P) * (F + 2 * P) * C * sizeof(short));
}
size_t wp_bytes(int N, int C) { return align256((size_t)N * 3 * round_up(3 * C, 32) * sizeof(short)); }

int launch_pad(int B, int T, int F, int C, int P, int reflect, const float* x, short* xp, hipStream_t s) {
  const size_t nq = (size_t)B * (T + 2 * P) * (F + 2 * P) * (C / 4);
  hipLaunchKernelGGL(pad_bf16_kernel, dim3(grid_for(nq)), dim3(CT), 0, s, T, F, C, P, reflect, nq, x, xp);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

int launch_pack(int N, int C, int flip, const float* w, short* wp, hipStream_t s) {
  const int Rp = round_up(3 * C, 32);
  hipLaunchKernelGGL(pack_w_kernel, dim3(grid_for((size_t)N * 3 * Rp)), dim3(CT), 0, s, N, C, Rp, flip, w, wp);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

// y [B][Tp-2][Fp-2][N] from xp [B][Tp][Fp][C]
int launch_mfma(int B, int Tp, int Fp, int C, int N, const short* xp, const short* wp, const float* bias, float* y,
                hipStream_t s) {
  C2Args a{};
  a.Tp = Tp; a.Fp = Fp; a.C = C; a.N = N; a.To = Tp - 2; a.Fo = Fp - 2; a.Rp = round_up(3 * C, 32);
  a.M = (long long)B * a.To * a.Fo;
  a.xp = xp; a.wp = wp; a.bias = bias; a.y = y;
  if (N % 128 == 0) {  // the LDS-staged form
    hipLaunchKernelGGL(conv2d_mfma_lds_kernel, dim3((unsigned)((a.M + 127) / 128), N / 128), dim3(CT), 0, s, a);
    MLVAE_CHECK_LAUNCH();
    return 0;
  }
  // the direct form: a wave owns 16 MF positions x 16 NT channels: MF = 4 (64 positions; twice the
  // MFMAs per operand load) once that still leaves every CU a workgroup, MF = 2 below
  const int NT = N % 64 == 0 ? 4 : (N % 32 == 0 ? 2 : 1), ny = N / (16 * NT);
  const bool wide = (a.M + 255) / 256 * ny >= 256;
  const dim3 grid((unsigned)((a.M + (wide ? 255 : 127)) / (wide ? 256 : 128)), ny);
#define C2_LAUNCH(mf, nt) hipLaunchKernelGGL((conv2d_mfma_kernel<mf, nt>), grid, dim3(CT), 0, s, a)
  if (wide) {
    if (NT == 4) C2_LAUNCH(4, 4); else if (NT == 2) C2_LAUNCH(4, 2); else C2_LAUNCH(4, 1);
  } else {
    if (NT == 4) C2_LAUNCH(2, 4); else if (NT == 2) C2_LAUNCH(2, 2); else C2_LAUNCH(2, 1);
  }
#undef C2_LAUNCH
  MLVAE_CHECK_LAUNCH();
  return 0;
}

// weight-gradient splits over the positions: a function of the shape alone
void wgrad_plan(int B, int T, int F, int Cin, int Cout, int* steps, int* sps, int* splits) {
  const long long M = (long long)B * T * F;
  const int st = (int)((M + 31) / 32);
  const int tiles = 3 * ((Cout + 63) / 64) * ((3 * Cin + 63) / 64);
  int z = 2048 / tiles;
  z = z < 1 ? 1 : (z > 64 ? 64 : z);
  if (z > st) z = st;
  const int per = (st + z - 1) / z;
  *steps = st; *sps = per; *splits = (st + per - 1) / per;
}

constexpr int CS_G = 256;   // column-sum / first-layer partial blocks (at most)
int part_blocks(long long M) {
  const long long g = (M + 63) / 64;
  return (int)(g < CS_G ? g : CS_G);
}

constexpr int LN_Z = 32;    // LayerNorm parameter-gradient row splits (at most)

}  // namespace

extern "C" int mlvae_conv2d_supported(int Cin, int Cout) { return chan_ok(Cin, Cout) ? 1 : 0; }

extern "C" size_t mlvae_conv2d_workspace_size(int op, int B, int T, int F, int Cin, int Cout) {
  if (!chan_ok(Cin, Cout) || !dims_ok(B, T, F)) return 0;
  if (op == 0) return padded_bytes(B, T, F, Cin, 1) + wp_bytes(Cout, Cin);
  if (op == 1)
    return padded_bytes(B, T, F, Cout, 2) + wp_bytes(Cin, Cout) +
           align256((size_t)B * (T + 2) * (F + 2) * Cin * sizeof(float));
  int steps, sps, splits;
  wgrad_plan(B, T, F, Cin, Cout, &steps, &sps, &splits);
  return padded_bytes(B, T, F, Cin, 1) + align256((size_t)splits * 9 * Cin * Cout * sizeof(float)) +
         align256((size_t)CS_G * Cout * sizeof(float));
}

// the reflect-padded bf16 copy xp [B][T+2][F+2][C] on its own (the forward's first launch): for
// compositions over it and for timing
extern "C" int mlvae_conv2d_pad_bf16(int B, int T, int F, int C, const float* x, void* xp, void* stream) {
  if (!dims_ok(B, T, F) || C < 4 || C % 4 || !x || !xp || !aligned16(x) || !aligned16(xp)) {
    mlvae_set_error("mlvae_conv2d_pad_bf16: unsupported shape / alignment (B %d T %d F %d C %d)", B, T, F, C);
    return 1;
  }
  return launch_pad(B, T, F, C, 1, 1, x, static_cast<short*>(xp), (hipStream_t)stream);
}

#define C2_CHECK(who, cond)                                                                             \
  if (!(cond)) {                                                                                         \
    mlvae_set_error(who ": unsupported shape / alignment / workspace (B %d T %d F %d Cin %d Cout %d)", B, T, F, \
                    Cin, Cout);                                                                          \
    return 1;                                                                                            \
  }

extern "C" int mlvae_conv2d_fwd(int B, int T, int F, int Cin, int Cout, const float* x, const float* w,
                                const float* bias, float* y, void* ws, size_t ws_bytes, void* stream) {
  C2_CHECK("mlvae_conv2d_fwd", chan_ok(Cin, Cout) && dims_ok(B, T, F) && x && w && y && ws && aligned16(x) &&
                                   aligned16(y) && aligned16(ws) && (!bias || aligned16(bias)) &&
                                   ws_bytes >= mlvae_conv2d_workspace_size(0, B, T, F, Cin, Cout));
  hipStream_t s = (hipStream_t)stream;
  short* xp = static_cast<short*>(ws);
  short* wp = reinterpret_cast<short*>(static_cast<char*>(ws) + padded_bytes(B, T, F, Cin, 1));
  if (int rc = launch_pad(B, T, F, Cin, 1, 1, x, xp, s)) return rc;
  if (int rc = launch_pack(Cout, Cin, 0, w, wp, s)) return rc;
  return launch_mfma(B, T + 2, F + 2, Cin, Cout, xp, wp, bias, y, s);
}

extern "C" int mlvae_conv2d_dgrad(int B, int T, int F, int Cin, int Cout, const float* dy, const float* w, float* dx,
                                  void* ws, size_t ws_bytes, void* stream) {
  C2_CHECK("mlvae_conv2d_dgrad", chan_ok(Cin, Cout) && dims_ok(B, T, F) && dy && w && dx && ws && aligned16(dy) &&
                                     aligned16(dx) && aligned16(ws) &&
                                     ws_bytes >= mlvae_conv2d_workspace_size(1, B, T, F, Cin, Cout));
  hipStream_t s = (hipStream_t)stream;
  char* p = static_cast<char*>(ws);
  short* dyp = reinterpret_cast<short*>(p);
  p += padded_bytes(B, T, F, Cout, 2);
  short* wp = reinterpret_cast<short*>(p);
  p += wp_bytes(Cin, Cout);
  float* dxp = reinterpret_cast<float*>(p);
  if (int rc = launch_pad(B, T, F, Cout, 2, 0, dy, dyp, s)) return rc;
  if (int rc = launch_pack(Cin, Cout, 1, w, wp, s)) return rc;
  if (int rc = launch_mfma(B, T + 4, F + 4, Cout, Cin, dyp, wp, nullptr, dxp, s)) return rc;
  const size_t nq = (size_t)B * T * F * (Cin / 4);
  hipLaunchKernelGGL(fold_kernel, dim3(grid_for(nq)), dim3(CT), 0, s, T, F, Cin, nq, (const float*)dxp, dx);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_conv2d_wgrad(int B, int T, int F, int Cin, int Cout, const float* dy, const float* x, float* dw,
                                  float* db, void* ws, size_t ws_bytes, void* stream) {
  C2_CHECK("mlvae_conv2d_wgrad", chan_ok(Cin, Cout) && dims_ok(B, T, F) && dy && x && dw && ws && aligned16(dy) &&
                                     aligned16(x) && aligned16(ws) &&
                                     ws_bytes >= mlvae_conv2d_workspace_size(2, B, T, F, Cin, Cout));
  hipStream_t s = (hipStream_t)stream;
  WgArgs a{};
  int splits;
  wgrad_plan(B, T, F, Cin, Cout, &a.steps, &a.sps, &splits);
  char* p = static_cast<char*>(ws);
  short* xp = reinterpret_cast<short*>(p);
  p += padded_bytes(B, T, F, Cin, 1);
  float* slabs = reinterpret_cast<float*>(p);
  p += align256((size_t)splits * 9 * Cin * Cout * sizeof(float));
  float* part = reinterpret_cast<float*>(p);
  if (int rc = launch_pad(B, T, F, Cin, 1, 1, x, xp, s)) return rc;
  a.T = T; a.F = F; a.C = Cin; a.N = Cout; a.Tp = T + 2; a.Fp = F + 2;
  a.nCo = (Cout + 63) / 64; a.nJ = (3 * Cin + 63) / 64;
  a.M = (long long)B * T * F;
  a.dy = dy; a.xp = xp; a.slabs = slabs; a.S = (size_t)9 * Cin * Cout;
  hipLaunchKernelGGL(conv2d_wgrad_kernel, dim3(3 * a.nCo * a.nJ, splits), dim3(CT), 0, s, a);
  MLVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((a.S + CT - 1) / CT)), dim3(CT), 0, s, Cin, Cout, splits,
                     a.S, (const float*)slabs, dw);
  MLVAE_CHECK_LAUNCH();
  if (db) {
    const int G = part_blocks(a.M);
    const long long rpb = (a.M + G - 1) / G;
    hipLaunchKernelGGL(colsum_part_kernel, dim3(G), dim3(CT), 0, s, a.M, Cout, rpb, dy, part);
    MLVAE_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_final_kernel, dim3((Cout + CT - 1) / CT), dim3(CT), 0, s, G, Cout, (const float*)part,
                       db);
    MLVAE_CHECK_LAUNCH();
  }
  return 0;
}

#undef C2_CHECK

static bool first_ok(int B, int T, int F, int Cout) {
  return dims_ok(B, T, F) && Cout >= 16 && Cout <= 256 && Cout % 16 == 0;
}

extern "C" int mlvae_conv2d_first_fwd(int B, int T, int F, int Cout, const float* x, const float* w,
                                      const float* bias, float* y, void* stream) {
  if (!first_ok(B, T, F, Cout) || !x || !w || !y || !aligned16(y) || (bias && !aligned16(bias))) {
    mlvae_set_error("mlvae_conv2d_first_fwd: unsupported shape / alignment (B %d T %d F %d Cout %d)", B, T, F, Cout);
    return 1;
  }
  const size_t nq = (size_t)B * T * F * (Cout / 4);
  hipLaunchKernelGGL(conv2d_first_fwd_kernel, dim3(grid_for(nq)), dim3(CT), 0, (hipStream_t)stream, T, F, Cout, nq, x,
                     w, bias, y);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_conv2d_first_wgrad_workspace_size(int B, int T, int F, int Cout) {
  if (!first_ok(B, T, F, Cout)) return 0;
  return (size_t)CS_G * Cout * 10 * sizeof(float);
}

extern "C" int mlvae_conv2d_first_wgrad(int B, int T, int F, int Cout, const float* dy, const float* x, float* dw,
                                        float* db, void* ws, size_t ws_bytes, void* stream) {
  if (!first_ok(B, T, F, Cout) || !dy || !x || !dw || !ws ||
      ws_bytes < mlvae_conv2d_first_wgrad_workspace_size(B, T, F, Cout)) {
    mlvae_set_error("mlvae_conv2d_first_wgrad: unsupported shape / workspace (B %d T %d F %d Cout %d)", B, T, F,
                    Cout);
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  const long long M = (long long)B * T * F;
  const int G = part_blocks(M);
  const long long ppb = (M + G - 1) / G;
  float* part = static_cast<float*>(ws);
  hipLaunchKernelGGL(conv2d_first_wgrad_kernel, dim3(G), dim3(CT), CT * 10 * sizeof(float), s, T, F, Cout, M, ppb, dy,
                     x, part);
  MLVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(conv2d_first_wgrad_final_kernel, dim3((Cout * 10 + CT - 1) / CT), dim3(CT), 0, s, G, Cout,
                     (const float*)part, dw, db);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

static bool ln_ok(long long rows, int T, int F, int C, int pool) {
  return rows > 0 && T > 0 && rows % T == 0 && F >= 1 && C >= 4 && C % 4 == 0 && (long long)F * C <= (1 << 24) &&
         (!pool || F >= 2);
}

extern "C" int mlvae_ln_fc_act_fwd(long long rows, int T, int F, int C, const float* x, const float* gamma,
                                   const float* beta, const float* keep, int pool, float eps, float* y, float* mean,
                                   float* rstd, void* stream) {
  if (!ln_ok(rows, T, F, C, pool) || !x || !gamma || !beta || !y || !mean || !rstd || (keep && !pool) ||
      !aligned16(x) || !aligned16(gamma) || !aligned16(beta) || !aligned16(y)) {
    mlvae_set_error("mlvae_ln_fc_act_fwd: unsupported shape / alignment (rows %lld T %d F %d C %d pool %d)", rows, T,
                    F, C, pool);
    return 1;
  }
  hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)rows), dim3(CT), 0, (hipStream_t)stream, T, F, C, pool, eps, x,
                     gamma, beta, keep, y, mean, rstd);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_ln_fc_act_bwd_workspace_size(long long rows, int F, int C) {
  if (rows <= 0 || F < 1 || C < 1) return 0;
  return (size_t)LN_Z * 2 * F * C * sizeof(float);
}

extern "C" int mlvae_ln_fc_act_bwd(long long rows, int T, int F, int C, const float* dy, const float* x,
                                   const float* gamma, const float* beta, const float* keep, int pool,
                                   const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta,
                                   void* ws, size_t ws_bytes, void* stream) {
  if (!ln_ok(rows, T, F, C, pool) || !dy || !x || !gamma || !beta || !mean || !rstd || !dx || !dgamma || !dbeta ||
      (keep && !pool) || !ws || ws_bytes < mlvae_ln_fc_act_bwd_workspace_size(rows, F, C)) {
    mlvae_set_error("mlvae_ln_fc_act_bwd: unsupported shape / workspace (rows %lld T %d F %d C %d pool %d)", rows, T,
                    F, C, pool);
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  LnBwd a{T, F, C, pool, dy, x, gamma, beta, keep, mean, rstd};
  hipLaunchKernelGGL(ln_bwd_dx_kernel, dim3((unsigned)rows), dim3(CT), 0, s, a, dx);
  MLVAE_CHECK_LAUNCH();
  const int D = F * C;
  const int Z = rows < LN_Z ? (int)rows : LN_Z;
  const size_t rps = ((size_t)rows + Z - 1) / Z;
  const int Zu = (int)(((size_t)rows + rps - 1) / rps);
  float* part = static_cast<float*>(ws);
  hipLaunchKernelGGL(ln_bwd_param_kernel, dim3((D + CT - 1) / CT, Zu), dim3(CT), 0, s, a, (size_t)rows, rps, part);
  MLVAE_CHECK_LAUNCH();
  hipLaunchKernelGGL(ln_bwd_param_final_kernel, dim3((D + CT - 1) / CT), dim3(CT), 0, s, D, Zu, (const float*)part,
                     dgamma, dbeta);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_time_pool_fwd(int B, int T, int D, const float* x, float* y, void* stream) {
  if (B <= 0 || T < 2 || D < 4 || D % 4 || !x || !y || !aligned16(x) || !aligned16(y)) {
    mlvae_set_error("mlvae_time_pool_fwd: unsupported shape / alignment (B %d T %d D %d)", B, T, D);
    return 1;
  }
  const size_t nq = (size_t)B * (T / 2) * (D / 4);
  hipLaunchKernelGGL(time_pool_fwd_kernel, dim3(grid_for(nq)), dim3(CT), 0, (hipStream_t)stream, T, D / 4, nq,
                     (const f32x4*)x, (f32x4*)y);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_time_pool_bwd(int B, int T, int D, const float* dy, const float* x, float* dx, void* stream) {
  if (B <= 0 || T < 2 || D < 4 || D % 4 || !dy || !x || !dx || !aligned16(dy) || !aligned16(x) || !aligned16(dx)) {
    mlvae_set_error("mlvae_time_pool_bwd: unsupported shape / alignment (B %d T %d D %d)", B, T, D);
    return 1;
  }
  const size_t nq = (size_t)B * T * (D / 4);
  hipLaunchKernelGGL(time_pool_bwd_kernel, dim3(grid_for(nq)), dim3(CT), 0, (hipStream_t)stream, T, D / 4, nq,
                     (const f32x4*)dy, (const f32x4*)x, (f32x4*)dx);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
