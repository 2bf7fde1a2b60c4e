// The wav2vec2 encoder's own kernels: the forward and, for fine-tuning above the frozen conv
// stack, its backward ("The wav2vec2 encoder").  The matrix products -- conv layers 1-6 and the positional conv as GEMMs over
// overlapping rows, QKV / out-proj / FFN -- are mlvae_gemm_bf16 / mlvae_gemm; this file holds what
// sits between them.
//
// Reference: the HuggingFace wav2vec2 architecture (stable-layer-norm family) as SpeechBrain's
// HuggingFaceWav2Vec2 wraps it, built at ref:src/models/w2v_MD_VAE/model.yaml:11-16 and called at
// ref:src/models/w2v_MD_VAE/model.py:24.  tests/w2v_ref.py restates the forward in plain torch
// and is the checker of these kernels.
//
//   stats_partial / stats_final   mean and rstd of a whole tensor (normalize_wav, output_norm):
//                                 fp64 partial sums per workgroup, folded in a fixed order
//   scale_shift_kernel            out = (x - mean) rstd (the output norm's apply pass)
//   conv0_kernel                  waveform -> [B, T0, C] channels-last: conv(Cin = 1) + bias +
//                                 LN over C + GELU, one wave per frame, weights in registers
//   rows_kernel                   y = [res +] [GELU] [LN] (x [+ bias]) per row, fp32 and/or bf16 out,
//                                 one wave per row, 16-byte accesses
//   regroup_kernel                h [B, T, C] -> zero-padded group-major [B, G, T + K, C / G]
//   attention_kernel              softmax(Q K^T) V per (utterance, head), online softmax over
//                                 streamed 32-key tiles, MFMA both products
//   attention_bwd_kernel         D = sum_k P dP, dQ (waves own queries), dK / dV (waves own keys): three
//                                 passes of one kernel, P recomputed from the forward's log-sum-exp
//   rows_bwd_kernel / _fold       the row kernel's backward, dgamma / dbeta from per-wave partial rows
//   conv0_bwd_kernel / _fold      conv0_kernel's backward: dW, dbias, dgamma, dbeta, the pre-LN activation
//                                 recomputed from the waveform, per-wave partial rows
//   pad_rows_kernel               zero guard rows around every utterance of a conv layer's output gradient
//                                 (the strided conv's input gradient is one GEMM per residue over them)
//   norm_bwd_partial/_final/_apply  the whole-tensor norm's backward
// No atomics; every reduction runs in a fixed order, so the outputs are bit-reproducible.
#include "common.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float gelu_erf(float x) {
  return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f));
}

// ------------------------------------------------------------------ whole-tensor statistics
constexpr int STATS_MAX_BLOCKS = 1024;
constexpr int STATS_PER_BLOCK = NT * 16;

int stats_blocks(size_t n) {
  size_t b = (n + STATS_PER_BLOCK - 1) / STATS_PER_BLOCK;
  if (b < 1) b = 1;
  if (b > STATS_MAX_BLOCKS) b = STATS_MAX_BLOCKS;
  return (int)b;
}

// workgroup sum of (s, q) in a fixed order; the result is valid on thread 0
__device__ __forceinline__ void block_sum2(double& s, double& q, double* sh) {
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[2 * wave] = s; sh[2 * wave + 1] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = ((sh[0] + sh[2]) + sh[4]) + sh[6];
    q = ((sh[1] + sh[3]) + sh[5]) + sh[7];
  }
}

__global__ __launch_bounds__(NT) void stats_partial(size_t n, const float* __restrict__ x,
                                                    double* __restrict__ part) {
  __shared__ double sh[8];
  double s = 0.0, q = 0.0;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const double v = (double)x[i];
    s += v;
    q += v * v;
  }
  block_sum2(s, q, sh);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = q; }
}

__global__ __launch_bounds__(NT) void stats_final(size_t n, int nb, const double* __restrict__ part,
                                                  float eps, float* __restrict__ stats) {
  __shared__ double sh[8];
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < nb; i += NT) { s += part[2 * i]; q += part[2 * i + 1]; }
  block_sum2(s, q, sh);
  if (threadIdx.x == 0) {
    const double mean = s / (double)n;
    double var = q / (double)n - mean * mean;  // biased, as F.layer_norm
    if (var < 0.0) var = 0.0;
    stats[0] = (float)mean;
    stats[1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

__global__ __launch_bounds__(NT) void scale_shift_kernel(size_t n, const float* __restrict__ x,
                                                         const float* __restrict__ stats,
                                                         float* __restrict__ out) {
  const float mean = stats[0], rstd = stats[1];
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT)
    out[i] = (x[i] - mean) * rstd;
}

// ------------------------------------------------------------------ conv layer 0
constexpr int CONV0_KMAX = 10;
constexpr int CONV0_FRAMES = 16;  // frames per wave

// lane l owns channels l CPL .. l CPL + CPL - 1 (consecutive: a lane's stores of a frame are adjacent)
template <int CPL, bool OUT_BF16>
__global__ __launch_bounds__(NT) void conv0_kernel(int B, int N, int T0, int C, int K, int stride,
                                                   const float* __restrict__ wav,
                                                   const float* __restrict__ stats,
                                                   const float* __restrict__ w,
                                                   const float* __restrict__ bias,
                                                   const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, float eps,
                                                   void* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const long long frames = (long long)B * T0;
  const long long f0 = wave * CONV0_FRAMES;
  if (f0 >= frames) return;
  float wr[CPL][CONV0_KMAX], br[CPL], gr[CPL], be[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane * CPL + i;
    const bool ok = c < C;
#pragma unroll
    for (int k = 0; k < CONV0_KMAX; ++k) wr[i][k] = (ok && k < K) ? w[(size_t)c * K + k] : 0.f;
    br[i] = ok ? bias[c] : 0.f;
    gr[i] = ok ? gamma[c] : 0.f;
    be[i] = ok ? beta[c] : 0.f;
  }
  const float mean = stats ? stats[0] : 0.f, rstd = stats ? stats[1] : 1.f;
  const float invC = 1.f / (float)C;
  const long long f1 = f0 + CONV0_FRAMES < frames ? f0 + CONV0_FRAMES : frames;
  for (long long f = f0; f < f1; ++f) {
    const int b = (int)(f / T0), t = (int)(f - (long long)b * T0);
    const float* xw = wav + (size_t)b * N + (size_t)t * stride;  // t stride + K <= N by T0's definition
    float xv[CONV0_KMAX];
#pragma unroll
    for (int k = 0; k < CONV0_KMAX; ++k) xv[k] = k < K ? (xw[k] - mean) * rstd : 0.f;
    float y[CPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < CONV0_KMAX; ++k) a = fmaf(wr[i][k], xv[k], a);
      y[i] = a + br[i];
      if (lane * CPL + i < C) s += y[i];
    }
    const float mu = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const float d = y[i] - mu;
      if (lane * CPL + i < C) q += d * d;
    }
    const float rs = 1.f / sqrtf(wave_sum(q) * invC + eps);
#pragma unroll
    for (int i = 0; i < CPL; ++i) y[i] = gelu_erf((y[i] - mu) * rs * gr[i] + be[i]);
    const size_t o = (size_t)f * C + (size_t)lane * CPL;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      if (lane * CPL + i < C) {
        if constexpr (OUT_BF16) static_cast<short*>(out)[o + i] = f2bf(y[i]);
        else static_cast<float*>(out)[o + i] = y[i];
      }
    }
  }
}

// ------------------------------------------------------------------ the row kernel
constexpr int ROWS_MAX_LN = 8;  // LN keeps a row in registers: C <= 64 lanes x 4 columns x 8

// one wave per row, lane l at the column quads l, l + 64, ...: 16-byte accesses throughout
template <bool LN>
__global__ __launch_bounds__(NT) void rows_kernel(int N, int C, const float* __restrict__ x, int ldx,
                                                  const float* __restrict__ bias,
                                                  const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float eps, int gelu,
                                                  const float* res, int ldres, float* out_f32,
                                                  short* out_bf16, int ldo) {
  const int lane = threadIdx.x & 63, C4 = C / 4;
  const long long row = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (row >= N) return;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * ldx);
  const f32x4* rr = res ? reinterpret_cast<const f32x4*>(res + (size_t)row * ldres) : nullptr;
  const f32x4* b4 = reinterpret_cast<const f32x4*>(bias);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto finish = [&](int q, f32x4 y) {
    if (gelu) {
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = gelu_erf(y[e]);
    }
    if (rr) y += rr[q];  // res may be out_f32: this thread's own quad, read before it is written
    if (out_f32) *reinterpret_cast<f32x4*>(out_f32 + (size_t)row * ldo + 4 * q) = y;
    if (out_bf16)
      *reinterpret_cast<bf16x4*>(out_bf16 + (size_t)row * ldo + 4 * q) =
          bf16x4{f2bf(y[0]), f2bf(y[1]), f2bf(y[2]), f2bf(y[3])};
  };
  if constexpr (LN) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(gamma);
    const f32x4* be4 = reinterpret_cast<const f32x4*>(beta);
    f32x4 v[ROWS_MAX_LN];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < ROWS_MAX_LN; ++i) {
      const int q = lane + 64 * i;
      v[i] = q < C4 ? xr[q] + (bias ? b4[q] : zero) : zero;
      s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float invC = 1.f / (float)C;
    const float mu = wave_sum(s) * invC;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < ROWS_MAX_LN; ++i) {
      if (lane + 64 * i < C4) {
        const f32x4 d = v[i] - mu;
        sq += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
      }
    }
    const float rs = 1.f / sqrtf(wave_sum(sq) * invC + eps);
#pragma unroll
    for (int i = 0; i < ROWS_MAX_LN; ++i) {
      const int q = lane + 64 * i;
      if (q < C4) finish(q, (v[i] - mu) * rs * g4[q] + be4[q]);
    }
  } else {
    for (int q = lane; q < C4; q += 64) finish(q, xr[q] + (bias ? b4[q] : zero));
  }
}

// ------------------------------------------------------------------ positional-conv regroup
template <bool OUT_BF16>
__global__ __launch_bounds__(NT) void regroup_kernel(int B, int T, int C, int G, int K,
                                                     const float* __restrict__ h, void* __restrict__ out) {
  const int Cg = C / G, TP = T + K, pad = K / 2;
  const size_t n = (size_t)B * G * TP * Cg;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const int c = (int)(i % Cg);
    size_t r = i / Cg;
    const int tp = (int)(r % TP);
    r /= TP;
    const int g = (int)(r % G), b = (int)(r / G);
    const int t = tp - pad;
    const float v = (t >= 0 && t < T) ? h[((size_t)b * T + t) * C + (size_t)g * Cg + c] : 0.f;
    if constexpr (OUT_BF16) static_cast<short*>(out)[i] = f2bf(v);
    else static_cast<float*>(out)[i] = v;
  }
}

// ------------------------------------------------------------------ attention
// One wave per 16 queries of one (utterance, head); no LDS.  Transposed products keep everything
// lane-local: S^T = K Q^T puts a query in a lane column (C layout: col = lane & 15 = the query,
// row = 4 (lane >> 4) + r = the key), so the online max / sum of a query is an in-register fold
// plus two lane exchanges (xor 16, 32), and the probabilities of the four keys a lane holds are
// already a B-operand slice of O^T = V^T P^T once the keys of the product's K dimension are taken
// in the order the lanes hold them (V^T's rows are read in the same order).
template <bool IN_BF16> struct QkvT;
template <> struct QkvT<true> { typedef short T; };
template <> struct QkvT<false> { typedef float T; };

__device__ __forceinline__ float ld_f(const short* p) { return bf2f(*p); }
__device__ __forceinline__ float ld_f(const float* p) { return *p; }

template <int D, bool F32MATH, bool IN_BF16, bool OUT_BF16, bool LSE = false>
__global__ __launch_bounds__(NT) void attention_kernel(int T, int H, const void* __restrict__ qkv_,
                                                       float scale, void* __restrict__ out_,
                                                       float* __restrict__ lse = nullptr) {
  typedef typename QkvT<IN_BF16>::T ET;
  const ET* qkv = static_cast<const ET*>(qkv_);
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const int q0 = (blockIdx.x * (NT / 64) + (threadIdx.x >> 6)) * 16;
  if (q0 >= T) return;
  const int h = blockIdx.y, b = blockIdx.z;
  const size_t ld = (size_t)3 * H * D;
  const ET* base = qkv + (size_t)b * T * ld + (size_t)h * D;
  const ET* Kb = base + (size_t)H * D;
  const ET* Vb = base + (size_t)2 * H * D;
  const int qi = q0 + col, qc = qi < T ? qi : T - 1;
  constexpr int DB = D / 16;
  f32x4 acc[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, lsum = 0.f;

  // the query operand (B of S^T = K Q^T), kept for the whole key loop
  constexpr int NQ = F32MATH ? D / 4 : D / 32;
  float qf[F32MATH ? NQ : 1];
  bf16x8 qb[F32MATH ? 1 : NQ];
  if constexpr (F32MATH) {
#pragma unroll
    for (int c = 0; c < NQ; ++c) qf[c] = ld_f(base + (size_t)qc * ld + 4 * c + g);
  } else {
#pragma unroll
    for (int c = 0; c < NQ; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) qb[c][j] = f2bf(ld_f(base + (size_t)qc * ld + 32 * c + 8 * g + j));
  }

  for (int kt = 0; kt < T; kt += 32) {
    f32x4 s[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      s[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int kk = kt + 16 * blk + col, kc = kk < T ? kk : T - 1;
      const ET* kr = Kb + (size_t)kc * ld;
      if constexpr (F32MATH) {
#pragma unroll
        for (int c = 0; c < NQ; ++c)
          s[blk] = __builtin_amdgcn_mfma_f32_16x16x4f32(ld_f(kr + 4 * c + g), qf[c], s[blk], 0, 0, 0);
      } else {
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          bf16x8 kf;
          if constexpr (IN_BF16) {
            kf = *reinterpret_cast<const bf16x8*>(kr + 32 * c + 8 * g);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) kf[j] = f2bf(ld_f(kr + 32 * c + 8 * g + j));
          }
          s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qb[c], s[blk], 0, 0, 0);
        }
      }
    }
    // mask the keys past T, fold the tile into the running max / sum
    float mx = -INFINITY;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt + 16 * blk + 4 * g + r;
        const float v = key < T ? s[blk][r] * scale : -INFINITY;
        s[blk][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);  // finite: key kt < T is in every tile
    const float resc = expf(m - mn);  // 0 on the first tile (m = -inf)
    float ps = 0.f;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = expf(s[blk][r] - mn);  // exp(-inf) = 0 for a masked key
        s[blk][r] = p;
        ps += p;
      }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    lsum = lsum * resc + ps;
    m = mn;
#pragma unroll
    for (int i = 0; i < DB; ++i) acc[i] *= resc;

    // O^T += V^T P^T over the tile's 32 keys, in the lanes' key order
    if constexpr (F32MATH) {
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kt + 16 * blk + 4 * g + r, kc = key < T ? key : T - 1;
          const ET* vr = Vb + (size_t)kc * ld;
#pragma unroll
          for (int i = 0; i < DB; ++i)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ld_f(vr + 16 * i + col), s[blk][r], acc[i], 0, 0, 0);
        }
    } else {
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = f2bf(s[j >> 2][j & 3]);
#pragma unroll
      for (int i = 0; i < DB; ++i) {
        bf16x8 vf;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int key = kt + 16 * (j >> 2) + 4 * g + (j & 3), kc = key < T ? key : T - 1;
          vf[j] = f2bf(ld_f(Vb + (size_t)kc * ld + 16 * i + col));
        }
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[i], 0, 0, 0);
      }
    }
  }
  if (qi < T) {
    // training: the query's log-sum-exp [B, H, T], what the backward recomputes P from
    if constexpr (LSE) {
      if (g == 0) lse[((size_t)b * H + h) * T + qi] = m + logf(lsum);
    }
    const float inv = 1.f / lsum;
    const size_t o = ((size_t)b * T + qi) * ((size_t)H * D) + (size_t)h * D;
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float y = acc[i][r] * inv;
        const size_t e = o + 16 * i + 4 * g + r;
        if constexpr (OUT_BF16) static_cast<short*>(out_)[e] = f2bf(y);
        else static_cast<float*>(out_)[e] = y;
      }
  }
}

template <int D, bool LSE>
void launch_attention(dim3 grid, hipStream_t st, int T, int H, const void* qkv, int in_bf16, int f32math,
                      float scale, void* out, int out_bf16, float* lse) {
#define W2V_ATT(F, I, O) attention_kernel<D, F, I, O, LSE><<<grid, NT, 0, st>>>(T, H, qkv, scale, out, lse)
  if (f32math) {
    if (in_bf16) {
      if (out_bf16) W2V_ATT(true, true, true);
      else W2V_ATT(true, true, false);
    } else {
      if (out_bf16) W2V_ATT(true, false, true);
      else W2V_ATT(true, false, false);
    }
  } else {
    if (in_bf16) {
      if (out_bf16) W2V_ATT(false, true, true);
      else W2V_ATT(false, true, false);
    } else {
      if (out_bf16) W2V_ATT(false, false, true);
      else W2V_ATT(false, false, false);
    }
  }
#undef W2V_ATT
}

unsigned stream_grid(size_t n) {
  size_t g = (n + NT - 1) / NT;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// ------------------------------------------------------------------ attention backward
// Three passes of ONE kernel, no atomics.  A wave owns 16 rows (lane column = the row) and streams
// the other side in tiles of 32, exactly as the forward streams keys:
//   MODE 0: owns queries, streams keys:    D[q] = sum_k P dP  (= rowsum(dO o O), once per query)
//   MODE 1: owns queries, streams keys:    dQ^T += K^T dS^T
//   MODE 2: owns keys,    streams queries: dK^T += Q^T dS,  dV^T += dO^T P
// D is summed from the recomputed probabilities, not from the stored output: with a bf16 O the
// stored product leaves rowsum(dS) = sum_k P dP - D at 2^-9 of its terms instead of 0, which
// reaches every gradient that cancels over the keys (k_proj.bias's is identically zero).
// Per tile both products S = (other)(own)^T and dP = (other')(own')^T land in the C layout
// (row = the streamed index 4 (lane >> 4) + r, col = the owned index), P = exp(scale S - lse[q]) is
// recomputed, dS = P (dP - D[q]), and the four values a lane holds are a B-operand slice of the
// accumulating product once its K dimension is taken in the lanes' order (as the forward's P V).
template <int D, bool F32MATH, bool IN_BF16, int MODE>
__global__ __launch_bounds__(NT) void attention_bwd_kernel(int T, int H, const void* __restrict__ qkv_,
                                                           const void* __restrict__ dout_,
                                                           const float* __restrict__ lse, float* delta,
                                                           float scale, void* __restrict__ dqkv_) {
  typedef typename QkvT<IN_BF16>::T ET;
  constexpr bool KV = MODE == 2;
  const ET* qkv = static_cast<const ET*>(qkv_);
  const int lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
  const int o0 = (blockIdx.x * (NT / 64) + (threadIdx.x >> 6)) * 16;
  if (o0 >= T) return;
  const int h = blockIdx.y, b = blockIdx.z;
  const size_t ld = (size_t)3 * H * D, ldo = (size_t)H * D;
  const ET* Qb = qkv + (size_t)b * T * ld + (size_t)h * D;
  const ET* Kb = Qb + (size_t)H * D;
  const ET* Vb = Qb + (size_t)2 * H * D;
  const ET* dOb = static_cast<const ET*>(dout_) + (size_t)b * T * ldo + (size_t)h * D;
  const float* lse_bh = lse + ((size_t)b * H + h) * T;
  float* del_bh = delta + ((size_t)b * H + h) * T;
  // own (B operands, kept) and streamed (A operands) sides
  const ET* own1 = KV ? Kb : Qb;
  const ET* own2 = KV ? Vb : dOb;
  const size_t ldw2 = KV ? ld : ldo;
  const ET* oth1 = KV ? Qb : Kb;
  const ET* oth2 = KV ? dOb : Vb;
  const size_t ldt2 = KV ? ldo : ld;
  const int oi = o0 + col, oc = oi < T ? oi : T - 1;
  constexpr int DB = D / 16;
  f32x4 acc1[DB], acc2[KV ? DB : 1];
#pragma unroll
  for (int i = 0; i < DB; ++i) acc1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < (KV ? DB : 1); ++i) acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int NQ = F32MATH ? D / 4 : D / 32;
  float w1f[F32MATH ? NQ : 1], w2f[F32MATH ? NQ : 1];
  bf16x8 w1b[F32MATH ? 1 : NQ], w2b[F32MATH ? 1 : NQ];
  if constexpr (F32MATH) {
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
      w1f[c] = ld_f(own1 + (size_t)oc * ld + 4 * c + g);
      w2f[c] = ld_f(own2 + (size_t)oc * ldw2 + 4 * c + g);
    }
  } else {
#pragma unroll
    for (int c = 0; c < NQ; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w1b[c][j] = f2bf(ld_f(own1 + (size_t)oc * ld + 32 * c + 8 * g + j));
        w2b[c][j] = f2bf(ld_f(own2 + (size_t)oc * ldw2 + 32 * c + 8 * g + j));
      }
  }
  float own_lse = 0.f, own_del = 0.f, dsum = 0.f;
  if constexpr (!KV) own_lse = lse_bh[oc];
  if constexpr (MODE == 1) own_del = del_bh[oc];

  for (int xt = 0; xt < T; xt += 32) {
    f32x4 s[2], dp[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      s[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int xx = xt + 16 * blk + col, xc = xx < T ? xx : T - 1;
      const ET* r1 = oth1 + (size_t)xc * ld;
      const ET* r2 = oth2 + (size_t)xc * ldt2;
      if constexpr (F32MATH) {
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          s[blk] = __builtin_amdgcn_mfma_f32_16x16x4f32(ld_f(r1 + 4 * c + g), w1f[c], s[blk], 0, 0, 0);
          dp[blk] = __builtin_amdgcn_mfma_f32_16x16x4f32(ld_f(r2 + 4 * c + g), w2f[c], dp[blk], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int c = 0; c < NQ; ++c) {
          bf16x8 f1, f2;
          if constexpr (IN_BF16) {
            f1 = *reinterpret_cast<const bf16x8*>(r1 + 32 * c + 8 * g);
            f2 = *reinterpret_cast<const bf16x8*>(r2 + 32 * c + 8 * g);
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              f1[j] = f2bf(ld_f(r1 + 32 * c + 8 * g + j));
              f2[j] = f2bf(ld_f(r2 + 32 * c + 8 * g + j));
            }
          }
          s[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f1, w1b[c], s[blk], 0, 0, 0);
          dp[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f2, w2b[c], dp[blk], 0, 0, 0);
        }
      }
    }
    // P and dS of the tile; a streamed row past T contributes nothing
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = xt + 16 * blk + 4 * g + r, xc = x < T ? x : T - 1;
        float l = own_lse, dl = own_del;
        if constexpr (KV) { l = lse_bh[xc]; dl = del_bh[xc]; }
        const float p = x < T ? expf(s[blk][r] * scale - l) : 0.f;
        s[blk][r] = p;
        if constexpr (MODE == 0) dsum = fmaf(p, dp[blk][r], dsum);
        dp[blk][r] = p * (dp[blk][r] - dl);
      }
    if constexpr (MODE == 0) continue;
    if constexpr (F32MATH) {
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int x = xt + 16 * blk + 4 * g + r, xc = x < T ? x : T - 1;
#pragma unroll
          for (int i = 0; i < DB; ++i) {
            acc1[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ld_f(oth1 + (size_t)xc * ld + 16 * i + col),
                                                           dp[blk][r], acc1[i], 0, 0, 0);
            if constexpr (KV)
              acc2[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ld_f(oth2 + (size_t)xc * ldt2 + 16 * i + col),
                                                             s[blk][r], acc2[i], 0, 0, 0);
          }
        }
    } else {
      bf16x8 dsf, pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dsf[j] = f2bf(dp[j >> 2][j & 3]);
        pf[j] = f2bf(s[j >> 2][j & 3]);
      }
#pragma unroll
      for (int i = 0; i < DB; ++i) {
        bf16x8 a1, a2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int x = xt + 16 * (j >> 2) + 4 * g + (j & 3), xc = x < T ? x : T - 1;
          a1[j] = f2bf(ld_f(oth1 + (size_t)xc * ld + 16 * i + col));
          if constexpr (KV) a2[j] = f2bf(ld_f(oth2 + (size_t)xc * ldt2 + 16 * i + col));
        }
        acc1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, dsf, acc1[i], 0, 0, 0);
        if constexpr (KV) acc2[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, pf, acc2[i], 0, 0, 0);
      }
    }
  }
  if constexpr (MODE == 0) {  // the lanes of a column hold its keys 4 g + r of every tile: fold the four groups
    dsum += __shfl_xor(dsum, 16, 64);
    dsum += __shfl_xor(dsum, 32, 64);
    if (g == 0 && oi < T) del_bh[oi] = dsum;
    return;
  }
  if (oi < T) {
    // dQ (section 0) or dK (1) carry the logits' scale; dV (2) does not
    const size_t o = ((size_t)b * T + oi) * ld + (size_t)h * D + (KV ? (size_t)H * D : 0);
#pragma unroll
    for (int i = 0; i < DB; ++i) {
      const size_t e = o + 16 * i + 4 * g;
      const f32x4 y1 = acc1[i] * scale;
      if constexpr (IN_BF16) {
        *reinterpret_cast<bf16x4*>(static_cast<short*>(dqkv_) + e) =
            bf16x4{f2bf(y1[0]), f2bf(y1[1]), f2bf(y1[2]), f2bf(y1[3])};
        if constexpr (KV)
          *reinterpret_cast<bf16x4*>(static_cast<short*>(dqkv_) + e + (size_t)H * D) =
              bf16x4{f2bf(acc2[i][0]), f2bf(acc2[i][1]), f2bf(acc2[i][2]), f2bf(acc2[i][3])};
      } else {
        *reinterpret_cast<f32x4*>(static_cast<float*>(dqkv_) + e) = y1;
        if constexpr (KV) *reinterpret_cast<f32x4*>(static_cast<float*>(dqkv_) + e + (size_t)H * D) = acc2[i];
      }
    }
  }
}

template <int D, int MODE>
void launch_attention_bwd(dim3 grid, hipStream_t st, int T, int H, const void* qkv, const void* dout,
                          const float* lse, float* delta, int bf16, int f32math, float scale, void* dqkv) {
#define W2V_ATTB(F, I) \
  attention_bwd_kernel<D, F, I, MODE><<<grid, NT, 0, st>>>(T, H, qkv, dout, lse, delta, scale, dqkv)
  if (f32math) {
    if (bf16) W2V_ATTB(true, true);
    else W2V_ATTB(true, false);
  } else {
    if (bf16) W2V_ATTB(false, true);
    else W2V_ATTB(false, false);
  }
#undef W2V_ATTB
}

// ------------------------------------------------------------------ the row kernel's backward
__device__ __forceinline__ float gelu_erf_grad(float x) {
  return 0.5f * (1.f + erff(x * 0.70710678118654752440f)) +
         x * 0.39894228040143267794f * expf(-0.5f * x * x);
}

// every wave writes a partial dgamma / dbeta row and rows_bwd_fold walks them with 2 C / 256
// workgroups: more waves cost more in the fold than they save here (256 workgroups uncapped without
// LN measured 13.99 ms per forward + backward at the large sizes against 9.70 ms with this cap)
constexpr int ROWS_BWD_MAX_BLOCKS = 128;

int rows_bwd_blocks(int N) {
  int b = (N + NT / 64 - 1) / (NT / 64);
  if (b < 1) b = 1;
  if (b > ROWS_BWD_MAX_BLOCKS) b = ROWS_BWD_MAX_BLOCKS;
  return b;
}

// dx of y = [GELU] [LN] (x [+ bias]) given dy and the saved row input x; out = [acc +] dx as fp32 and
// / or bf16 (acc may be out_f32: a thread reads its own quad before writing it).  One wave per row,
// waves stride over the rows; LN: each wave keeps its dgamma / dbeta sums in registers and writes
// them as its own partial row part[wave][2][C] (every wave writes, rows or not).
template <bool LN>
__global__ __launch_bounds__(NT) void rows_bwd_kernel(int N, int C, const float* __restrict__ dy,
                                                      const float* __restrict__ x,
                                                      const float* __restrict__ bias,
                                                      const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, int gelu,
                                                      const float* acc, float* out_f32, short* out_bf16,
                                                      float* __restrict__ part) {
  const int lane = threadIdx.x & 63, C4 = C / 4;
  const int wave = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), nw = gridDim.x * (NT / 64);
  const f32x4* b4 = reinterpret_cast<const f32x4*>(bias);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  auto emit = [&](long long row, int q, f32x4 d) {
    const size_t o = (size_t)row * C + 4 * q;
    if (acc) d += *reinterpret_cast<const f32x4*>(acc + o);
    if (out_f32) *reinterpret_cast<f32x4*>(out_f32 + o) = d;
    if (out_bf16)
      *reinterpret_cast<bf16x4*>(out_bf16 + o) = bf16x4{f2bf(d[0]), f2bf(d[1]), f2bf(d[2]), f2bf(d[3])};
  };
  if constexpr (LN) {
    const f32x4* g4 = reinterpret_cast<const f32x4*>(gamma);
    const f32x4* be4 = reinterpret_cast<const f32x4*>(beta);
    f32x4 dg[ROWS_MAX_LN], db[ROWS_MAX_LN];
#pragma unroll
    for (int i = 0; i < ROWS_MAX_LN; ++i) dg[i] = db[i] = zero;
    const float invC = 1.f / (float)C;
    for (long long row = wave; row < N; row += nw) {
      const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * C);
      const f32x4* dr = reinterpret_cast<const f32x4*>(dy + (size_t)row * C);
      f32x4 v[ROWS_MAX_LN], d[ROWS_MAX_LN];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < ROWS_MAX_LN; ++i) {
        const int q = lane + 64 * i;
        v[i] = q < C4 ? xr[q] + (bias ? b4[q] : zero) : zero;
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      }
      const float mu = wave_sum(s) * invC;  // the forward's statistics, in its order
      float sq = 0.f;
#pragma unroll
      for (int i = 0; i < ROWS_MAX_LN; ++i) {
        if (lane + 64 * i < C4) {
          const f32x4 c = v[i] - mu;
          sq += (c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3]);
        }
      }
      const float rs = 1.f / sqrtf(wave_sum(sq) * invC + eps);
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < ROWS_MAX_LN; ++i) {
        const int q = lane + 64 * i;
        if (q < C4) {
          v[i] = (v[i] - mu) * rs;  // x hat
          f32x4 dv = dr[q];
          if (gelu) {
            const f32x4 z = v[i] * g4[q] + be4[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) dv[e] *= gelu_erf_grad(z[e]);
          }
          dg[i] += dv * v[i];
          db[i] += dv;
          d[i] = dv * g4[q];
          s1 += (d[i][0] + d[i][1]) + (d[i][2] + d[i][3]);
          const f32x4 t = d[i] * v[i];
          s2 += (t[0] + t[1]) + (t[2] + t[3]);
        } else {
          d[i] = zero;
        }
      }
      const float m1 = wave_sum(s1) * invC, m2 = wave_sum(s2) * invC;
#pragma unroll
      for (int i = 0; i < ROWS_MAX_LN; ++i) {
        const int q = lane + 64 * i;
        if (q < C4) emit(row, q, (d[i] - m1 - v[i] * m2) * rs);
      }
    }
    float* pg = part + (size_t)wave * 2 * C;
#pragma unroll
    for (int i = 0; i < ROWS_MAX_LN; ++i) {
      const int q = lane + 64 * i;
      if (q < C4) {
        *reinterpret_cast<f32x4*>(pg + 4 * q) = dg[i];
        *reinterpret_cast<f32x4*>(pg + C + 4 * q) = db[i];
      }
    }
  } else {
    for (long long row = wave; row < N; row += nw) {
      const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * C);
      const f32x4* dr = reinterpret_cast<const f32x4*>(dy + (size_t)row * C);
      for (int q = lane; q < C4; q += 64) {
        f32x4 dv = dr[q];
        if (gelu) {
          const f32x4 z = xr[q] + (bias ? b4[q] : zero);
#pragma unroll
          for (int e = 0; e < 4; ++e) dv[e] *= gelu_erf_grad(z[e]);
        }
        emit(row, q, dv);
      }
    }
  }
}

// dgamma [C] | dbeta [C] = the waves' partial rows summed in wave order, one thread per column
__global__ __launch_bounds__(NT) void rows_bwd_fold(int nw, int C, const float* __restrict__ part,
                                                    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= 2 * C) return;
  double s = 0.0;  // a serial fp32 chain over up to 512 partials would round n times
  for (int w = 0; w < nw; ++w) s += (double)part[(size_t)w * 2 * C + c];
  if (c < C) dgamma[c] = (float)s;
  else dbeta[c - C] = (float)s;
}

// ------------------------------------------------------------------ conv layer 0's backward
// dW [C][K], dbias, dgamma, dbeta of conv0_kernel from the gradient at its output, nothing stored in
// between: the wave recomputes a frame's window, y = conv + bias and the LN statistics exactly as the
// forward does, goes back through GELU and LN, and keeps the CPL x K weight-gradient sums and the three
// CPL-vectors of its channels in registers over the `per` consecutive frames it walks.  Every wave
// writes its partial row part[wave][C K | C | C | C] (frames or not) and conv0_bwd_fold adds the rows
// in wave order.  There is no input gradient: the waveform carries none.
constexpr int CONV0_BWD_FRAMES = 16;  // a wave has at least this many frames before another one starts
// a partial row is (K + 3) C floats (26 KB at C = 512, K = 10), so the fold's traffic grows with the
// waves: DESIGN.md section 4, "The conv stack", has the caps this one was measured against
int conv0_bwd_max_blocks = 256;

int conv0_bwd_blocks(long long frames) {
  long long waves = (frames + CONV0_BWD_FRAMES - 1) / CONV0_BWD_FRAMES;
  long long b = (waves + NT / 64 - 1) / (NT / 64);
  if (b < 1) b = 1;
  if (b > conv0_bwd_max_blocks) b = conv0_bwd_max_blocks;
  return (int)b;
}

template <int CPL>
__global__ __launch_bounds__(NT) void conv0_bwd_kernel(int B, int N, int T0, int C, int K, int stride,
                                                       long long per, const float* __restrict__ wav,
                                                       const float* __restrict__ stats,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ bias,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps,
                                                       const float* __restrict__ dout, int vec,
                                                       float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const long long frames = (long long)B * T0;
  const long long f0 = wave * per;
  const long long f1 = f0 + per < frames ? f0 + per : frames;
  float wr[CPL][CONV0_KMAX], br[CPL], gr[CPL], be[CPL];
  float dw[CPL][CONV0_KMAX], db[CPL], dg[CPL], dbe[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane * CPL + i;
    const bool ok = c < C;
#pragma unroll
    for (int k = 0; k < CONV0_KMAX; ++k) {
      wr[i][k] = (ok && k < K) ? w[(size_t)c * K + k] : 0.f;
      dw[i][k] = 0.f;
    }
    br[i] = ok ? bias[c] : 0.f;
    gr[i] = ok ? gamma[c] : 0.f;
    be[i] = ok ? beta[c] : 0.f;
    db[i] = dg[i] = dbe[i] = 0.f;
  }
  const float mean = stats ? stats[0] : 0.f, rstd = stats ? stats[1] : 1.f;
  const float invC = 1.f / (float)C;
  // a frame's slice of dout, the one HBM stream of the kernel (channels past C: 0)
  auto fetch = [&](long long f, float* d) {
    const size_t o = (size_t)f * C + (size_t)lane * CPL;
    if constexpr (CPL % 4 == 0) {
      if (vec) {  // C % 4 == 0: a lane's quad is inside the row or wholly past it
#pragma unroll
        for (int j = 0; j < CPL / 4; ++j) {
          f32x4 q = {0.f, 0.f, 0.f, 0.f};
          if (lane * CPL + 4 * j < C) q = *reinterpret_cast<const f32x4*>(dout + o + 4 * j);
#pragma unroll
          for (int e = 0; e < 4; ++e) d[4 * j + e] = q[e];
        }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < CPL; ++i) d[i] = lane * CPL + i < C ? dout[o + i] : 0.f;
  };
  float dn[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) dn[i] = 0.f;
  if (f0 < f1) fetch(f0, dn);
  for (long long f = f0; f < f1; ++f) {
    const int b = (int)(f / T0), t = (int)(f - (long long)b * T0);
    const float* xw = wav + (size_t)b * N + (size_t)t * stride;  // t stride + K <= N by T0's definition
    // the output's gradient: this frame's was fetched a frame ago, the next one's goes out now
    float dv[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) dv[i] = dn[i];
    if (f + 1 < f1) fetch(f + 1, dn);
    // the forward again, in its order
    float xv[CONV0_KMAX];
#pragma unroll
    for (int k = 0; k < CONV0_KMAX; ++k) xv[k] = k < K ? (xw[k] - mean) * rstd : 0.f;
    float y[CPL];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < CONV0_KMAX; ++k) a = fmaf(wr[i][k], xv[k], a);
      y[i] = a + br[i];
      if (lane * CPL + i < C) s += y[i];
    }
    const float mu = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const float d = y[i] - mu;
      if (lane * CPL + i < C) q += d * d;
    }
    const float rs = 1.f / sqrtf(wave_sum(q) * invC + eps);
    // back through GELU and LN (dv of a channel past C is 0, and so is everything it feeds)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const float xh = (y[i] - mu) * rs;
      const float dz = dv[i] * gelu_erf_grad(xh * gr[i] + be[i]);
      dg[i] = fmaf(dz, xh, dg[i]);
      dbe[i] += dz;
      y[i] = xh;
      dv[i] = dz * gr[i];
      s1 += dv[i];
      s2 = fmaf(dv[i], xh, s2);
    }
    const float m1 = wave_sum(s1) * invC, m2 = wave_sum(s2) * invC;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const float dy = lane * CPL + i < C ? (dv[i] - m1 - y[i] * m2) * rs : 0.f;
      db[i] += dy;
#pragma unroll
      for (int k = 0; k < CONV0_KMAX; ++k) dw[i][k] = fmaf(dy, xv[k], dw[i][k]);
    }
  }
  float* p = part + (size_t)wave * (size_t)C * (K + 3);
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = lane * CPL + i;
    if (c < C) {
#pragma unroll
      for (int k = 0; k < CONV0_KMAX; ++k)
        if (k < K) p[(size_t)c * K + k] = dw[i][k];
      p[(size_t)C * K + c] = db[i];
      p[(size_t)C * (K + 1) + c] = dg[i];
      p[(size_t)C * (K + 2) + c] = dbe[i];
    }
  }
}

// dW [C K] | dbias [C] | dgamma [C] | dbeta [C] = the waves' partial rows summed in wave order, one
// thread per column (fp64: a serial fp32 chain over a thousand partials would round a thousand times)
__global__ __launch_bounds__(NT) void conv0_bwd_fold(int nw, int C, int K, const float* __restrict__ part,
                                                     float* __restrict__ dw, float* __restrict__ dbias,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int ncol = C * (K + 3);
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= ncol) return;
  double s = 0.0;
#pragma unroll 8
  for (int wv = 0; wv < nw; ++wv) s += (double)part[(size_t)wv * ncol + c];
  if (c < C * K) dw[c] = (float)s;
  else if (c < C * (K + 1)) dbias[c - C * K] = (float)s;
  else if (c < C * (K + 2)) dgamma[c - C * (K + 1)] = (float)s;
  else dbeta[c - C * (K + 2)] = (float)s;
}

// ------------------------------------------------------------------ guard rows for the strided conv's dgrad
// x [B, T, C] fp32 -> [B, pf + T + pa, C] (fp32 or bf16) with zero rows before and after every
// utterance: the conv layers' output gradient as the residue GEMMs of the input gradient read it
template <bool OUT_BF16>
__global__ __launch_bounds__(NT) void pad_rows_kernel(int B, int T, int C, int pf, int TP,
                                                      const float* __restrict__ x, void* __restrict__ out) {
  const int C4 = C / 4;
  const size_t n = (size_t)B * TP * C4;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const int c4 = (int)(i % C4);
    const size_t r = i / C4;
    const int tp = (int)(r % TP), b = (int)(r / TP);
    const int t = tp - pf;
    const f32x4 v = (t >= 0 && t < T) ? reinterpret_cast<const f32x4*>(x)[((size_t)b * T + t) * C4 + c4] : zero;
    if constexpr (OUT_BF16)
      reinterpret_cast<bf16x4*>(out)[i] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    else reinterpret_cast<f32x4*>(out)[i] = v;
  }
}

// ------------------------------------------------------------------ whole-tensor norm backward
__global__ __launch_bounds__(NT) void norm_bwd_partial(size_t n, const float* __restrict__ dy,
                                                       const float* __restrict__ xh,
                                                       double* __restrict__ part) {
  __shared__ double sh[8];
  double s = 0.0, q = 0.0;
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const double d = (double)dy[i];
    s += d;
    q += d * (double)xh[i];
  }
  block_sum2(s, q, sh);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = q; }
}

__global__ __launch_bounds__(NT) void norm_bwd_final(size_t n, int nb, const double* __restrict__ part,
                                                     float* __restrict__ means) {
  __shared__ double sh[8];
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < nb; i += NT) { s += part[2 * i]; q += part[2 * i + 1]; }
  block_sum2(s, q, sh);
  if (threadIdx.x == 0) {
    means[0] = (float)(s / (double)n);
    means[1] = (float)(q / (double)n);
  }
}

__global__ __launch_bounds__(NT) void norm_bwd_apply(size_t n, const float* __restrict__ dy,
                                                     const float* __restrict__ xh,
                                                     const float* __restrict__ stats,
                                                     const float* __restrict__ means,
                                                     float* __restrict__ dx) {
  const float rstd = stats[1], m1 = means[0], m2 = means[1];
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT)
    dx[i] = rstd * (dy[i] - m1 - xh[i] * m2);
}

}  // namespace

extern "C" size_t mlvae_w2v_stats_workspace_size(size_t n) {
  return (size_t)stats_blocks(n) * 2 * sizeof(double);
}

extern "C" int mlvae_w2v_tensor_stats(size_t n, const float* x, float eps, float* stats, void* ws,
                                      size_t ws_bytes, void* stream) {
  if (n == 0 || !x || !stats || !ws || ((uintptr_t)ws % 8) || ws_bytes < mlvae_w2v_stats_workspace_size(n)) {
    mlvae_set_error("w2v_tensor_stats: n=%zu needs x, stats and an 8-byte aligned workspace of %zu bytes", n,
                    mlvae_w2v_stats_workspace_size(n));
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = stats_blocks(n);
  stats_partial<<<nb, NT, 0, st>>>(n, x, static_cast<double*>(ws));
  stats_final<<<1, NT, 0, st>>>(n, nb, static_cast<const double*>(ws), eps, stats);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_scale_shift(size_t n, const float* x, const float* stats, float* out, void* stream) {
  if (!x || !stats || !out) { mlvae_set_error("w2v_scale_shift: null pointer"); return 1; }
  if (n == 0) return 0;
  scale_shift_kernel<<<stream_grid(n), NT, 0, (hipStream_t)stream>>>(n, x, stats, out);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_conv0_supported(int C, int K) { return C >= 1 && C <= 512 && K >= 1 && K <= CONV0_KMAX; }

extern "C" int mlvae_w2v_conv0(int B, int N, int T0, int C, int K, int stride, const float* wav,
                               const float* stats, const float* w, const float* bias, const float* gamma,
                               const float* beta, float eps, void* out, int out_bf16, void* stream) {
  if (!mlvae_w2v_conv0_supported(C, K) || B < 1 || stride < 1 || T0 < 1 || N < K ||
      (long long)(T0 - 1) * stride + K > N || !wav || !w || !bias || !gamma || !beta || !out) {
    mlvae_set_error("w2v_conv0: B=%d N=%d T0=%d C=%d K=%d stride=%d unsupported (C <= 512, K <= %d, "
                    "(T0 - 1) stride + K <= N)", B, N, T0, C, K, stride, CONV0_KMAX);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long frames = (long long)B * T0;
  const long long waves = (frames + CONV0_FRAMES - 1) / CONV0_FRAMES;
  const unsigned grid = (unsigned)((waves + NT / 64 - 1) / (NT / 64));
#define W2V_CONV0(CPL)                                                                                      \
  do {                                                                                                      \
    if (out_bf16) conv0_kernel<CPL, true><<<grid, NT, 0, st>>>(B, N, T0, C, K, stride, wav, stats, w, bias, \
                                                                gamma, beta, eps, out);                     \
    else conv0_kernel<CPL, false><<<grid, NT, 0, st>>>(B, N, T0, C, K, stride, wav, stats, w, bias, gamma,  \
                                                       beta, eps, out);                                     \
  } while (0)
  if (C <= 64) W2V_CONV0(1);
  else if (C <= 128) W2V_CONV0(2);
  else if (C <= 256) W2V_CONV0(4);
  else W2V_CONV0(8);
#undef W2V_CONV0
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_rows(int N, int C, const float* x, int ldx, const float* bias, const float* gamma,
                              const float* beta, float eps, int gelu, const float* res, int ldres,
                              float* out_f32, void* out_bf16, int ldo, void* stream) {
  const bool ln = gamma != nullptr;
  if (N < 0 || C < 4 || C % 4 || !x || ldx < C || ldo < C || (res && ldres < C) || (!out_f32 && !out_bf16) ||
      (ln && (!beta || C > 256 * ROWS_MAX_LN))) {
    mlvae_set_error("w2v_rows: N=%d C=%d ldx=%d ldo=%d unsupported (C %% 4 == 0, LN needs gamma and beta, "
                    "C <= %d)", N, C, ldx, ldo, 256 * ROWS_MAX_LN);
    return 1;
  }
  // 16-byte accesses: aligned rows (8 bytes for the bf16 output)
  if ((ldx % 4) || (ldo % 4) || (res && (ldres % 4)) || ((uintptr_t)out_bf16 % 8) ||
      (((uintptr_t)x | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)res |
        (uintptr_t)out_f32) % 16)) {
    mlvae_set_error("w2v_rows: buffers must be 16-byte aligned and the leading dimensions multiples of 4");
    return 1;
  }
  if (N == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)(((long long)N + NT / 64 - 1) / (NT / 64));
  if (ln) rows_kernel<true><<<grid, NT, 0, st>>>(N, C, x, ldx, bias, gamma, beta, eps, gelu, res, ldres, out_f32,
                                                 static_cast<short*>(out_bf16), ldo);
  else rows_kernel<false><<<grid, NT, 0, st>>>(N, C, x, ldx, bias, gamma, beta, eps, gelu, res, ldres, out_f32,
                                               static_cast<short*>(out_bf16), ldo);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_regroup(int B, int T, int C, int G, int K, const float* h, void* out, int out_bf16,
                                 void* stream) {
  if (B < 1 || T < 1 || C < 1 || G < 1 || K < 1 || C % G || !h || !out) {
    mlvae_set_error("w2v_regroup: B=%d T=%d C=%d G=%d K=%d unsupported (C %% G == 0)", B, T, C, G, K);
    return 1;
  }
  const size_t n = (size_t)B * (T + K) * C;
  hipStream_t st = (hipStream_t)stream;
  if (out_bf16) regroup_kernel<true><<<stream_grid(n), NT, 0, st>>>(B, T, C, G, K, h, out);
  else regroup_kernel<false><<<stream_grid(n), NT, 0, st>>>(B, T, C, G, K, h, out);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_attention_supported(int T, int H, int d) {
  return T >= 1 && H >= 1 && H <= 65535 && (d == 32 || d == 64);
}

extern "C" int mlvae_w2v_attention(int B, int T, int H, int d, const void* qkv, int qkv_bf16, int f32_math,
                                   float scale, void* out, int out_bf16, void* stream) {
  if (!mlvae_w2v_attention_supported(T, H, d) || B < 1 || B > 65535 || !qkv || !out ||
      (qkv_bf16 && ((uintptr_t)qkv % 16))) {
    mlvae_set_error("w2v_attention: B=%d T=%d H=%d d=%d unsupported (d in {32, 64}, B, H <= 65535, "
                    "16-byte aligned bf16 qkv)", B, T, H, d);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((T + 63) / 64), (unsigned)H, (unsigned)B);
  if (d == 32) launch_attention<32, false>(grid, st, T, H, qkv, qkv_bf16, f32_math, scale, out, out_bf16, nullptr);
  else launch_attention<64, false>(grid, st, T, H, qkv, qkv_bf16, f32_math, scale, out, out_bf16, nullptr);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_attention_train(int B, int T, int H, int d, const void* qkv, int qkv_bf16, int f32_math,
                                         float scale, void* out, int out_bf16, float* lse, void* stream) {
  if (!mlvae_w2v_attention_supported(T, H, d) || B < 1 || B > 65535 || !qkv || !out || !lse ||
      (qkv_bf16 && ((uintptr_t)qkv % 16))) {
    mlvae_set_error("w2v_attention_train: B=%d T=%d H=%d d=%d unsupported (d in {32, 64}, B, H <= 65535, "
                    "16-byte aligned bf16 qkv, lse required)", B, T, H, d);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((T + 63) / 64), (unsigned)H, (unsigned)B);
  if (d == 32) launch_attention<32, true>(grid, st, T, H, qkv, qkv_bf16, f32_math, scale, out, out_bf16, lse);
  else launch_attention<64, true>(grid, st, T, H, qkv, qkv_bf16, f32_math, scale, out, out_bf16, lse);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_attention_bwd(int B, int T, int H, int d, const void* qkv, const void* dout, int bf16,
                                       int f32_math, float scale, const float* lse, float* delta, void* dqkv,
                                       void* stream) {
  if (!mlvae_w2v_attention_supported(T, H, d) || B < 1 || B > 65535 || !qkv || !dout || !lse || !delta ||
      !dqkv || (((uintptr_t)qkv | (uintptr_t)dout | (uintptr_t)dqkv) % 16)) {
    mlvae_set_error("w2v_attention_bwd: B=%d T=%d H=%d d=%d unsupported (d in {32, 64}, B, H <= 65535, "
                    "16-byte aligned buffers)", B, T, H, d);
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((T + 63) / 64), (unsigned)H, (unsigned)B);
  if (d == 32) {
    launch_attention_bwd<32, 0>(grid, st, T, H, qkv, dout, lse, delta, bf16, f32_math, scale, dqkv);
    launch_attention_bwd<32, 1>(grid, st, T, H, qkv, dout, lse, delta, bf16, f32_math, scale, dqkv);
    launch_attention_bwd<32, 2>(grid, st, T, H, qkv, dout, lse, delta, bf16, f32_math, scale, dqkv);
  } else {
    launch_attention_bwd<64, 0>(grid, st, T, H, qkv, dout, lse, delta, bf16, f32_math, scale, dqkv);
    launch_attention_bwd<64, 1>(grid, st, T, H, qkv, dout, lse, delta, bf16, f32_math, scale, dqkv);
    launch_attention_bwd<64, 2>(grid, st, T, H, qkv, dout, lse, delta, bf16, f32_math, scale, dqkv);
  }
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_w2v_rows_bwd_workspace_size(int N, int C) {
  if (N < 0 || C < 0) return 0;
  return (size_t)rows_bwd_blocks(N) * (NT / 64) * 2 * (size_t)C * sizeof(float);
}

extern "C" int mlvae_w2v_rows_bwd(int N, int C, const float* dy, const float* x, const float* bias,
                                  const float* gamma, const float* beta, float eps, int gelu, const float* acc,
                                  float* out_f32, void* out_bf16, float* dgamma, float* dbeta, void* ws,
                                  size_t ws_bytes, void* stream) {
  const bool ln = gamma != nullptr;
  if (N < 0 || C < 4 || C % 4 || !dy || (!out_f32 && !out_bf16) || ((ln || gelu) && !x) ||
      (ln && (!beta || !dgamma || !dbeta || !ws || C > 256 * ROWS_MAX_LN ||
              ws_bytes < mlvae_w2v_rows_bwd_workspace_size(N, C)))) {
    mlvae_set_error("w2v_rows_bwd: N=%d C=%d unsupported (C %% 4 == 0; LN needs gamma, beta, dgamma, dbeta, "
                    "C <= %d and a workspace of %zu bytes)", N, C, 256 * ROWS_MAX_LN,
                    mlvae_w2v_rows_bwd_workspace_size(N, C));
    return 1;
  }
  if (((uintptr_t)out_bf16 % 8) ||
      (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)acc |
        (uintptr_t)out_f32 | (uintptr_t)ws) % 16)) {
    mlvae_set_error("w2v_rows_bwd: buffers must be 16-byte aligned");
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = rows_bwd_blocks(N);
  if (ln) {
    rows_bwd_kernel<true><<<nb, NT, 0, st>>>(N, C, dy, x, bias, gamma, beta, eps, gelu, acc, out_f32,
                                             static_cast<short*>(out_bf16), static_cast<float*>(ws));
    rows_bwd_fold<<<(2 * C + NT - 1) / NT, NT, 0, st>>>(nb * (NT / 64), C, static_cast<const float*>(ws), dgamma,
                                                        dbeta);
  } else if (N > 0) {
    rows_bwd_kernel<false><<<nb, NT, 0, st>>>(N, C, dy, x, bias, gamma, beta, eps, gelu, acc, out_f32,
                                              static_cast<short*>(out_bf16), nullptr);
  }
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_w2v_norm_bwd_workspace_size(size_t n) {
  return (size_t)stats_blocks(n) * 2 * sizeof(double) + 2 * sizeof(double);
}

extern "C" int mlvae_w2v_norm_bwd(size_t n, const float* dy, const float* xhat, const float* stats, float* dx,
                                  void* ws, size_t ws_bytes, void* stream) {
  if (n == 0 || !dy || !xhat || !stats || !dx || !ws || ((uintptr_t)ws % 8) ||
      ws_bytes < mlvae_w2v_norm_bwd_workspace_size(n)) {
    mlvae_set_error("w2v_norm_bwd: n=%zu needs dy, xhat, stats, dx and an 8-byte aligned workspace of %zu bytes",
                    n, mlvae_w2v_norm_bwd_workspace_size(n));
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = stats_blocks(n);
  double* part = static_cast<double*>(ws);
  float* means = reinterpret_cast<float*>(part + 2 * (size_t)nb);
  norm_bwd_partial<<<nb, NT, 0, st>>>(n, dy, xhat, part);
  norm_bwd_final<<<1, NT, 0, st>>>(n, nb, part, means);
  norm_bwd_apply<<<stream_grid(n), NT, 0, st>>>(n, dy, xhat, stats, means, dx);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_conv0_bwd_set_max_blocks(int blocks) {
  const int prev = conv0_bwd_max_blocks;
  if (blocks >= 1) conv0_bwd_max_blocks = blocks;
  return prev;
}

extern "C" size_t mlvae_w2v_conv0_bwd_workspace_size(int B, int T0, int C, int K) {
  if (B < 1 || T0 < 1 || C < 1 || K < 1) return 0;
  return (size_t)conv0_bwd_blocks((long long)B * T0) * (NT / 64) * (size_t)C * (K + 3) * sizeof(float);
}

extern "C" int mlvae_w2v_conv0_bwd(int B, int N, int T0, int C, int K, int stride, const float* wav,
                                   const float* stats, const float* w, const float* bias, const float* gamma,
                                   const float* beta, float eps, const float* dout, float* dw, float* dbias,
                                   float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (!mlvae_w2v_conv0_supported(C, K) || B < 1 || stride < 1 || T0 < 1 || N < K ||
      (long long)(T0 - 1) * stride + K > N || !wav || !w || !bias || !gamma || !beta || !dout || !dw || !dbias ||
      !dgamma || !dbeta || !ws || ((uintptr_t)ws % 4) ||
      ws_bytes < mlvae_w2v_conv0_bwd_workspace_size(B, T0, C, K)) {
    mlvae_set_error("w2v_conv0_bwd: B=%d N=%d T0=%d C=%d K=%d stride=%d unsupported (C <= 512, K <= %d, "
                    "(T0 - 1) stride + K <= N, dout and the four gradients, a workspace of %zu bytes)", B, N, T0,
                    C, K, stride, CONV0_KMAX, mlvae_w2v_conv0_bwd_workspace_size(B, T0, C, K));
    return 1;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long frames = (long long)B * T0;
  const int nb = conv0_bwd_blocks(frames), nw = nb * (NT / 64);
  const long long per = (frames + nw - 1) / nw;
  const int vec = C % 4 == 0 && (uintptr_t)dout % 16 == 0;
  float* part = static_cast<float*>(ws);
#define W2V_CONV0_BWD(CPL)                                                                                   \
  conv0_bwd_kernel<CPL><<<nb, NT, 0, st>>>(B, N, T0, C, K, stride, per, wav, stats, w, bias, gamma, beta, eps, \
                                           dout, vec, part)
  if (C <= 64) W2V_CONV0_BWD(1);
  else if (C <= 128) W2V_CONV0_BWD(2);
  else if (C <= 256) W2V_CONV0_BWD(4);
  else W2V_CONV0_BWD(8);
#undef W2V_CONV0_BWD
  conv0_bwd_fold<<<(C * (K + 3) + NT - 1) / NT, NT, 0, st>>>(nw, C, K, part, dw, dbias, dgamma, dbeta);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_w2v_pad_rows(int B, int T, int C, int pad_front, int pad_back, const float* x, void* out,
                                  int out_bf16, void* stream) {
  if (B < 1 || T < 1 || C < 4 || C % 4 || pad_front < 0 || pad_back < 0 || !x || !out ||
      (((uintptr_t)x | (uintptr_t)out) % 16)) {
    mlvae_set_error("w2v_pad_rows: B=%d T=%d C=%d pads %d / %d unsupported (C %% 4 == 0, 16-byte aligned buffers)",
                    B, T, C, pad_front, pad_back);
    return 1;
  }
  const int TP = pad_front + T + pad_back;
  const size_t n = (size_t)B * TP * (C / 4);
  hipStream_t st = (hipStream_t)stream;
  if (out_bf16) pad_rows_kernel<true><<<stream_grid(n), NT, 0, st>>>(B, T, C, pad_front, TP, x, out);
  else pad_rows_kernel<false><<<stream_grid(n), NT, 0, st>>>(B, T, C, pad_front, TP, x, out);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
