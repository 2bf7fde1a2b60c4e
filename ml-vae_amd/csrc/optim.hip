// Optimizer step and small reductions of the VAE train step.
//
//   check_gradients (SpeechBrain Brain, un-vendored; called ref:src/models/md_model.py:82):
//     non-finite loss -> skip the update; else clip_grad_norm_(params, max_grad_norm=5.0)
//   torch.optim.Adam(lr) (ref:src/models/test_vanilla_vae/model.yaml:45-47), defaults
//     betas (0.9, 0.999), eps 1e-8, no weight decay, bias-corrected; step counter on device.
//   bias gradients: deterministic column sums over the B*T rows.
//   inter-layer LSTM dropout (p = 0.15 in train mode, ref:src/models/test_vanilla_vae/model.yaml:25):
//     counter-based Philox-4x32-10 (common.h dropout_scale) keyed by (seed, element index): the
//     backward re-derives the forward mask (dgrad GEMM epilogue) instead of storing it.
#include "common.h"

namespace {

// ---------------------------------------------------------------- grad norm
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, size_t n,
                                                    double* __restrict__ partials) {
  __shared__ double sm[4];
  double acc = 0.0;
  const size_t n4 = n / 4;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 v = g4[i];
    acc += (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < n; i += 256) acc += (double)g[i] * g[i];
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

struct AdamArgs {
  float* p; float* m; float* v; const float* g;
  size_t n;
  const float* hyp;           // [coef, skip, step_size, bc2_sqrt] from adam_prologue
  float b1, b2, eps;
};

// clip coefficient, non-finite skip and bias corrections, once per step (one block):
// total = ||g||_2 from the sum-of-squares partials folded in a fixed order.
// err (optional): the persistent recurrences' hand-off timeout word -- once set, this step's
// gradients are undefined and the update is skipped like a non-finite loss's.
__global__ __launch_bounds__(256) void adam_prologue(const double* partials, int nparts,
                                                     const float* loss, const int* step, float lr,
                                                     float b1, float b2, float max_norm,
                                                     float* hyp, float* norm_out, const int* err) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += partials[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float total = (float)sqrt(red[0]);
  float coef = max_norm / (total + 1e-6f);
  coef = coef < 1.f ? coef : 1.f;  // clamp(max=1)
  if (!(total == total)) coef = total;  // a NaN norm propagates as in torch
  const int t = *step + 1;
  const double bc1 = 1.0 - pow((double)b1, (double)t);
  const double bc2 = 1.0 - pow((double)b2, (double)t);
  hyp[0] = coef;
  hyp[1] = ((loss && !isfinite(*loss)) || (err && *err != 0)) ? 1.f : 0.f;
  hyp[2] = (float)((double)lr / bc1);
  hyp[3] = (float)sqrt(bc2);
  if (norm_out) *norm_out = total;
}

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
  if (a.hyp[1] != 0.f) return;  // check_gradients: non-finite loss -> skip the update
  const float coef = a.hyp[0], step_size = a.hyp[2], bc2s = a.hyp[3];
  const float w1 = 1.f - a.b1, w2 = 1.f - a.b2;
  const size_t n4 = a.n / 4;
  f32x4* p4 = reinterpret_cast<f32x4*>(a.p);
  f32x4* m4 = reinterpret_cast<f32x4*>(a.m);
  f32x4* v4 = reinterpret_cast<f32x4*>(a.v);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(a.g);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 g = g4[i] * coef, m = m4[i], v = v4[i], p = p4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      m[e] = m[e] + w1 * (g[e] - m[e]);               // exp_avg.lerp_(grad, 1-beta1)
      v[e] = v[e] * a.b2 + w2 * g[e] * g[e];          // mul_(beta2).addcmul_(g, g, 1-beta2)
      const float denom = sqrtf(v[e]) / bc2s + a.eps;
      p[e] = p[e] + (-step_size) * (m[e] / denom);    // addcdiv_(exp_avg, denom, -step_size)
    }
    p4[i] = p; m4[i] = m; v4[i] = v;
  }
  if (blockIdx.x == 0) {
    for (size_t i = n4 * 4 + threadIdx.x; i < a.n; i += 256) {
      const float g = a.g[i] * coef;
      float m = a.m[i], v = a.v[i];
      m = m + w1 * (g - m);
      v = v * a.b2 + w2 * g * g;
      a.p[i] = a.p[i] + (-step_size) * (m / (sqrtf(v) / bc2s + a.eps));
      a.m[i] = m; a.v[i] = v;
    }
  }
}

__global__ void step_counter_kernel(const float* loss, int* step, int* nonfinite, const int* err,
                                    int* err_skips) {
  if (threadIdx.x || blockIdx.x) return;
  if (err && *err != 0) { if (err_skips) *err_skips += 1; }  // counted apart from non-finite losses
  else if (loss && !isfinite(*loss)) { if (nonfinite) *nonfinite += 1; }
  else *step += 1;
}

// clip_grad_norm_ for separately allocated grads: coef from all partials (fixed order), then
// g *= min(max_norm / (total + 1e-6), 1) on this tensor.
__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ g, size_t n,
                                                         const double* __restrict__ partials,
                                                         int nparts, float max_norm,
                                                         float* norm_out) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += partials[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float total = (float)sqrt(red[0]);
  float coef = max_norm / (total + 1e-6f);
  coef = coef < 1.f ? coef : 1.f;
  if (!(total == total)) coef = total;
  if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = total;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    g[i] *= coef;
}

// ---------------------------------------------------------------- column sums
// Block = 64 columns x a chunk of rows; 256 threads = 16 column quads x 16 row lanes, float4
// loads, fixed-order LDS fold -> part[chunk][c]; colsum_final folds the chunks in order.
template <bool BF>
__device__ __forceinline__ f32x4 load4(const void* in, size_t off) {
  if constexpr (BF) {
    const u32x2 v = *reinterpret_cast<const u32x2*>(static_cast<const unsigned short*>(in) + off);
    return f32x4{__uint_as_float(v[0] << 16), __uint_as_float(v[0] & 0xffff0000u),
                 __uint_as_float(v[1] << 16), __uint_as_float(v[1] & 0xffff0000u)};
  } else {
    return *reinterpret_cast<const f32x4*>(static_cast<const float*>(in) + off);
  }
}
template <bool BF>
__device__ __forceinline__ float load1(const void* in, size_t off) {
  if constexpr (BF) return __uint_as_float((unsigned)static_cast<const unsigned short*>(in)[off] << 16);
  else return static_cast<const float*>(in)[off];
}

// in: fp32, or bf16 (the bf16 mode's dG copy)
template <bool BF>
__global__ __launch_bounds__(256) void colsum_partial(int N, int C, const void* __restrict__ in,
                                                      int ld, int rows_per, int vec,
                                                      float* __restrict__ part) {
  __shared__ f32x4 red[16][16];
  const int cq = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int c = blockIdx.x * 64 + cq * 4;
  const int r0 = blockIdx.y * rows_per, r1 = min(N, r0 + rows_per);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    if (vec && c + 3 < C) {
      // two-level: blocks of 16 rows per thread (256 rows of the chunk) folded into acc
      for (int rb = r0 + rl; rb < r1; rb += 256) {
        f32x4 blk = {0.f, 0.f, 0.f, 0.f};
        const int re = min(r1, rb + 256);
        for (int r = rb; r < re; r += 16) blk += load4<BF>(in, (size_t)r * ld + c);
        acc += blk;
      }
    } else {
      for (int r = r0 + rl; r < r1; r += 16)
        for (int e = 0; e < 4; ++e)
          if (c + e < C) acc[e] += load1<BF>(in, (size_t)r * ld + c + e);
    }
  }
  red[rl][cq] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int q = threadIdx.x >> 2, e = threadIdx.x & 3;
    float s = 0.f;
    for (int i = 0; i < 16; ++i) s += red[i][q][e];
    const int cc = blockIdx.x * 64 + threadIdx.x;
    if (cc < C) part[(size_t)blockIdx.y * C + cc] = s;
  }
}

__global__ __launch_bounds__(256) void colsum_final(int C, int R, const float* __restrict__ part,
                                                    float* __restrict__ out, float* __restrict__ out2,
                                                    float beta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  // two-level fixed-order sum (blocks of 16 chunks): a 256-long sequential chain rounded ~4x worse
  // than the fp32 oracle's pairwise sums (round 5, fp64-anchored parity test)
  float s = 0.f;
  for (int r0 = 0; r0 < R; r0 += 16) {
    float b = 0.f;
    const int r1 = min(R, r0 + 16);
    for (int r = r0; r < r1; ++r) b += part[(size_t)r * C + c];
    s += b;
  }
  out[c] = beta != 0.f ? beta * out[c] + s : s;
  if (out2) out2[c] = out[c];
}

static int colsum_chunks(int N, int C) {
  const int cb = (C + 63) / 64;
  int R = (1024 + cb - 1) / cb;
  const int rmax = (N + 63) / 64;  // >= 64 rows per chunk
  if (R > rmax) R = rmax;
  if (R > 256) R = 256;
  if (R < 1) R = 1;
  return R;
}

// ---------------------------------------------------------------- dropout
// one thread per 4 consecutive elements: one mask quad (common.h drop_quad) gives all four
__global__ __launch_bounds__(256) void dropout_kernel(size_t n, const float* __restrict__ x,
                                                      float* __restrict__ y,
                                                      unsigned short* __restrict__ ybf,
                                                      const float* __restrict__ mask,
                                                      unsigned long long seed,
                                                      unsigned long long qoff, float p, bool vec) {
  const float keep = 1.f - p, scale = 1.f / keep;
  const size_t nq = (n + 3) / 4;
  const unsigned long long dk = drop_key(seed);
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (size_t)gridDim.x * 256) {
    unsigned long long r = 0;
    if (!mask) r = drop_quad(dk, qoff + q);  // element offset 4*qoff: the shard's first row
    if (vec && q * 4 + 3 < n) {  // 16-byte load, 16- / 8-byte stores
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + q * 4);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = xv[e] * (mask ? mask[q * 4 + e] : drop_elem_scale(r, e, keep, scale));
      if (y) *reinterpret_cast<f32x4*>(y + q * 4) = v;
      if (ybf) *reinterpret_cast<bf16x4*>(ybf + q * 4) = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      continue;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t i = q * 4 + e;
      if (i >= n) break;
      const float m = mask ? mask[i] : drop_elem_scale(r, e, keep, scale);
      const float v = x[i] * m;
      if (y) y[i] = v;
      if (ybf) ybf[i] = (unsigned short)f2bf(v);
    }
  }
}

// The same mask over the [B, T, C] rows of a data-parallel shard: element (b, t, c) is mask
// element (g(b) T + t) C + c (common.h UttMap).  Per element (its quad and lane from the global
// index): a shard's rows need not start on a quad, any C.  In place (y == x) is fine.
__global__ __launch_bounds__(256) void dropout_rows_kernel(size_t n, unsigned T, unsigned C,
                                                           const float* __restrict__ x,
                                                           float* __restrict__ y,
                                                           unsigned long long seed, UttMap m, float p) {
  const float keep = 1.f - p, scale = 1.f / keep;
  const unsigned long long dk = drop_key(seed);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t row = i / C;
    const unsigned long long e = frame_global(m, row, T) * C + (i - row * C);
    y[i] = x[i] * drop_elem_scale(drop_quad(dk, e >> 2), (int)(e & 3), keep, scale);
  }
}

int grid_for(size_t total, int cap) {
  size_t g = (total + 255) / 256;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

extern "C" int mlvae_sumsq_partials_count(size_t n) { return grid_for(n / 4 + 1, 1024); }

extern "C" int mlvae_grad_sumsq(const float* g, size_t n, double* partials, void* stream) {
  if (((uintptr_t)g & 15) != 0) { mlvae_set_error("grad_sumsq: grads must be 16-byte aligned"); return 1; }
  sumsq_kernel<<<mlvae_sumsq_partials_count(n), 256, 0, (hipStream_t)stream>>>(g, n, partials);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

// hyp: device scratch of >= 4 floats (clip coef, skip flag, step size, sqrt(bias corr 2))
extern "C" int mlvae_adam_step_ex(float* params, float* exp_avg, float* exp_avg_sq, const float* grads,
                                  size_t n, const double* partials, int nparts, const float* loss,
                                  int* step, int* nonfinite, const int* err, int* err_skips, float lr,
                                  float beta1, float beta2, float eps, float max_norm, float* norm_out,
                                  float* hyp, int advance, void* stream) {
  if (!hyp || (((uintptr_t)params | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)grads) & 15)) {
    mlvae_set_error("adam_step: needs hyp scratch and 16-byte aligned buffers");
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  if (advance >= 0)  // advance < 0: reuse hyp from an earlier call of this optimizer step
    adam_prologue<<<1, 256, 0, s>>>(partials, nparts, loss, step, lr, beta1, beta2, max_norm, hyp,
                                    norm_out, err);
  AdamArgs a;
  a.p = params; a.m = exp_avg; a.v = exp_avg_sq; a.g = grads; a.n = n; a.hyp = hyp;
  a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  adam_kernel<<<grid_for(n / 4 + 1, 2048), 256, 0, s>>>(a);
  if (advance > 0) step_counter_kernel<<<1, 64, 0, s>>>(loss, step, nonfinite, err, err_skips);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_adam_step(float* params, float* exp_avg, float* exp_avg_sq, const float* grads,
                               size_t n, const double* partials, int nparts, const float* loss,
                               int* step, int* nonfinite, float lr, float beta1, float beta2,
                               float eps, float max_norm, float* norm_out, float* hyp,
                               int advance, void* stream) {
  return mlvae_adam_step_ex(params, exp_avg, exp_avg_sq, grads, n, partials, nparts, loss, step,
                            nonfinite, nullptr, nullptr, lr, beta1, beta2, eps, max_norm, norm_out,
                            hyp, advance, stream);
}

extern "C" int mlvae_clip_scale(float* g, size_t n, const double* partials, int nparts,
                                float max_norm, float* norm_out, void* stream) {
  if (n == 0) return 0;
  clip_scale_kernel<<<grid_for(n, 512), 256, 0, (hipStream_t)stream>>>(g, n, partials, nparts,
                                                                       max_norm, norm_out);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_colsum_workspace_size(int N, int C) {
  return (size_t)colsum_chunks(N, C) * C * sizeof(float);
}

// out[c] (+= if beta) = sum_n in[n][c]; out2 (optional) receives a copy (b_ih / b_hh pairs)
extern "C" int mlvae_colsum_ex(int N, int C, const void* in, int in_bf16, int ld, float* out,
                               float* out2, float beta, float* ws, size_t ws_bytes, void* stream) {
  if (C == 0) return 0;
  const int R = colsum_chunks(N, C);
  if (!ws || ws_bytes < (size_t)R * C * sizeof(float)) { mlvae_set_error("colsum: workspace too small"); return 1; }
  const int rows_per = (N + R - 1) / R;
  const int vec = in_bf16 ? ((((uintptr_t)in & 7) == 0) && (ld % 4 == 0))
                          : ((((uintptr_t)in & 15) == 0) && (ld % 4 == 0));
  hipStream_t s = (hipStream_t)stream;
  if (in_bf16) colsum_partial<true><<<dim3((C + 63) / 64, R), 256, 0, s>>>(N, C, in, ld, rows_per, vec, ws);
  else colsum_partial<false><<<dim3((C + 63) / 64, R), 256, 0, s>>>(N, C, in, ld, rows_per, vec, ws);
  colsum_final<<<(C + 255) / 256, 256, 0, s>>>(C, R, ws, out, out2, beta);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_colsum(int N, int C, const float* in, int ld, float* out, float* out2,
                            float beta, float* ws, size_t ws_bytes, void* stream) {
  return mlvae_colsum_ex(N, C, in, 0, ld, out, out2, beta, ws, ws_bytes, stream);
}

extern "C" int mlvae_dropout_ex(size_t n, const float* x, float* y, void* y_bf16,
                                const float* mask, unsigned long long seed,
                                unsigned long long offset, float p, void* stream) {
  if (p < 0.f || p >= 1.f) { mlvae_set_error("dropout: p=%f out of range", p); return 1; }
  if (offset % 4) { mlvae_set_error("dropout: element offset %llu not a multiple of 4", offset); return 1; }
  if (!y && !y_bf16) { mlvae_set_error("dropout: no output"); return 1; }
  const bool vec = ((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)y_bf16 % 8) == 0;
  dropout_kernel<<<grid_for(n, 2048), 256, 0, (hipStream_t)stream>>>(
      n, x, y, static_cast<unsigned short*>(y_bf16), mask, seed, offset / 4, p, vec);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_dropout(size_t n, const float* x, float* y, const float* mask,
                             unsigned long long seed, float p, void* stream) {
  return mlvae_dropout_ex(n, x, y, nullptr, mask, seed, 0ull, p, stream);
}

extern "C" int mlvae_dropout_rows(int B, int T, int C, const float* x, float* y,
                                  unsigned long long seed, float p, const long long* map,
                                  void* stream) {
  if (B < 0 || T < 0 || C < 0) { mlvae_set_error("dropout_rows: B, T and C must be >= 0"); return 1; }
  if (p < 0.f || p >= 1.f) { mlvae_set_error("dropout_rows: p=%f out of range", p); return 1; }
  const size_t n = (size_t)B * T * C;
  if (n == 0) return 0;
  if (!x || !y) { mlvae_set_error("dropout_rows: null pointer"); return 1; }
  UttMap m;
  if (!utt_map_load(map, B, &m, "dropout_rows")) return 1;
  dropout_rows_kernel<<<grid_for(n, 2048), 256, 0, (hipStream_t)stream>>>(
      n, (unsigned)T, (unsigned)C, x, y, seed, m, p);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

// ---- data parallel: the step's scalars ride in the gradient all-reduce.  hdr[4] is a float
// header placed right before the flat gradient (one contiguous all-reduce with the last bucket):
// pack writes [loss3 | err != 0], unpack reads the SUMMED header back -- loss3 = the global loss
// shares, err = set when any rank's recurrence timed out (the fused Adam then skips the update on
// every rank).  One collective instead of the separate loss-sum and err-max ones.
__global__ void dp_scalars_kernel(int pack, float* hdr, float* loss3, int* err) {
  if (threadIdx.x || blockIdx.x) return;
  if (pack) {
    hdr[0] = loss3[0]; hdr[1] = loss3[1]; hdr[2] = loss3[2];
    hdr[3] = *err != 0 ? 1.f : 0.f;
  } else {
    loss3[0] = hdr[0]; loss3[1] = hdr[1]; loss3[2] = hdr[2];
    if (hdr[3] > 0.f && *err == 0) *err = 1;
  }
}
extern "C" int mlvae_dp_scalars(int pack, float* hdr, float* loss3, int* err, void* stream) {
  if (!hdr || !loss3 || !err) { mlvae_set_error("dp_scalars: null pointer"); return 1; }
  dp_scalars_kernel<<<1, 64, 0, (hipStream_t)stream>>>(pack, hdr, loss3, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
