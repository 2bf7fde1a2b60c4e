// The LSTM_FC baseline's frame-level MD head (ref:src/models/LSTM_FC/model.py:29-67) on gfx950:
// everything after the FCBlock's last hidden layer, for N = B T frames of E features.
//
//   flvl_fwd_kernel     logits = h w^T + bias (two classes), the class-weighted BCE-with-logits
//                       against [1 - label, label] per frame and class (padded frames too: the
//                       masked mean drops them), the predicted label x1 > x0 (-1 past the
//                       utterance's length) and the four MD counts per utterance.  16 lanes share
//                       a frame: they stride its [E] row together and reduce both dot products by
//                       xor shuffles in a fixed order; the counts are integer atomics (exact in
//                       any order).
//   flvl_bwd_kernel     dlogits per frame, dh = dlogits w, and this workgroup's partial sums of
//                       dw = dlogits^T h and db, written to the workspace.
//   flvl_reduce_kernel  the partials summed over the workgroups in index order: no floating-point
//                       atomics anywhere, a rerun is bit-identical.
// At the recipe's N = 4000, E = 64 the three are launch-bound (1 MB of h each way).
#include "common.h"

namespace {

constexpr int FL_LANES = 16;               // lanes per frame (forward)
constexpr int FL_FRAMES = 256 / FL_LANES;  // frames per block (forward)
constexpr int FL_CHUNK = 256;              // frames per backward chunk: one per thread
constexpr int FL_FWD_GRID = 4096;          // grid caps: 65536 frames a sweep, either way
constexpr int FL_BWD_GRID = 256;

// softplus(x) = log(1 + e^x), finite at any x
__device__ __forceinline__ float softplus_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

template <bool VEC>
__global__ __launch_bounds__(256) void flvl_fwd_kernel(
    int B, int T, int E, const float* __restrict__ h, const float* __restrict__ w,
    const float* __restrict__ bias, const float* __restrict__ labels, const float* __restrict__ lens,
    float pw0, float pw1, float2* __restrict__ logits, float2* __restrict__ loss_e,
    int* __restrict__ pred, int* __restrict__ counts, int* err) {
  const int lane = threadIdx.x % FL_LANES;
  const size_t n = (size_t)B * T;
  const float b0 = bias[0], b1 = bias[1];
  const float* w1 = w + E;
  int bad = 0;
  // a 16-lane group enters and leaves the loop together: the shuffles see all of its lanes
  for (size_t i = (size_t)blockIdx.x * FL_FRAMES + threadIdx.x / FL_LANES; i < n;
       i += (size_t)gridDim.x * FL_FRAMES) {
    const float* row = h + i * E;
    float s0 = 0.f, s1 = 0.f;
    if (VEC) {
      const float4 *r4 = (const float4*)row, *w04 = (const float4*)w, *w14 = (const float4*)w1;
      for (int j = lane; j < E / 4; j += FL_LANES) {
        const float4 v = r4[j], a = w04[j], c = w14[j];
        s0 += (v.x * a.x + v.y * a.y) + (v.z * a.z + v.w * a.w);
        s1 += (v.x * c.x + v.y * c.y) + (v.z * c.z + v.w * c.w);
      }
    } else {
      for (int j = lane; j < E; j += FL_LANES) {
        const float v = row[j];
        s0 += v * w[j];
        s1 += v * w1[j];
      }
    }
    for (int o = FL_LANES / 2; o > 0; o >>= 1) {
      s0 += __shfl_xor(s0, o, FL_LANES);
      s1 += __shfl_xor(s1, o, FL_LANES);
    }
    if (lane == 0) {
      const float x0 = s0 + b0, x1 = s1 + b1, l = labels[i];
      const float y0 = 1.f - l, y1 = l;
      logits[i] = make_float2(x0, x1);
      loss_e[i] = make_float2(pw0 * y0 * softplus_(-x0) + (1.f - y0) * softplus_(x0),
                              pw1 * y1 * softplus_(-x1) + (1.f - y1) * softplus_(x1));
      const int b = (int)(i / (size_t)T), t = (int)(i - (size_t)b * T);
      int p = -1;
      if (t < valid_frames(lens[b], T)) {
        p = x1 > x0 ? 1 : 0;  // torch.argmax: the first maximum on a tie
        if (l != 0.f && l != 1.f) bad = MLVAE_ERR_FLVL_LABEL;
        const int g = l == 1.f ? 1 : 0;
        // md_metric_stats._counts: both correct, both mispronounced, missed, false alarm
        atomicAdd(counts + 4 * b + (p == g ? g : (g ? 2 : 3)), 1);
      }
      pred[i] = p;
    }
  }
  if (bad) atomicOr(err, bad);
}

// W = 4: E % 4 == 0 and h, w, dh 16-byte aligned, rows moved as float4; W = 1: scalar.
// Partials of workgroup g at part + g (2 E + 2): dw[0,:], dw[1,:], db[0], db[1].
template <int W>
__global__ __launch_bounds__(256) void flvl_bwd_kernel(
    size_t n, int E, const float* __restrict__ h, const float* __restrict__ w,
    const float2* __restrict__ logits, const float* __restrict__ labels,
    const float2* __restrict__ dloss_e, float pw0, float pw1, float* __restrict__ dh,
    float* __restrict__ part) {
  __shared__ float2 sdl[FL_CHUNK];          // the chunk's dlogits
  __shared__ float sred[2][256 * W];        // the row groups' dw sums
  __shared__ float2 sdb[4];
  const int tid = threadIdx.x;
  const int EW = E / W;                     // columns in units of W
  const int cols = EW < 256 ? EW : 256;     // column units per pass
  const int R = 256 / cols;                 // row groups: thread (r, jj) takes frames r, r + R, ..
  const int jj = tid % cols, r = tid / cols;
  const size_t chunks = (n + FL_CHUNK - 1) / FL_CHUNK;
  float* mine = part + (size_t)blockIdx.x * (2 * (size_t)E + 2);
  const float* w1 = w + E;
  float db0 = 0.f, db1 = 0.f;
  // one pass per 256 column units (one pass up to E = 256 W); later passes recompute dlogits
  for (int jb = 0; jb < EW; jb += cols) {
    const int ju = jb + jj;                 // this thread's column unit
    const bool own = r < R && ju < EW;
    float a0[W], a1[W];
#pragma unroll
    for (int k = 0; k < W; ++k) a0[k] = a1[k] = 0.f;
    for (size_t c = blockIdx.x; c < chunks; c += gridDim.x) {
      const size_t base = c * FL_CHUNK;
      const int nf = (int)(n - base < (size_t)FL_CHUNK ? n - base : (size_t)FL_CHUNK);
      float2 d = make_float2(0.f, 0.f);
      if (tid < nf) {
        const float2 x = logits[base + tid], g = dloss_e[base + tid];
        const float l = labels[base + tid];
        // sigma(x) and 1 - sigma(x) from e = exp(-|x|): no cancellation, exact 0 / 1 at saturation
        const float e0 = expf(-fabsf(x.x)), e1 = expf(-fabsf(x.y));
        const float hi0 = 1.f / (1.f + e0), lo0 = e0 / (1.f + e0);
        const float hi1 = 1.f / (1.f + e1), lo1 = e1 / (1.f + e1);
        const float s0 = x.x >= 0.f ? hi0 : lo0, c0 = x.x >= 0.f ? lo0 : hi0;
        const float s1 = x.y >= 0.f ? hi1 : lo1, c1 = x.y >= 0.f ? lo1 : hi1;
        const float y0 = 1.f - l, y1 = l;
        d.x = g.x * ((1.f - y0) * s0 - pw0 * y0 * c0);
        d.y = g.y * ((1.f - y1) * s1 - pw1 * y1 * c1);
      }
      __syncthreads();  // the previous chunk's readers are done with sdl
      sdl[tid] = d;
      if (jb == 0) { db0 += d.x; db1 += d.y; }
      __syncthreads();
      if (jb == 0) {  // dh = dlogits w, all columns, coalesced along the rows
        const int total = nf * EW;
        for (int idx = tid; idx < total; idx += 256) {
          const int f = idx / EW, u = idx - f * EW;
          const float2 q = sdl[f];
          if constexpr (W == 4) {
            const float4 a = ((const float4*)w)[u], b = ((const float4*)w1)[u];
            ((float4*)(dh + (base + f) * E))[u] =
                make_float4(q.x * a.x + q.y * b.x, q.x * a.y + q.y * b.y, q.x * a.z + q.y * b.z,
                            q.x * a.w + q.y * b.w);
          } else {
            dh[(base + f) * E + u] = q.x * w[u] + q.y * w1[u];
          }
        }
      }
      if (own) {  // dw: frames r, r + R, .. of the chunk, in order
        for (int f = r; f < nf; f += R) {
          const float2 q = sdl[f];
          if constexpr (W == 4) {
            const float4 v = ((const float4*)(h + (base + f) * E))[ju];
            a0[0] += q.x * v.x; a0[1] += q.x * v.y; a0[2] += q.x * v.z; a0[3] += q.x * v.w;
            a1[0] += q.y * v.x; a1[1] += q.y * v.y; a1[2] += q.y * v.z; a1[3] += q.y * v.w;
          } else {
            const float v = h[(base + f) * E + ju];
            a0[0] += q.x * v;
            a1[0] += q.y * v;
          }
        }
      }
    }
    // the R row groups' sums, added in the order r = 0, 1, ..
    __syncthreads();
#pragma unroll
    for (int k = 0; k < W; ++k) {
      sred[0][tid * W + k] = own ? a0[k] : 0.f;
      sred[1][tid * W + k] = own ? a1[k] : 0.f;
    }
    __syncthreads();
    if (r == 0 && ju < EW) {
#pragma unroll
      for (int k = 0; k < W; ++k) {
        float t0 = 0.f, t1 = 0.f;
        for (int q = 0; q < R; ++q) {
          t0 += sred[0][(q * cols + jj) * W + k];
          t1 += sred[1][(q * cols + jj) * W + k];
        }
        mine[ju * W + k] = t0;
        mine[E + ju * W + k] = t1;
      }
    }
  }
  // db: the wave's butterfly, then the four waves in order
  db0 = wave_sum(db0);
  db1 = wave_sum(db1);
  if ((tid & 63) == 0) sdb[tid >> 6] = make_float2(db0, db1);
  __syncthreads();
  if (tid == 0) {
    mine[2 * (size_t)E] = ((sdb[0].x + sdb[1].x) + sdb[2].x) + sdb[3].x;
    mine[2 * (size_t)E + 1] = ((sdb[0].y + sdb[1].y) + sdb[2].y) + sdb[3].y;
  }
}

// out[o] = sum over the G workgroups' partials, in index order; o < 2 E goes to dw, the rest to db
__global__ __launch_bounds__(256) void flvl_reduce_kernel(int G, int E, const float* __restrict__ part,
                                                          float* __restrict__ dw, float* __restrict__ db) {
  const int len = 2 * E + 2;
  for (int o = blockIdx.x * 256 + threadIdx.x; o < len; o += gridDim.x * 256) {
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * len + o];
    if (o < 2 * E) dw[o] = s; else db[o - 2 * E] = s;
  }
}

int grid_fwd(size_t n) {
  const size_t b = (n + FL_FRAMES - 1) / FL_FRAMES;
  return (int)(b > (size_t)FL_FWD_GRID ? FL_FWD_GRID : (b < 1 ? 1 : b));
}

int grid_bwd(size_t n) {
  const size_t b = (n + FL_CHUNK - 1) / FL_CHUNK;
  return (int)(b > (size_t)FL_BWD_GRID ? FL_BWD_GRID : (b < 1 ? 1 : b));
}

bool aligned16(const void* a, const void* b, const void* c) {
  return ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16 == 0;
}

}  // namespace

extern "C" size_t mlvae_flvl_head_workspace_size(int B, int T, int E) {
  if (B <= 0 || T <= 0 || E <= 0) return 0;
  return (size_t)grid_bwd((size_t)B * T) * (2 * (size_t)E + 2) * sizeof(float);
}

extern "C" int mlvae_flvl_head_fwd(int B, int T, int E, const float* h, const float* w, const float* bias,
                                   const float* labels, const float* lens, float pos_w0, float pos_w1,
                                   float* logits, float* loss_e, int* pred, int* counts, int* err,
                                   void* stream) {
  if (B < 0 || T < 0 || E <= 0) { mlvae_set_error("mlvae_flvl_head_fwd: B, T must be >= 0 and E >= 1"); return 1; }
  if (B == 0 || T == 0) return 0;
  if (!h || !w || !bias || !labels || !lens || !logits || !loss_e || !pred || !counts || !err) {
    mlvae_set_error("mlvae_flvl_head_fwd: null pointer");
    return 1;
  }
  const size_t n = (size_t)B * T;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) { mlvae_set_error("mlvae_flvl_head_fwd: memset failed: %s", hipGetErrorString(e)); return 2; }
  const bool vec = E % 4 == 0 && aligned16(h, w, h);
  auto kern = vec ? flvl_fwd_kernel<true> : flvl_fwd_kernel<false>;
  kern<<<grid_fwd(n), 256, 0, (hipStream_t)stream>>>(B, T, E, h, w, bias, labels, lens, pos_w0, pos_w1,
                                                    (float2*)logits, (float2*)loss_e, pred, counts, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_flvl_head_bwd(int B, int T, int E, const float* h, const float* w, const float* logits,
                                   const float* labels, const float* dloss_e, float pos_w0, float pos_w1,
                                   float* dh, float* dw, float* db, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (B < 0 || T < 0 || E <= 0) { mlvae_set_error("mlvae_flvl_head_bwd: B, T must be >= 0 and E >= 1"); return 1; }
  if (B == 0 || T == 0) return 0;
  if (!h || !w || !logits || !labels || !dloss_e || !dh || !dw || !db || !ws) {
    mlvae_set_error("mlvae_flvl_head_bwd: null pointer");
    return 1;
  }
  const size_t need = mlvae_flvl_head_workspace_size(B, T, E);
  if (ws_bytes < need) {
    mlvae_set_error("mlvae_flvl_head_bwd: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return 1;
  }
  const size_t n = (size_t)B * T;
  const int G = grid_bwd(n);
  const bool vec = E % 4 == 0 && aligned16(h, w, dh);
  auto kern = vec ? flvl_bwd_kernel<4> : flvl_bwd_kernel<1>;
  kern<<<G, 256, 0, (hipStream_t)stream>>>(n, E, h, w, (const float2*)logits, labels,
                                          (const float2*)dloss_e, pos_w0, pos_w1, dh, (float*)ws);
  MLVAE_CHECK_LAUNCH();
  const int rb = (2 * E + 2 + 255) / 256;
  flvl_reduce_kernel<<<rb > 64 ? 64 : rb, 256, 0, (hipStream_t)stream>>>(G, E, (const float*)ws, dw, db);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
