// Per-utterance scoring of the upstream-module recipes on gfx950: the integer counts behind
// phn_acc.* (ref:src/utils/metric_stats/phn_acc_metric_stats.py:22-85) and boundary.*
// (ref:src/utils/metric_stats/boundary_metric_stats.py:58-86), and the top-k boundary frames of
// ref:src/models/test_b_ind_classifier/model.py:53-63.  The reference does all of it on the host,
// per utterance, on every batch of every stage; here one workgroup per utterance leaves
//
//   phn_acc_kernel         (flvl_correct, T_b, plvl_correct, L_b)
//   boundary_topk_kernel   pred[b, t] = 1 for the k_b largest of v[b, :T_b] (0 otherwise, -1 past T_b)
//   boundary_score_kernel  (correct, n_pred, n_target)
//
// on the device, and the stats objects rebuild the reference's scores from them once per stage
// (an fp32 mean of 0/1 values is an exact integer sum and one division).  Everything written is
// an integer: no floating-point atomics, a rerun is bit-identical.  Lengths follow
// undo_padding_tensor and mlvae_phn_bce: T_b = round(T feat_len) in fp32, half to even; nothing
// at t >= T_b or l >= L_b is read.  At the recipes' sizes (B = 8, T ~ 500) all three are
// launch-bound.
#include "common.h"

namespace {

constexpr int ST = 256;                  // threads
constexpr int SW = ST / 64;              // waves
constexpr int TOPK_MAX_T = 12288;        // frames of one row kept in LDS (48 KB of keys)

// torch.argmax's order: a NaN is the maximum, the first maximal index wins
__device__ __forceinline__ bool beats(float x, float best) {
  return best == best && (x != x || x > best);
}

// sum of v over the workgroup (every thread calls it; all get the result); sh: SW ints
__device__ __forceinline__ int block_count(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // the previous use of sh is over
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < SW; ++w) s += sh[w];
  return s;
}

__global__ __launch_bounds__(ST) void phn_acc_kernel(
    int T, int C, int L, const float* __restrict__ logits, int ldl, const float* __restrict__ feat_lens,
    const long long* __restrict__ flvl_tgt, const long long* __restrict__ plvl_tgt,
    const float* __restrict__ phn_lens, const float* __restrict__ boundary, int* __restrict__ counts,
    int* err) {
  __shared__ int sh[SW];
  __shared__ int wcnt[SW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Ti = round_len(feat_lens[b], T);
  const int Li = plvl_tgt ? round_len(phn_lens[b], L) : 0;
  const float* lg = logits + (size_t)b * T * ldl;
  const long long* ft = flvl_tgt + (size_t)b * T;
  const float* bnd = boundary + (size_t)b * T;

  // frame level: one frame per thread, the classes in a loop (any C)
  int ok = 0;
  for (int t = tid; t < Ti; t += ST) {
    const float* row = lg + (size_t)t * ldl;
    float best = row[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float x = row[c];
      if (beats(x, best)) { best = x; arg = c; }
    }
    ok += (long long)arg == ft[t];
  }
  const int flvl_correct = block_count(ok, sh);

  // phoneme level: the flags == 1 in [0, T_b) open the segments
  int plvl_correct = 0;
  if (plvl_tgt && (Ti > 0 || Li > 0)) {
    int nf = 0;
    for (int t = tid; t < Ti; t += ST) nf += bnd[t] == 1.f;
    nf = block_count(nf, sh);
    // the reference's asserts: one flag per phoneme, durations that cover [0, T_b)
    const bool good = nf == Li && Ti > 0 && bnd[0] == 1.f;
    if (!good) {
      if (tid == 0) atomicOr(err, MLVAE_ERR_SCORE_SEGMENTS);
    } else {
      const long long* pt = plvl_tgt + (size_t)b * L;
      int run = 0, hit = 0;  // run: flags before this chunk of ST frames (uniform)
      for (int base = 0; base < Ti; base += ST) {
        const int t = base + tid;
        const bool f = t < Ti && bnd[t] == 1.f;
        const unsigned long long m = __ballot(f);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SW; ++w) {
          before += w < wave ? wcnt[w] : 0;
          total += wcnt[w];
        }
        if (f) {  // this thread owns segment k = [t, next flag or T_b)
          const int k = run + before + __popcll(m & ((1ull << lane) - 1ull));
          int end = t + 1;
          while (end < Ti && bnd[end] != 1.f) ++end;
          float best = 0.f;
          int arg = 0;
          for (int c = 0; c < C; ++c) {
            float s = 0.f;  // fp32 from 0, frames in increasing t
            for (int u = t; u < end; ++u) s += lg[(size_t)u * ldl + c];
            if (c == 0 || beats(s, best)) { best = s; arg = c; }
          }
          hit += (long long)arg == pt[k];  // k < nf == L_b <= L
        }
        run += total;
        __syncthreads();  // wcnt free for the next chunk
      }
      plvl_correct = block_count(hit, sh);
    }
  }
  if (tid == 0) {
    int* o = counts + 4 * (size_t)b;
    o[0] = flvl_correct; o[1] = Ti; o[2] = plvl_correct; o[3] = Li;
  }
}

// Order of torch.topk as a 32-bit key: larger key = ranks first.  A NaN ranks above every number;
// -0 and +0 are the same value.
__device__ __forceinline__ unsigned topk_key(float x) {
  if (x != x) return 0xffffffffu;
  const unsigned u = __float_as_uint(x + 0.f);  // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // +inf -> 0xff800000 < the NaN key
}

__global__ __launch_bounds__(ST) void boundary_topk_kernel(
    int T, const float* __restrict__ v, const float* __restrict__ feat_lens,
    const float* __restrict__ fa, int* __restrict__ pred, int* __restrict__ k_out, int* err) {
  extern __shared__ unsigned keys[];  // [T_b]
  __shared__ int sh[SW];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Ti = round_len(feat_lens[b], T);
  const float* row = v + (size_t)b * T;
  const float* fr = fa + (size_t)b * T;
  int* out = pred + (size_t)b * T;
  // k_b: the ones of the whole padded row (model.py:59 sums the row)
  int k = 0;
  for (int t = tid; t < T; t += ST) k += fr[t] == 1.f;
  k = block_count(k, sh);
  for (int t = tid; t < Ti; t += ST) keys[t] = topk_key(row[t]);
  for (int t = Ti + tid; t < T; t += ST) out[t] = -1;
  if (tid == 0) {
    k_out[b] = k;
    if (k > Ti) atomicOr(err, MLVAE_ERR_SCORE_K);  // torch.topk raises; the row gets no ones
  }
  if (k > Ti) k = 0;
  __syncthreads();
  // frame i is chosen iff fewer than k frames precede it in (value descending, index ascending)
  for (int i = tid; i < Ti; i += ST) {
    int chosen = 0;
    if (k > 0) {
      const unsigned ki = keys[i];
      int ahead = 0;
      for (int j = 0; j < i; ++j) ahead += keys[j] >= ki;
      for (int j = i + 1; j < Ti; ++j) ahead += keys[j] > ki;
      chosen = ahead < k;
    }
    out[i] = chosen;
  }
}

__global__ __launch_bounds__(ST) void boundary_score_kernel(
    int T, const int* __restrict__ pred, const float* __restrict__ target,
    const float* __restrict__ feat_lens, int* __restrict__ counts) {
  __shared__ int sh[SW];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Ti = round_len(feat_lens[b], T);
  const int* p = pred + (size_t)b * T;
  const float* g = target + (size_t)b * T;
  int np = 0, ng = 0;
  for (int t = tid; t < Ti; t += ST) {
    np += p[t] == 1;
    ng += g[t] == 1.f;
  }
  np = block_count(np, sh);
  ng = block_count(ng, sh);
  if (tid != 0) return;  // no barrier below
  // the reference's two-pointer walk: predictions h and true segments [left, right] in time order,
  // right = the next true flag, T_b after the last one
  auto next_pred = [&](int t) { while (t < Ti && p[t] != 1) ++t; return t; };
  auto next_flag = [&](int t) { while (t < Ti && g[t] != 1.f) ++t; return t; };
  int correct = 0;
  if (np > 0 && ng > 0) {
    int h = next_pred(0), left = next_flag(0), right = next_flag(left + 1);
    while (left < Ti && h < Ti) {
      if (h < left) {            // before the segment: spurious
        h = next_pred(h + 1);
      } else {
        if (h <= right) {        // inside: matched
          ++correct;
          h = next_pred(h + 1);
        }                        // else past it: the segment was missed
        left = right;
        right = left < Ti ? next_flag(left + 1) : Ti;
      }
    }
  }
  int* o = counts + 3 * (size_t)b;
  o[0] = correct; o[1] = np; o[2] = ng;
}

bool zero_async(void* p, size_t bytes, void* stream, const char* who) {
  hipError_t e = hipMemsetAsync(p, 0, bytes, (hipStream_t)stream);
  if (e != hipSuccess) mlvae_set_error("%s: memset failed: %s", who, hipGetErrorString(e));
  return e == hipSuccess;
}

}  // namespace

extern "C" int mlvae_boundary_topk_max_frames(void) { return TOPK_MAX_T; }

extern "C" int mlvae_phn_acc(int B, int T, int C, int L, const float* logits, int ldl,
                             const float* feat_lens, const long long* flvl_tgt,
                             const long long* plvl_tgt, const float* phn_lens, const float* boundary,
                             int* counts, int* err, void* stream) {
  if (B < 0 || T < 0 || C < 1 || L < 0 || ldl < C) {
    mlvae_set_error("mlvae_phn_acc: B, T, L must be >= 0, C >= 1 and ldl >= C");
    return 1;
  }
  if (B == 0 || T == 0) return 0;
  if (!logits || !feat_lens || !flvl_tgt || !counts || !err || (plvl_tgt && (!phn_lens || !boundary))) {
    mlvae_set_error("mlvae_phn_acc: null pointer");
    return 1;
  }
  if (!zero_async(counts, (size_t)B * 4 * sizeof(int), stream, "mlvae_phn_acc")) return 2;
  phn_acc_kernel<<<B, ST, 0, (hipStream_t)stream>>>(T, C, L, logits, ldl, feat_lens, flvl_tgt, plvl_tgt,
                                                     phn_lens, boundary, counts, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_boundary_topk(int B, int T, const float* v, const float* feat_lens,
                                   const float* fa_boundary, int* pred, int* k_out, int* err,
                                   void* stream) {
  if (B < 0 || T < 0) { mlvae_set_error("mlvae_boundary_topk: B, T must be >= 0"); return 1; }
  if (B == 0 || T == 0) return 0;
  if (!v || !feat_lens || !fa_boundary || !pred || !k_out || !err) {
    mlvae_set_error("mlvae_boundary_topk: null pointer");
    return 1;
  }
  if (T > TOPK_MAX_T) {
    mlvae_set_error("mlvae_boundary_topk: T = %d frames, the row is ranked in LDS: at most %d", T, TOPK_MAX_T);
    return 1;
  }
  if (!zero_async(pred, (size_t)B * T * sizeof(int), stream, "mlvae_boundary_topk") ||
      !zero_async(k_out, (size_t)B * sizeof(int), stream, "mlvae_boundary_topk")) return 2;
  boundary_topk_kernel<<<B, ST, (size_t)T * sizeof(unsigned), (hipStream_t)stream>>>(
      T, v, feat_lens, fa_boundary, pred, k_out, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_boundary_score(int B, int T, const int* pred, const float* target,
                                    const float* feat_lens, int* counts, void* stream) {
  if (B < 0 || T < 0) { mlvae_set_error("mlvae_boundary_score: B, T must be >= 0"); return 1; }
  if (B == 0 || T == 0) return 0;
  if (!pred || !target || !feat_lens || !counts) {
    mlvae_set_error("mlvae_boundary_score: null pointer");
    return 1;
  }
  if (!zero_async(counts, (size_t)B * 3 * sizeof(int), stream, "mlvae_boundary_score")) return 2;
  boundary_score_kernel<<<B, ST, 0, (hipStream_t)stream>>>(T, pred, target, feat_lens, counts);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
