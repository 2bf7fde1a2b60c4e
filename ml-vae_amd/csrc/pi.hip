// MD-VAE pi path (ref:src/models/MD_VAE/model.py:119-150) on gfx950.
//
//   pi_sample_kernel   Categorical(logits = pi_logits) over the two classes of each frame: one
//                      draw per frame in train (label 1 with probability softmax(l)[1]), the
//                      argmax in eval, written as the one-hot row [1 - label, label] that weights
//                      the H-VAE.
//   pi_nll_kernel      pi_nll_loss = -log_prob(decoded frame labels) and its gradient.  The labels
//                      are the Viterbi decode's int32 flvl_out (csrc/decode.hip), read where the
//                      decode left them: no host lists, no pad_sequence.
// All three entries are elementwise passes over [n, 2] logits (8 B read + 8 B / 4 B written per
// frame): launch-bound at the recipe's n = B T = 4000.
//
// MD_VAE_sfl, the score-function estimator (ref:src/models/MD_VAE_sfl/model.py:139-187):
//   pi_sample_k_kernel K draws per frame, draw k of frame i on the uniform of index k n + i.
//   sfl_fwd_kernel     per frame the K rewards (row means of the detached recon / KL losses and
//                      the pi NLL), rif, the negative entropy and the baseline's squared error.
//                      16 lanes share a frame: they stride its [F] and [Z] rows together and
//                      reduce by xor shuffles in a fixed order (no atomics: a rerun is bit-equal).
//   sfl_bwd_kernel     the gradients to the logits and the baseline, one thread per frame.
#include <float.h>

#include "common.h"

namespace {

// U(0,1) draw of local element i: injected (u[i]), or the 24-bit Philox(seed) draw of stream
// element k (k = offset + i without an utterance map; md.hip's draw)
__device__ __forceinline__ float draw(const float* u, unsigned long long seed, unsigned long long k,
                                      size_t i) {
  if (u) return u[i];
  unsigned w[4];
  philox4(seed, k >> 2, w);
  return (w[k & 3] >> 8) * (1.f / 16777216.f);
}

__global__ __launch_bounds__(256) void pi_sample_kernel(size_t n, const float2* __restrict__ logits,
                                                        const float* __restrict__ u,
                                                        unsigned long long seed, unsigned long long off,
                                                        int train, float2* __restrict__ sampled_pi) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float2 l = logits[i];
    int label;
    if (train) {
      // p0 = softmax(l)[0]; saturates to exactly 0 (l1 - l0 large: expf = inf) or 1 (expf = 0),
      // and every draw is in [0, 1): u >= 0 always, u >= 1 never
      const float p0 = 1.f / (1.f + expf(l.y - l.x));
      label = draw(u, seed, off + i, i) >= p0 ? 1 : 0;
    } else {
      label = l.y > l.x ? 1 : 0;  // torch.argmax: the first maximum on a tie
    }
    sampled_pi[i] = make_float2((float)(1 - label), (float)label);
  }
}

template <bool BWD>
__global__ __launch_bounds__(256) void pi_nll_kernel(size_t n, const float2* __restrict__ logits,
                                                     const int* __restrict__ labels,
                                                     float* __restrict__ nll,
                                                     const float* __restrict__ dnll,
                                                     float2* __restrict__ dlogits, int* err) {
  int bad = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float2 l = logits[i];
    int k = labels[i];
    if (k < -1 || k > 1) { bad = MLVAE_ERR_PI_LABEL; k = 0; }  // Categorical.log_prob raises for it
    if (k < 0) k = 0;                          // past T_i: pad_sequence's zero fill
    // e = exp(min - max): the maximum subtracted before the exponential
    const float e = expf(-fabsf(l.y - l.x));
    if (!BWD) {
      const float m = fmaxf(l.x, l.y);
      nll[i] = (m + log1pf(e)) - (k ? l.y : l.x);
    } else {
      const float pmax = 1.f / (1.f + e), pmin = e / (1.f + e);
      const float p0 = l.x >= l.y ? pmax : pmin, p1 = l.x >= l.y ? pmin : pmax;
      const float g = dnll[i];
      dlogits[i] = make_float2(g * (p0 - (k == 0 ? 1.f : 0.f)), g * (p1 - (k == 1 ? 1.f : 0.f)));
    }
  }
  if (!BWD && bad) atomicOr(err, bad);
}

// MAP: the frames are those of a shard (common.h UttMap, T frames per utterance): draw k of
// frame i is stream element k total_utts T + g T + t, what the single process draws for it.
template <bool MAP>
__global__ __launch_bounds__(256) void pi_sample_k_kernel(size_t n, int K,
                                                          const float2* __restrict__ logits,
                                                          const float* __restrict__ u,
                                                          unsigned long long seed, unsigned long long off,
                                                          UttMap m, unsigned T,
                                                          float2* __restrict__ sampled_pi) {
  const unsigned long long dstride = MAP ? m.total * T : n;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float2 l = logits[i];
    const float p0 = 1.f / (1.f + expf(l.y - l.x));  // as pi_sample_kernel
    const unsigned long long gi = MAP ? frame_global(m, i, T) : i;
    for (int k = 0; k < K; ++k) {
      const size_t j = (size_t)k * n + i;
      const int label = draw(u, seed, off + (unsigned long long)k * dstride + gi, j) >= p0 ? 1 : 0;
      sampled_pi[j] = make_float2((float)(1 - label), (float)label);
    }
  }
}

// log_softmax and softmax of one frame's two logits, the maximum subtracted before the
// exponential.  The log-probabilities are clamped to -FLT_MAX (torch clamps to finfo.min in
// Categorical.entropy), so p log p is 0 x finite = 0 at saturation, never NaN.
struct Pi2 {
  float lp0, lp1, p0, p1;
};
__device__ __forceinline__ Pi2 pi2(float2 l) {
  const float gap = fabsf(l.y - l.x), e = expf(-gap);
  // log p of the larger logit is -log1p(e), of the smaller -gap - log1p(e): max - logsumexp
  // written without the cancellation of (max + log1p(e)) - max
  const float lpmax = -log1pf(e), lpmin = fmaxf(-gap - log1pf(e), -FLT_MAX);
  const float pmax = 1.f / (1.f + e), pmin = e / (1.f + e);
  const bool first = l.x >= l.y;
  Pi2 r;
  r.lp0 = first ? lpmax : lpmin;
  r.lp1 = first ? lpmin : lpmax;
  r.p0 = first ? pmax : pmin;
  r.p1 = first ? pmin : pmax;
  return r;
}

constexpr int SFL_LANES = 16;                // lanes per frame
constexpr int SFL_FRAMES = 256 / SFL_LANES;  // frames per block

// Sum of row[0 .. len) over the frame's 16 lanes: each lane adds its strided elements in
// order, then four xor shuffles inside the 16-lane group.  VEC: len % 4 == 0 and the rows are
// 16-byte aligned, read as float4.
template <bool VEC>
__device__ __forceinline__ float row_sum(const float* __restrict__ row, int len, int lane) {
  float s = 0.f;
  if (VEC) {
    const float4* r4 = (const float4*)row;
    for (int j = lane; j < len / 4; j += SFL_LANES) {
      const float4 v = r4[j];
      s += (v.x + v.y) + (v.z + v.w);
    }
  } else {
    for (int j = lane; j < len; j += SFL_LANES) s += row[j];
  }
  for (int o = SFL_LANES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, SFL_LANES);
  return s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void sfl_fwd_kernel(
    size_t n, int K, int F, int Z, const float2* __restrict__ logits,
    const float2* __restrict__ sampled_pi, const float* __restrict__ recon,
    const float* __restrict__ kld, const float* __restrict__ pi_nll,
    const float* __restrict__ baseline, float w_recon, float w_kld, float w_nll,
    float* __restrict__ reward, float* __restrict__ rif, float* __restrict__ neg_entropy,
    float* __restrict__ baseline_loss) {
  const int lane = threadIdx.x % SFL_LANES;
  const float inv_f = 1.f / (float)F, inv_z = 1.f / (float)Z, inv_k = 1.f / (float)K;
  // a 16-lane group enters and leaves the loop together: the shuffles see all of its lanes
  for (size_t i = (size_t)blockIdx.x * SFL_FRAMES + threadIdx.x / SFL_LANES; i < n;
       i += (size_t)gridDim.x * SFL_FRAMES) {
    const Pi2 q = pi2(logits[i]);
    const float b = baseline[i], wn = w_nll * pi_nll[i];
    float acc_rif = 0.f, acc_bl = 0.f;
    for (int k = 0; k < K; ++k) {
      const size_t j = (size_t)k * n + i;
      const float mr = row_sum<VEC>(recon + j * F, F, lane) * inv_f;
      const float mk = row_sum<VEC>(kld + j * Z, Z, lane) * inv_z;
      const float r = -(w_recon * mr + w_kld * mk + wn);
      const float2 s = sampled_pi[j];
      const float nll = -(s.x * q.lp0 + s.y * q.lp1);
      acc_rif += (r - b) * nll;
      acc_bl += (b - r) * (b - r);
      if (lane == 0) reward[j] = r;
    }
    if (lane == 0) {
      rif[i] = acc_rif * inv_k;
      baseline_loss[i] = acc_bl * inv_k;
      neg_entropy[i] = q.p0 * q.lp0 + q.p1 * q.lp1;
    }
  }
}

__global__ __launch_bounds__(256) void sfl_bwd_kernel(
    size_t n, int K, const float2* __restrict__ logits, const float2* __restrict__ sampled_pi,
    const float* __restrict__ reward, const float* __restrict__ baseline,
    const float* __restrict__ d_rif, const float* __restrict__ d_ent, const float* __restrict__ d_bl,
    float2* __restrict__ dlogits, float* __restrict__ dbaseline) {
  const float inv_k = 1.f / (float)K;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const Pi2 q = pi2(logits[i]);
    const float b = baseline[i];
    float g0 = 0.f, g1 = 0.f, gb = 0.f;
    for (int k = 0; k < K; ++k) {
      const size_t j = (size_t)k * n + i;
      const float2 s = sampled_pi[j];
      const float a = reward[j] - b;
      // d nll_k / d l_c = (s_0 + s_1) p_c - s_c: p - onehot_k for a one-hot draw
      g0 += a * ((s.x + s.y) * q.p0 - s.x);
      g1 += a * ((s.x + s.y) * q.p1 - s.y);
      gb -= a;
    }
    const float gr = d_rif[i] * inv_k, ge = d_ent[i];
    const float t0 = q.p0 * q.lp0, t1 = q.p1 * q.lp1, h = t0 + t1;
    dlogits[i] = make_float2(gr * g0 + ge * (t0 - q.p0 * h), gr * g1 + ge * (t1 - q.p1 * h));
    dbaseline[i] = 2.f * inv_k * d_bl[i] * gb;
  }
}

int grid_n(size_t n) {
  size_t b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

int grid_sfl(size_t n) {
  size_t b = (n + SFL_FRAMES - 1) / SFL_FRAMES;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" int mlvae_pi_sample(size_t n, const float* logits, const float* u, unsigned long long seed,
                               unsigned long long offset, int train, float* sampled_pi, void* stream) {
  if (n == 0) return 0;
  if (!logits || !sampled_pi) { mlvae_set_error("mlvae_pi_sample: null pointer"); return 1; }
  pi_sample_kernel<<<grid_n(n), 256, 0, (hipStream_t)stream>>>(
      n, (const float2*)logits, u, seed, offset, train, (float2*)sampled_pi);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_pi_nll_fwd(size_t n, const float* logits, const int* labels, float* nll, int* err,
                                void* stream) {
  if (n == 0) return 0;
  if (!logits || !labels || !nll || !err) { mlvae_set_error("mlvae_pi_nll_fwd: null pointer"); return 1; }
  pi_nll_kernel<false><<<grid_n(n), 256, 0, (hipStream_t)stream>>>(n, (const float2*)logits, labels, nll,
                                                                 nullptr, nullptr, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_pi_nll_bwd(size_t n, const float* logits, const int* labels, const float* dnll,
                                float* dlogits, void* stream) {
  if (n == 0) return 0;
  if (!logits || !labels || !dnll || !dlogits) { mlvae_set_error("mlvae_pi_nll_bwd: null pointer"); return 1; }
  pi_nll_kernel<true><<<grid_n(n), 256, 0, (hipStream_t)stream>>>(n, (const float2*)logits, labels, nullptr,
                                                                dnll, (float2*)dlogits, nullptr);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_pi_sample_k(size_t n, int K, const float* logits, const float* u,
                                 unsigned long long seed, unsigned long long offset, int train,
                                 float* sampled_pi, void* stream) {
  if (n == 0) return 0;
  if (!logits || !sampled_pi) { mlvae_set_error("mlvae_pi_sample_k: null pointer"); return 1; }
  if (K < 1) { mlvae_set_error("mlvae_pi_sample_k: K must be >= 1"); return 1; }
  if (!train) {
    if (K != 1) { mlvae_set_error("mlvae_pi_sample_k: eval (train == 0) is the argmax: K must be 1"); return 1; }
    return mlvae_pi_sample(n, logits, u, seed, offset, 0, sampled_pi, stream);
  }
  pi_sample_k_kernel<false><<<grid_n(n), 256, 0, (hipStream_t)stream>>>(
      n, K, (const float2*)logits, u, seed, offset, UttMap{}, 1u, (float2*)sampled_pi);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_pi_sample_rows(int B, int T, int K, const float* logits, const float* u,
                                    unsigned long long seed, const long long* map, int train,
                                    float* sampled_pi, void* stream) {
  if (B < 0 || T < 0) { mlvae_set_error("mlvae_pi_sample_rows: B and T must be >= 0"); return 1; }
  const size_t n = (size_t)B * T;
  if (n == 0) return 0;
  if (!logits || !sampled_pi) { mlvae_set_error("mlvae_pi_sample_rows: null pointer"); return 1; }
  if (K < 1) { mlvae_set_error("mlvae_pi_sample_rows: K must be >= 1"); return 1; }
  UttMap m;
  if (!utt_map_load(map, B, &m, "mlvae_pi_sample_rows")) return 1;
  if (!train) {  // the argmax draws nothing: no map to apply
    if (K != 1) { mlvae_set_error("mlvae_pi_sample_rows: eval (train == 0) is the argmax: K must be 1"); return 1; }
    return mlvae_pi_sample(n, logits, u, seed, 0ull, 0, sampled_pi, stream);
  }
  pi_sample_k_kernel<true><<<grid_n(n), 256, 0, (hipStream_t)stream>>>(
      n, K, (const float2*)logits, u, seed, 0ull, m, (unsigned)T, (float2*)sampled_pi);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_sfl_fwd(size_t n, int K, int F, int Z, const float* logits, const float* sampled_pi,
                             const float* recon, const float* kld, const float* pi_nll,
                             const float* baseline, float w_recon, float w_kld, float w_nll,
                             float* reward, float* rif, float* neg_entropy, float* baseline_loss,
                             void* stream) {
  if (n == 0) return 0;
  if (!logits || !sampled_pi || !recon || !kld || !pi_nll || !baseline || !reward || !rif ||
      !neg_entropy || !baseline_loss) {
    mlvae_set_error("mlvae_sfl_fwd: null pointer");
    return 1;
  }
  if (K < 1 || F < 1 || Z < 1) { mlvae_set_error("mlvae_sfl_fwd: K, F and Z must be >= 1"); return 1; }
  const bool vec = F % 4 == 0 && Z % 4 == 0 && ((uintptr_t)recon | (uintptr_t)kld) % 16 == 0;
  auto kern = vec ? sfl_fwd_kernel<true> : sfl_fwd_kernel<false>;
  kern<<<grid_sfl(n), 256, 0, (hipStream_t)stream>>>(
      n, K, F, Z, (const float2*)logits, (const float2*)sampled_pi, recon, kld, pi_nll, baseline,
      w_recon, w_kld, w_nll, reward, rif, neg_entropy, baseline_loss);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_sfl_bwd(size_t n, int K, const float* logits, const float* sampled_pi,
                             const float* reward, const float* baseline, const float* d_rif,
                             const float* d_ent, const float* d_bl, float* dlogits, float* dbaseline,
                             void* stream) {
  if (n == 0) return 0;
  if (!logits || !sampled_pi || !reward || !baseline || !d_rif || !d_ent || !d_bl || !dlogits ||
      !dbaseline) {
    mlvae_set_error("mlvae_sfl_bwd: null pointer");
    return 1;
  }
  if (K < 1) { mlvae_set_error("mlvae_sfl_bwd: K must be >= 1"); return 1; }
  sfl_bwd_kernel<<<grid_n(n), 256, 0, (hipStream_t)stream>>>(
      n, K, (const float2*)logits, (const float2*)sampled_pi, reward, baseline, d_rif, d_ent, d_bl,
      (float2*)dlogits, dbaseline);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
