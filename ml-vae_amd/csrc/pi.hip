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
#include "common.h"

namespace {

// U(0,1) draw of frame i: injected, or Philox(seed, offset + i), 24 bits (md.hip's draw)
__device__ __forceinline__ float draw(const float* u, unsigned long long seed, unsigned long long off,
                                      size_t i) {
  if (u) return u[i];
  const unsigned long long k = off + i;
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
      label = draw(u, seed, off, i) >= p0 ? 1 : 0;
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
    if (k < -1 || k > 1) { bad = 32; k = 0; }  // Categorical.log_prob raises for it
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

int grid_n(size_t n) {
  size_t b = (n + 255) / 256;
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
