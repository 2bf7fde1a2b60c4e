// The sequence lattice of the HMM_DNN_ALI aligner (ref:src/models/HMM_DNN_ALI/model.py:47-91, the
// recurrences SpeechBrain's HMMAligner and ctc_loss run) on gfx950: forward-backward and Viterbi
// over a per-utterance left-to-right state chain, the centred log-softmax in front of it and the
// frame-accuracy counts behind it.
//
// Chain.  Phoneme p expands into spp states with emission classes p spp + j; utterance b has
// U_b = spp L_b states.  HMM topology: nodes = states, a path starts in node 0, stays or moves to
// the next node, and ends in node U_b - 1.  CTC topology: blank, s_0, blank, s_1, .., blank
// (2 U_b + 1 nodes); stay, next, and a skip over a blank between two different classes; a path
// starts in node 0 or 1 and ends in one of the last two.  Every transition weighs 0, a path scores
// the sum of its emissions pout[b, t, class(node_t)].
//
// Form ("The sequence lattice").  At the recipe's sizes (B = 8, T of a few
// hundred, up to a few hundred nodes) the recursion is a serial chain of T_b steps and latency
// bound, so one WAVE runs one (utterance, direction): lane l keeps nodes [l NPL, (l + 1) NPL) in
// registers, the neighbour term comes over a lane shift (no LDS, no workgroup barrier per frame),
// and the gathered emissions -- which do not depend on alpha -- are loaded AL_PF frames ahead.
// The beta chain is the alpha chain of the reversed lattice (nodes and frames both reversed; the
// skip rule is symmetric), so both directions are one code path and run concurrently as two
// workgroups.  Every AL_RN frames the wave subtracts its maximum (kept as a float64 offset for the
// score): alpha and beta stay near 0 where fp32 is dense.  A per-frame offset cancels in
//     gamma_t(n) = exp(alpha_t(n) + beta_t(n) - e_t(n)) / sum_n' (the same),
// which the second pass evaluates in parallel over (t, c): dpout[b,t,c] = g_b sum_{class(n)=c}
// gamma_t(n), the nodes of a class summed in ascending node order from a class-sorted node list
// -- no floating-point atomics, a rerun is bit-identical.
//
// Viterbi (HMM topology) keeps float64 sums of the fp32 emissions, as decode.hip does; on a tie
// the recursion keeps "stay", so the path is an exact function of the inputs.  One backpointer
// bit per node and frame goes to the workspace; the backtrack walks 64 frames at a time in LDS.
//
// Lengths: T_b = rintf(T lens_b), L_b = rintf(L phn_lens_b), fp32, half to even, clamped; nothing
// at t >= T_b or l >= L_b is read.  Data errors are bits of *err (ops.raise_align_err), the
// utterance then scores 0 with gradient 0 and alignment -1; no pointer is formed from a bad id.
#include <math.h>
#include "common.h"

namespace {

constexpr int AL_MAX_NODES = 1024;  // nodes of one chain: 64 lanes x at most 16 nodes
constexpr int AL_PF = 4;            // frames of gathered emissions in flight
constexpr int AL_RN = 4;            // frames between two renormalisations
constexpr int AL_TOPO_HMM = 0, AL_TOPO_CTC = 1;
constexpr float NINF = -INFINITY;

// One utterance's chain: lengths and the class of a node.
struct Chain {
  int Tb, Lb, U, N, spp, topo, blank, C;
  const long long* ph;  // phns[b, :]
  __device__ __forceinline__ Chain(int b, int T, int C_, int L, const float* lens, const long long* phns,
                                   const float* phn_lens, int spp_, int topo_, int blank_)
      : spp(spp_), topo(topo_), blank(blank_), C(C_), ph(phns + (size_t)b * L) {
    Tb = round_len(lens[b], T);
    Lb = round_len(phn_lens[b], L);
    U = spp * Lb;
    N = topo == AL_TOPO_CTC ? 2 * U + 1 : U;
  }
  // the HMM chain needs a frame per state; the CTC chain is tried and may find no path
  __device__ __forceinline__ bool shape_ok() const {
    return Tb > 0 && (topo == AL_TOPO_CTC || (U > 0 && Tb >= U));
  }
  // class of node n in [0, N): -1 for an id out of range
  __device__ __forceinline__ int cls(int n) const {
    if (topo == AL_TOPO_CTC) {
      if (!(n & 1)) return blank;
      n >>= 1;
    }
    const long long p = ph[n / spp];
    const long long c = p * spp + n % spp;
    return (p < 0 || c >= C) ? -1 : (int)c;
  }
  __device__ __forceinline__ bool is_target(int n) const { return topo == AL_TOPO_HMM || (n & 1); }
};

// The data errors of one chain, decided by a whole wave the same way in every kernel that walks
// it (nodes strided over the lanes): bits of MLVAE_ERR_ALIGN_*.
__device__ __forceinline__ int chain_errors(const Chain& ch, int lane) {
  int bits = 0;
  if (!ch.shape_ok()) return ch.topo == AL_TOPO_HMM ? MLVAE_ERR_ALIGN_SHORT : 0;
  bool bad = false, blk = false;
  for (int n = lane; n < ch.N; n += 64) {
    if (!ch.is_target(n)) continue;
    const int c = ch.cls(n);
    bad |= c < 0;
    blk |= ch.topo == AL_TOPO_CTC && c == ch.blank;
  }
  if (__any(bad)) bits |= MLVAE_ERR_ALIGN_CLASS;
  if (__any(blk)) bits |= MLVAE_ERR_ALIGN_BLANK;
  return bits;
}

// log(exp a + exp b [+ exp c]) on the hardware exp / log: the step is on the serial path; the
// absolute error of a step (~1e-7) is far inside the bounds the scores are held to
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b), lo = fminf(a, b);
  const float r = m + __logf(1.f + __expf(lo - m));
  return m == NINF ? NINF : r;
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  const float r = m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
  return m == NINF ? NINF : r;
}

// ------------------------------------------------------------------ forward / backward chains
// grid (B, ndir), one wave each.  dir 0: alpha over (frame s, node n'); dir 1: the same recursion
// over the reversed lattice, frame T_b - 1 - s and node N - 1 - n', stored at its own (t, n').
// Row layout of alpha / beta: [B, T, 64 NPL] floats, lane-major (every lane stores its NPL values).
template <int NPL>
__global__ __launch_bounds__(64) void lattice_chain_kernel(
    int T, int C, int L, const float* __restrict__ pout, int ld, const float* __restrict__ lens,
    const long long* __restrict__ phns, const float* __restrict__ phn_lens, int spp, int topo, int blank,
    float* __restrict__ alpha, float* __restrict__ beta, float* __restrict__ score,
    int* __restrict__ okflag, int* err) {
  const int b = blockIdx.x, dir = blockIdx.y, lane = threadIdx.x;
  const Chain ch(b, T, C, L, lens, phns, phn_lens, spp, topo, blank);
  const int bits = chain_errors(ch, lane);
  if (bits || !ch.shape_ok()) {
    if (dir == 0 && lane == 0) {
      score[b] = 0.f;
      okflag[b] = 0;
      if (bits) atomicOr(err, bits);
    }
    return;
  }
  const int Tb = ch.Tb, N = ch.N;
  constexpr int NP = 64 * NPL;
  const int nstart = topo == AL_TOPO_CTC ? 2 : 1;  // start nodes 0 (and 1); by symmetry the end nodes of dir 1

  int cl[NPL];
  bool valid[NPL], skip[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int np = lane * NPL + j;
    valid[j] = np < N;
    cl[j] = 0;
    skip[j] = false;
    if (valid[j]) {
      const int n = dir ? N - 1 - np : np;
      cl[j] = ch.cls(n);  // in [0, C): chain_errors found no bad id
      if (topo == AL_TOPO_CTC && (n & 1) && np >= 2) skip[j] = cl[j] != ch.cls(dir ? n + 2 : n - 2);
    }
  }
  const float* rows = pout + (size_t)b * T * ld;
  float* out = (dir ? beta : alpha) + (size_t)b * T * NP + lane * NPL;

  float e[AL_PF][NPL];
  auto gather = [&](float (&dst)[NPL], int s) {
    const float* row = rows + (size_t)(dir ? Tb - 1 - s : s) * ld;
#pragma unroll
    for (int j = 0; j < NPL; ++j) dst[j] = valid[j] ? row[cl[j]] : NINF;
  };
#pragma unroll
  for (int k = 0; k < AL_PF; ++k)
    if (k < Tb) gather(e[k], k);

  float a[NPL];
  double off = 0.0;  // the renormalisations taken out so far (wave-uniform)
  for (int s0 = 0; s0 < Tb; s0 += AL_PF) {
#pragma unroll
    for (int k = 0; k < AL_PF; ++k) {
      const int s = s0 + k;
      if (s >= Tb) break;  // wave-uniform
      float cur[NPL];
#pragma unroll
      for (int j = 0; j < NPL; ++j) cur[j] = e[k][j];
      if (s + AL_PF < Tb) gather(e[k], s + AL_PF);
      if (s == 0) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) a[j] = (valid[j] && lane * NPL + j < nstart) ? cur[j] : NINF;
      } else {
        // the two nodes below this lane's run
        float p1 = __shfl_up(a[NPL - 1], 1, 64);
        float p2 = NPL >= 2 ? __shfl_up(a[NPL >= 2 ? NPL - 2 : 0], 1, 64) : __shfl_up(a[0], 2, 64);
        if (lane == 0) p1 = p2 = NINF;
        if (NPL == 1 && lane == 1) p2 = NINF;
#pragma unroll
        for (int j = NPL - 1; j >= 0; --j) {
          // descending j: a[j - 1] and a[j - 2] still hold the previous frame.  The node two
          // below j == 1 is the lane below's last (p1), below j == 0 its last but one (p2)
          const float one = j >= 1 ? a[j >= 1 ? j - 1 : 0] : p1;
          const float two = j >= 2 ? a[j >= 2 ? j - 2 : 0] : (j == 1 ? p1 : p2);
          const float r = skip[j] ? lse3(a[j], one, two) : lse2(a[j], one);
          a[j] = valid[j] ? cur[j] + r : NINF;
        }
      }
      if ((s % AL_RN) == AL_RN - 1) {
        float m = NINF;
#pragma unroll
        for (int j = 0; j < NPL; ++j) m = fmaxf(m, a[j]);
        m = wave_max(m);
        if (m > NINF) {
#pragma unroll
          for (int j = 0; j < NPL; ++j) a[j] -= m;  // -inf stays
          off += (double)m;
        }
      }
      float* row = out + (size_t)(dir ? Tb - 1 - s : s) * NP;
      if constexpr (NPL % 4 == 0) {
#pragma unroll
        for (int j = 0; j < NPL; j += 4)
          *reinterpret_cast<f32x4*>(row + j) = f32x4{a[j], a[j + 1], a[j + 2], a[j + 3]};
      } else {
#pragma unroll
        for (int j = 0; j < NPL; ++j) row[j] = a[j];
      }
    }
  }
  if (dir == 0) {
    // score = off + log sum over the end nodes (the last one; CTC: the last two)
    const int nend = topo == AL_TOPO_CTC ? 2 : 1;
    float m = NINF;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const int np = lane * NPL + j;
      if (!(valid[j] && np >= N - nend)) a[j] = NINF;
      m = fmaxf(m, a[j]);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) sum += a[j] > NINF ? expf(a[j] - m) : 0.f;
    sum = wave_sum(sum);
    if (lane == 0) {
      const bool found = m > NINF;  // CTC: no path is torch's zero_infinity, not an error
      score[b] = found ? (float)(off + (double)m + (double)logf(sum)) : 0.f;
      okflag[b] = found ? 1 : 0;
    }
  }
}

// ------------------------------------------------------------------ occupancies -> dpout
// grid (ceil(T / GM_FRAMES), B), 256 threads: the class-sorted node list once per workgroup, then
// one wave per frame.  Dynamic LDS: cls[NP] | list[NP] | start[C + 1] | gam[4][NP].
constexpr int GM_T = 256, GM_W = GM_T / 64, GM_FRAMES = 16;

__global__ __launch_bounds__(GM_T) void lattice_grad_kernel(
    int T, int C, int L, const float* __restrict__ pout, int ld, const float* __restrict__ lens,
    const long long* __restrict__ phns, const float* __restrict__ phn_lens, int spp, int topo, int blank,
    const float* __restrict__ g, const float* __restrict__ alpha, const float* __restrict__ beta,
    const int* __restrict__ okflag, int NP, float* __restrict__ dpout, int ldd) {
  extern __shared__ int lds[];
  int* cls = lds;
  int* list = cls + NP;
  int* start = list + NP;
  float* gam = reinterpret_cast<float*>(start + C + 1);
  const int b = blockIdx.y, t0 = blockIdx.x * GM_FRAMES, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t1 = min(t0 + GM_FRAMES, T);
  const Chain ch(b, T, C, L, lens, phns, phn_lens, spp, topo, blank);
  float* drow = dpout + (size_t)b * T * ldd;
  const bool ok = okflag[b] != 0;
  const int Tb = ok ? ch.Tb : 0, N = ch.N;
  // frames past the utterance, or all of an utterance without a path: exact zeros
  for (int t = max(t0, Tb) + wave; t < t1; t += GM_W)
    for (int c = lane; c < C; c += 64) drow[(size_t)t * ldd + c] = 0.f;
  if (t0 >= Tb) return;  // workgroup-uniform

  for (int n = tid; n < N; n += GM_T) cls[n] = ch.cls(n);  // valid ids: okflag says so
  __syncthreads();
  for (int c = tid; c < C; c += GM_T) {
    int cnt = 0;
    for (int n = 0; n < N; ++n) cnt += cls[n] == c;
    start[c + 1] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    start[0] = 0;
    for (int c = 0; c < C; ++c) start[c + 1] += start[c];
  }
  __syncthreads();
  for (int c = tid; c < C; c += GM_T) {
    int at = start[c];
    for (int n = 0; n < N; ++n)
      if (cls[n] == c) list[at++] = n;  // ascending node order inside a class
  }
  __syncthreads();

  const float gb = g[b];
  const float* rows = pout + (size_t)b * T * ld;
  float* gw = gam + (size_t)wave * NP;
  for (int it = 0; it < GM_FRAMES / GM_W; ++it) {  // uniform trip count: the barriers below
    const int t = t0 + it * GM_W + wave;
    const bool act = t < Tb;
    float m = NINF;
    if (act) {
      const float* ar = alpha + ((size_t)b * T + t) * NP;
      const float* br = beta + ((size_t)b * T + t) * NP;
      const float* er = rows + (size_t)t * ld;
      for (int n = lane; n < N; n += 64) {
        const float av = ar[n], bv = br[N - 1 - n];
        const float v = (av == NINF || bv == NINF) ? NINF : av + bv - er[cls[n]];
        gw[n] = v;
        m = fmaxf(m, v);
      }
    }
    m = wave_max(m);
    float sum = 0.f;
    if (act && m > NINF) {
      for (int n = lane; n < N; n += 64) {  // each lane rereads what it wrote
        const float w = expf(gw[n] - m);
        gw[n] = w;
        sum += w;
      }
    }
    sum = wave_sum(sum);
    __syncthreads();
    if (act) {
      const float scale = (m > NINF && sum > 0.f) ? gb / sum : 0.f;
      for (int c = lane; c < C; c += 64) {
        float s = 0.f;
        for (int i = start[c]; i < start[c + 1]; ++i) s += gw[list[i]];
        drow[(size_t)t * ldd + c] = start[c + 1] > start[c] ? s * scale : 0.f;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ Viterbi (HMM topology)
// One wave per utterance.  delta in float64 (exact sums of the fp32 emissions in frame order);
// bp[b, t, lane] bit j = node lane NPL + j at frame t came from the node below ("next"), 0 = "stay",
// kept on a tie.
template <int NPL>
__global__ __launch_bounds__(64) void hmm_viterbi_kernel(
    int T, int C, int L, const float* __restrict__ pout, int ld, const float* __restrict__ lens,
    const long long* __restrict__ phns, const float* __restrict__ phn_lens, int spp,
    float* __restrict__ vscore, int* __restrict__ align, unsigned* __restrict__ bp, int* err) {
  __shared__ unsigned sh[64][65];
  __shared__ int al[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const Chain ch(b, T, C, L, lens, phns, phn_lens, spp, AL_TOPO_HMM, 0);
  int* arow = align + (size_t)b * T;
  const int bits = chain_errors(ch, lane);
  if (bits) {
    for (int t = lane; t < T; t += 64) arow[t] = -1;
    if (lane == 0) {
      vscore[b] = 0.f;
      atomicOr(err, bits);
    }
    return;
  }
  const int Tb = ch.Tb, N = ch.N;
  int cl[NPL];
  bool valid[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int n = lane * NPL + j;
    valid[j] = n < N;
    cl[j] = valid[j] ? ch.cls(n) : 0;
  }
  const float* rows = pout + (size_t)b * T * ld;
  unsigned* bprow = bp + (size_t)b * T * 64;

  float e[AL_PF][NPL];
  auto gather = [&](float (&dst)[NPL], int t) {
    const float* row = rows + (size_t)t * ld;
#pragma unroll
    for (int j = 0; j < NPL; ++j) dst[j] = valid[j] ? row[cl[j]] : NINF;
  };
#pragma unroll
  for (int k = 0; k < AL_PF; ++k)
    if (k < Tb) gather(e[k], k);

  double d[NPL];
  const double DNINF = -INFINITY;
  for (int s0 = 0; s0 < Tb; s0 += AL_PF) {
#pragma unroll
    for (int k = 0; k < AL_PF; ++k) {
      const int t = s0 + k;
      if (t >= Tb) break;
      float cur[NPL];
#pragma unroll
      for (int j = 0; j < NPL; ++j) cur[j] = e[k][j];
      if (t + AL_PF < Tb) gather(e[k], t + AL_PF);
      unsigned word = 0;
      if (t == 0) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) d[j] = (lane == 0 && j == 0) ? (double)cur[j] : DNINF;
      } else {
        double p1 = __shfl_up(d[NPL - 1], 1, 64);
        if (lane == 0) p1 = DNINF;
#pragma unroll
        for (int j = NPL - 1; j >= 0; --j) {
          const double below = j >= 1 ? d[j >= 1 ? j - 1 : 0] : p1;
          const bool take = below > d[j];  // a tie keeps "stay"
          const double best = take ? below : d[j];
          word |= (take && valid[j]) ? (1u << j) : 0u;
          d[j] = valid[j] ? best + (double)cur[j] : DNINF;
        }
      }
      bprow[(size_t)t * 64 + lane] = word;
    }
  }
  // the end node's score
  {
    const int owner = (N - 1) / NPL, slot = (N - 1) % NPL;
    double v = DNINF;
#pragma unroll
    for (int j = 0; j < NPL; ++j) v = (j == slot) ? d[j] : v;
    v = __shfl(v, owner, 64);
    if (lane == 0) vscore[b] = (float)v;
  }
  __syncthreads();  // the backpointers of every lane are visible to the wave
  // backtrack from (T_b - 1, N - 1), 64 frames at a time
  int u = N - 1;  // lane 0's
  for (int tc = ((Tb - 1) / 64) * 64; tc >= 0; tc -= 64) {
    for (int r = 0; r < 64; ++r)
      if (tc + r < Tb) sh[r][lane] = bprow[(size_t)(tc + r) * 64 + lane];
    __syncthreads();
    if (lane == 0) {
      for (int r = 63; r >= 0; --r) {
        const int t = tc + r;
        if (t >= Tb) continue;
        al[r] = u;
        if (t > 0) u -= (int)((sh[r][u / NPL] >> (u % NPL)) & 1u);
      }
    }
    __syncthreads();
    if (tc + lane < Tb) arow[tc + lane] = al[lane];
    __syncthreads();
  }
  for (int t = Tb + lane; t < T; t += 64) arow[t] = -1;
}

// ------------------------------------------------------------------ alignment accuracy counts
__global__ __launch_bounds__(256) void align_counts_kernel(
    int T, int L, const int* __restrict__ align, const float* __restrict__ lens,
    const long long* __restrict__ phns, const float* __restrict__ phn_lens, int spp,
    const long long* __restrict__ ends, long long spf, int* __restrict__ counts) {
  __shared__ int sh[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = round_len(lens[b], T), Lb = round_len(phn_lens[b], L);
  const long long* ph = phns + (size_t)b * L;
  const long long* en = ends + (size_t)b * L;
  const int* ar = align + (size_t)b * T;
  int ok = 0;
  if (Lb > 0) {
    for (int t = tid; t < Tb; t += 256) {
      const int u = ar[t];
      if (u < 0 || u / spp >= Lb) continue;  // no alignment: the frame is wrong
      int k = 0;
      const long long at = (long long)t * spf;
      while (k < Lb - 1 && !(at < en[k])) ++k;  // the first segment that ends after the frame, else the last
      ok += ph[u / spp] == ph[k];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ok += __shfl_xor(ok, o, 64);
  if ((tid & 63) == 0) sh[tid >> 6] = ok;
  __syncthreads();
  if (tid == 0) {
    counts[2 * (size_t)b] = sh[0] + sh[1] + sh[2] + sh[3];
    counts[2 * (size_t)b + 1] = Tb;
  }
}

// ------------------------------------------------------------------ centre + log-softmax
// mean[b, c] = sum_t src[b, t, c] / T over all T rows of the padded batch (fp32, increasing t in
// four interleaved slices combined in a fixed order).  grid (ceil(C / 64), B), 256 threads.
__global__ __launch_bounds__(256) void colmean_kernel(int T, int C, const float* __restrict__ src,
                                                      float* __restrict__ mean) {
  __shared__ float part[4][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (c < C)
    for (int t = wave; t < T; t += 4) s += src[((size_t)b * T + t) * C + c];
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < C)
    mean[(size_t)b * C + c] = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / (float)T;
}

// y[r, :] = log_softmax(x[r, :] - mean[b, :]); one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void center_lsm_fwd_kernel(int rows, int T, int C,
                                                             const float* __restrict__ x,
                                                             const float* __restrict__ mean,
                                                             float* __restrict__ y) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* xr = x + (size_t)r * C;
  const float* mr = mean + (size_t)(r / T) * C;
  float* yr = y + (size_t)r * C;
  float m = NINF;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c] - mr[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(xr[c] - mr[c] - m);
  s = wave_sum(s);
  const float lz = m + logf(s);
  for (int c = lane; c < C; c += 64) yr[c] = xr[c] - mr[c] - lz;
}

// dz[r, :] = dy[r, :] - exp(y[r, :]) sum_c dy[r, c]
__global__ __launch_bounds__(256) void center_lsm_bwd_kernel(int rows, int C, const float* __restrict__ dy,
                                                             const float* __restrict__ y,
                                                             float* __restrict__ dz) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* gr = dy + (size_t)r * C;
  const float* yr = y + (size_t)r * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += gr[c];
  s = wave_sum(s);
  for (int c = lane; c < C; c += 64) dz[(size_t)r * C + c] = gr[c] - expf(yr[c]) * s;
}

// v[b, t, c] -= mean[b, c]
__global__ __launch_bounds__(256) void sub_colmean_kernel(size_t n, int T, int C, float* __restrict__ v,
                                                          const float* __restrict__ mean) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t r = i / C;
  v[i] -= mean[(r / T) * C + (i - r * C)];
}

// ------------------------------------------------------------------ host side
int nodes_bound(int L, int spp, int topo) {  // -1: over the limit
  const long long u = (long long)L * spp;
  const long long n = topo == AL_TOPO_CTC ? 2 * u + 1 : u;
  return n > AL_MAX_NODES ? -1 : (int)n;
}
int pick_npl(int n) {
  int npl = 1;
  while (64 * npl < n) npl *= 2;
  return npl;  // 1, 2, 4, 8 or 16 for n <= AL_MAX_NODES
}
struct LatticeWs {
  float *alpha, *beta;
  int* ok;
  size_t bytes;
};
LatticeWs lattice_ws(void* ws, int B, int T, int np) {
  const size_t plane = (size_t)B * T * np * sizeof(float);
  LatticeWs w;
  w.alpha = (float*)ws;
  w.beta = (float*)((char*)ws + plane);
  w.ok = (int*)((char*)ws + 2 * plane);
  w.bytes = 2 * plane + (size_t)B * sizeof(int);
  return w;
}
bool lattice_args(const char* who, int B, int T, int C, int L, int ld, int spp, int topo, int blank) {
  if (B < 0 || T < 0 || L < 0 || C < 1 || ld < C || spp < 1) {
    mlvae_set_error("%s: B, T, L must be >= 0, C >= 1, ld >= C and spp >= 1", who);
    return false;
  }
  if (topo != AL_TOPO_HMM && topo != AL_TOPO_CTC) {
    mlvae_set_error("%s: topology %d (0 HMM, 1 CTC)", who, topo);
    return false;
  }
  if (topo == AL_TOPO_CTC && (blank < 0 || blank >= C)) {
    mlvae_set_error("%s: blank %d outside [0, %d)", who, blank, C);
    return false;
  }
  if (nodes_bound(L, spp, topo) < 0) {
    mlvae_set_error("%s: L = %d phonemes of %d states give a chain of more than %d nodes (one wave "
                    "holds the chain in registers)", who, L, spp, AL_MAX_NODES);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int mlvae_lattice_max_nodes(void) { return AL_MAX_NODES; }

extern "C" size_t mlvae_lattice_workspace_size(int B, int T, int L, int spp, int topology) {
  const int n = nodes_bound(L < 0 ? 0 : L, spp < 1 ? 1 : spp, topology);
  if (n < 0 || B < 0 || T < 0) return 0;
  return lattice_ws(nullptr, B, T, 64 * pick_npl(n)).bytes;
}

extern "C" int mlvae_lattice_fb(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                                const long long* phns, const float* phn_lens, int spp, int topology,
                                int blank, int need_beta, float* score, void* ws, size_t ws_bytes,
                                int* err, void* stream) {
  if (!lattice_args("mlvae_lattice_fb", B, T, C, L, ld, spp, topology, blank)) return 1;
  if (B == 0) return 0;
  if (!pout || !lens || !phn_lens || !score || !ws || !err || (L > 0 && !phns)) {
    mlvae_set_error("mlvae_lattice_fb: null pointer");
    return 1;
  }
  const int npl = pick_npl(nodes_bound(L, spp, topology));
  const LatticeWs w = lattice_ws(ws, B, T, 64 * npl);
  if (ws_bytes < w.bytes) {
    mlvae_set_error("mlvae_lattice_fb: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return 1;
  }
  const dim3 grid(B, need_beta ? 2 : 1);
#define AL_CHAIN(N_)                                                                              \
  lattice_chain_kernel<N_><<<grid, 64, 0, (hipStream_t)stream>>>(T, C, L, pout, ld, lens, phns,  \
                                                                   phn_lens, spp, topology, blank, \
                                                                   w.alpha, w.beta, score, w.ok, err)
  switch (npl) {
    case 1: AL_CHAIN(1); break;
    case 2: AL_CHAIN(2); break;
    case 4: AL_CHAIN(4); break;
    case 8: AL_CHAIN(8); break;
    default: AL_CHAIN(16); break;
  }
#undef AL_CHAIN
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_lattice_grad(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                                  const long long* phns, const float* phn_lens, int spp, int topology,
                                  int blank, const float* g, const void* ws, size_t ws_bytes,
                                  float* dpout, int ldd, void* stream) {
  if (!lattice_args("mlvae_lattice_grad", B, T, C, L, ld, spp, topology, blank)) return 1;
  if (ldd < C) {
    mlvae_set_error("mlvae_lattice_grad: ldd %d < C %d", ldd, C);
    return 1;
  }
  if (B == 0 || T == 0) return 0;
  if (!pout || !lens || !phn_lens || !g || !ws || !dpout || (L > 0 && !phns)) {
    mlvae_set_error("mlvae_lattice_grad: null pointer");
    return 1;
  }
  const int np = 64 * pick_npl(nodes_bound(L, spp, topology));
  const LatticeWs w = lattice_ws(const_cast<void*>(ws), B, T, np);
  if (ws_bytes < w.bytes) {
    mlvae_set_error("mlvae_lattice_grad: workspace of %zu bytes, %zu needed", ws_bytes, w.bytes);
    return 1;
  }
  const size_t lds = ((size_t)2 * np + (size_t)C + 1 + (size_t)GM_W * np) * 4;
  if (lds > 64 * 1024) {
    mlvae_set_error("mlvae_lattice_grad: C = %d classes with %d nodes need %zu bytes of LDS (64 KB)", C, np, lds);
    return 1;
  }
  lattice_grad_kernel<<<dim3((T + GM_FRAMES - 1) / GM_FRAMES, B), GM_T, lds, (hipStream_t)stream>>>(
      T, C, L, pout, ld, lens, phns, phn_lens, spp, topology, blank, g, w.alpha, w.beta, w.ok, np, dpout, ldd);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_hmm_viterbi_workspace_size(int B, int T) {
  if (B < 0 || T < 0) return 0;
  return (size_t)B * T * 64 * sizeof(unsigned);
}

extern "C" int mlvae_hmm_viterbi(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                                 const long long* phns, const float* phn_lens, int spp, float* vscore,
                                 int* align, void* ws, size_t ws_bytes, int* err, void* stream) {
  if (!lattice_args("mlvae_hmm_viterbi", B, T, C, L, ld, spp, AL_TOPO_HMM, 0)) return 1;
  if (B == 0) return 0;
  if (!pout || !lens || !phn_lens || !vscore || !align || !ws || !err || (L > 0 && !phns)) {
    mlvae_set_error("mlvae_hmm_viterbi: null pointer");
    return 1;
  }
  const size_t need = mlvae_hmm_viterbi_workspace_size(B, T);
  if (ws_bytes < need) {
    mlvae_set_error("mlvae_hmm_viterbi: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return 1;
  }
#define AL_VIT(N_)                                                                            \
  hmm_viterbi_kernel<N_><<<B, 64, 0, (hipStream_t)stream>>>(T, C, L, pout, ld, lens, phns,   \
                                                             phn_lens, spp, vscore, align,    \
                                                             (unsigned*)ws, err)
  switch (pick_npl(nodes_bound(L, spp, AL_TOPO_HMM))) {
    case 1: AL_VIT(1); break;
    case 2: AL_VIT(2); break;
    case 4: AL_VIT(4); break;
    case 8: AL_VIT(8); break;
    default: AL_VIT(16); break;
  }
#undef AL_VIT
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_align_counts(int B, int T, int L, const int* align, const float* lens,
                                  const long long* phns, const float* phn_lens, int spp,
                                  const long long* phn_ends, long long samples_per_frame, int* counts,
                                  void* stream) {
  if (B < 0 || T < 0 || L < 0 || spp < 1 || samples_per_frame < 1) {
    mlvae_set_error("mlvae_align_counts: B, T, L must be >= 0, spp >= 1 and samples_per_frame >= 1");
    return 1;
  }
  if (B == 0) return 0;
  if (!lens || !phn_lens || !counts || (T > 0 && !align) || (L > 0 && (!phns || !phn_ends))) {
    mlvae_set_error("mlvae_align_counts: null pointer");
    return 1;
  }
  align_counts_kernel<<<B, 256, 0, (hipStream_t)stream>>>(T, L, align, lens, phns, phn_lens, spp, phn_ends,
                                                          samples_per_frame, counts);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_center_lsm_workspace_size(int B, int C) {
  return (B < 0 || C < 0) ? 0 : (size_t)B * C * sizeof(float);
}

extern "C" int mlvae_center_lsm_fwd(int B, int T, int C, const float* x, float* y, void* ws,
                                    size_t ws_bytes, void* stream) {
  if (B < 0 || T < 0 || C < 1) {
    mlvae_set_error("mlvae_center_lsm_fwd: B, T must be >= 0 and C >= 1");
    return 1;
  }
  if (B == 0 || T == 0) return 0;
  if (!x || !y || !ws || ws_bytes < mlvae_center_lsm_workspace_size(B, C)) {
    mlvae_set_error("mlvae_center_lsm_fwd: null pointer or a workspace under B C floats");
    return 1;
  }
  const int rows = B * T;
  colmean_kernel<<<dim3((C + 63) / 64, B), 256, 0, (hipStream_t)stream>>>(T, C, x, (float*)ws);
  center_lsm_fwd_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(rows, T, C, x, (const float*)ws, y);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_center_lsm_bwd(int B, int T, int C, const float* dy, const float* y, float* dx,
                                    void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || T < 0 || C < 1) {
    mlvae_set_error("mlvae_center_lsm_bwd: B, T must be >= 0 and C >= 1");
    return 1;
  }
  if (B == 0 || T == 0) return 0;
  if (!dy || !y || !dx || !ws || ws_bytes < mlvae_center_lsm_workspace_size(B, C)) {
    mlvae_set_error("mlvae_center_lsm_bwd: null pointer or a workspace under B C floats");
    return 1;
  }
  const int rows = B * T;
  const size_t n = (size_t)rows * C;
  center_lsm_bwd_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(rows, C, dy, y, dx);
  colmean_kernel<<<dim3((C + 63) / 64, B), 256, 0, (hipStream_t)stream>>>(T, C, dx, (float*)ws);
  sub_colmean_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(n, T, C, dx, (const float*)ws);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
