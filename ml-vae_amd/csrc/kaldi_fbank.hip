// Waveform -> Kaldi-compatible log-mel filterbank + deltas + delta-deltas, and per-speaker CMVN, on
// gfx950: what the reference's `kaldi_feat` holds (ref:src/utils/data_io_utils.py:150-206):
//   compute-fbank-feats --window-type=hamming --htk-compat=true --dither=0.0 --energy-floor=1.0
//                       --snip-edges=false | add-deltas | per-speaker compute-cmvn-stats and
//   apply-cmvn --norm-vars=true
// restated from Kaldi's documented behaviour.  No Kaldi binary is among the pinned references, so
// parity with Kaldi is unpinned; the pin is the float64 restatement tests/kaldi_fbank_ref.py.
// Per utterance b with N_b valid samples, shift and L in samples, P the power of two >= L:
//
//   T_b = (N_b + shift/2) / shift frames; frame f covers samples shift f + shift/2 - L/2 + i,
//   i = 0..L-1, an index outside [0, N_b) mirrored at the ends until it is inside (the padding of a
//   padded batch is never read); per frame: subtract the mean, pre-emphasis 0.97, symmetric Hamming
//   window, zero-pad to P; |X_k|^2, k = 0..P/2-1 (no Nyquist bin); triangular filters on the
//   1127 ln(1 + f/700) mel scale from 20 Hz to sample_rate/2; ln(max(energy, FLT_EPSILON));
//   delta_t = sum_{j=-2..2} j x_{clamp(t+j)} / 10; delta-delta = the 9 taps
//   [4 4 1 -4 -10 -4 1 4 4]/100 on the statics at clamped indices.
//   out [B, Tmax, 3 n_mels] = (static | delta | delta-delta), rows t >= T_b exact zeros.
//
//   kaldi_tile_kernel    one workgroup per (utterance, 32-frame tile), as fbank.hip's: a wave stages
//                        a frame (reflection map, mean as a wave reduction, pre-emphasis through lane
//                        shuffles, all fp32) to LDS; X = frames . table (the windowed twiddles, fp32
//                        from a float64 host fill) on the exact-f32 MFMA, the chain folded every
//                        KBLK samples, re and im of a bin in the same lane; |X|^2 to LDS, the mel
//                        projection and the log from there.  Only the log-mel tile leaves.
//   kaldi_finish_kernel  both delta orders with the edges at the utterance's own frames, the output
//                        rows and the zero rows.
//   cmvn_accumulate      one workgroup per speaker walks the batch's utterances in row order and
//                        their frames in time order, float64 running sums per column, then adds them
//                        to the caller's [S, 2 D + 1] buffer: a fixed order, no atomics on floats.
//   cmvn_apply           y = (x - mean) / sqrt(var) in place on the valid rows.
#include <float.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int FT = 32;        // frames per tile (one 32-row MFMA tile)
constexpr int NT = 256;       // threads
constexpr int NW = NT / 64;   // waves
constexpr int KBLK = 128;     // samples per MFMA chain before the fold
constexpr int GK = 16;        // samples per operand group of the DFT loop (double-buffered registers)
constexpr int MAX_P = 512;
constexpr int MAX_MELS = 64;
constexpr int MELP = 64;      // mel columns of the filter table (zero past n_mels)
constexpr float PREEMPH = 0.97f;
constexpr double LOW_HZ = 20.0;
constexpr double VAR_FLOOR = 1e-20;

struct Geo {
  int shift, L, P, n_mels;
  int wr;    // window rows of the table: L rounded up to even (a zero row)
  int K;     // bins P/2
  int nbt;   // 32-bin tiles
  int ldt;   // table row: nbt x (32 re | 32 im)
  int lda;   // LDS frame row (odd: conflict-free column reads)
  int ldp;   // LDS power row
};

Geo make_geo(int shift, int L, int P, int n_mels) {
  Geo g;
  g.shift = shift; g.L = L; g.P = P; g.n_mels = n_mels;
  g.wr = (L + 1) & ~1;
  g.K = P / 2;
  g.nbt = (g.K + 31) / 32;
  g.ldt = g.nbt * 64;
  g.lda = g.wr + 1;
  g.ldp = g.nbt * 32 + 1;
  return g;
}

bool geo_ok(const char* who, int shift, int L, int P, int n_mels) {
  if (P < 2 || (P & (P - 1)) || P > MAX_P) {
    mlvae_set_error("%s: P = %d must be a power of two in [2, %d]", who, P, MAX_P);
    return false;
  }
  if (L < 2 || L > P) {
    mlvae_set_error("%s: the window (L = %d samples) must be in [2, P = %d]", who, L, P);
    return false;
  }
  if (n_mels < 1 || n_mels > MAX_MELS) {
    mlvae_set_error("%s: n_mels = %d must be in [1, %d]", who, n_mels, MAX_MELS);
    return false;
  }
  if (shift < 1) {
    mlvae_set_error("%s: hop = %d samples must be >= 1", who, shift);
    return false;
  }
  return true;
}

size_t table_floats(const Geo& g) { return (size_t)g.wr * g.ldt + (size_t)g.K * MELP; }
size_t lds_bytes(const Geo& g) { return ((size_t)FT * g.lda + (size_t)FT * g.ldp) * sizeof(float); }
long long frames_of(long long N, int shift) { return (N + shift / 2) / shift; }

__global__ __launch_bounds__(NT) void kaldi_tile_kernel(
    Geo g, int Nmax, int Tmax, const float* __restrict__ wav, int ld, const int* __restrict__ n_samples,
    const float* __restrict__ table, float* __restrict__ ws_log) {
  extern __shared__ float lds[];
  float* As = lds;                // [FT][lda] the preprocessed frames
  float* Ps = lds + FT * g.lda;   // [FT][ldp] |X|^2
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Nb = clampi(n_samples[b], 0, Nmax);
  const int Tb = (int)(((long long)Nb + g.shift / 2) / g.shift);
  const int t0 = tile * FT;
  if (t0 >= Tb) return;  // uniform: the finish kernel reads rows below T_b only

  // the frame tile, a wave per frame, the lanes along the window (up to MAX_P / 64 loads in flight
  // per lane): sample s mirrored into [0, N_b) is r = s mod 2 N_b, or 2 N_b - 1 - r past N_b
  // (N_b >= 1 here: T_b >= 1)
  const float* w = wav + (size_t)b * ld;
  const long long two_n = 2ll * Nb;
  const float inv_L = 1.f / (float)g.L;
  for (int f = wave; f < FT; f += NW) {
    const long long s0 = (long long)(t0 + f) * g.shift + g.shift / 2 - g.L / 2;
    const bool live = t0 + f < Tb;
    float v[MAX_P / 64];
#pragma unroll
    for (int j = 0; j < MAX_P / 64; ++j) {
      const int n = lane + 64 * j;
      float x = 0.f;
      if (live && n < g.L) {
        long long r = s0 + n;
        if (r < 0 || r >= Nb) {  // the utterance's first and last frames only
          r %= two_n;
          if (r < 0) r += two_n;
          if (r >= Nb) r = two_n - 1 - r;
        }
        x = w[r];
      }
      v[j] = x;
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_P / 64; ++j) sum += v[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float mean = sum * inv_L;
#pragma unroll
    for (int j = 0; j < MAX_P / 64; ++j) v[j] = lane + 64 * j < g.L ? v[j] - mean : 0.f;
    // pre-emphasis: sample n - 1 is the lane below, lane 63 of the previous register for lane 0,
    // and sample 0 itself for n = 0
    float carry = __shfl(v[0], 0, 64);
#pragma unroll
    for (int j = 0; j < MAX_P / 64; ++j) {
      const float below = __shfl_up(v[j], 1, 64);
      const float prev = lane == 0 ? carry : below;
      carry = __shfl(v[j], 63, 64);
      const int n = lane + 64 * j;
      if (n < g.wr) As[f * g.lda + n] = n < g.L ? v[j] - PREEMPH * prev : 0.f;
    }
  }
  __syncthreads();

  // X = frames . table: A[i = frame][k = sample] one value per lane (lane l: i = l & 31, k = l >> 5),
  // B[k][j = column] straight from the table (L2-resident, 128-byte row segments per half wave)
  const int l32 = lane & 31, h = lane >> 5;
  for (int bt = wave; bt < g.nbt; bt += NW) {
    const float* tb = table + bt * 64 + l32;
    f32x16 tre, tim, are, aim;
#pragma unroll
    for (int v = 0; v < 16; ++v) { tre[v] = 0.f; tim[v] = 0.f; are[v] = 0.f; aim[v] = 0.f; }
    // groups of GK samples (GK / 2 MFMA steps), the next group's operands loaded (table: L2
    // latency) while the current one multiplies; zeros past the window
    const int ngroups = (g.wr + GK - 1) / GK;
    auto load = [&](int gi, float* a, float* re, float* im) {
#pragma unroll
      for (int j = 0; j < GK / 2; ++j) {
        const int k = gi * GK + 2 * j + h;
        const bool in = k < g.wr;
        const float* row = tb + (size_t)k * g.ldt;
        a[j] = in ? As[l32 * g.lda + k] : 0.f;
        re[j] = in ? row[0] : 0.f;
        im[j] = in ? row[32] : 0.f;
      }
    };
    auto mma = [&](int gi, const float* a, const float* re, const float* im) {
#pragma unroll
      for (int j = 0; j < GK / 2; ++j) {
        are = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], re[j], are, 0, 0, 0);
        aim = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], im[j], aim, 0, 0, 0);
      }
      if ((gi + 1) % (KBLK / GK) == 0) {  // uniform: fold the chain
#pragma unroll
        for (int v = 0; v < 16; ++v) { tre[v] += are[v]; tim[v] += aim[v]; are[v] = 0.f; aim[v] = 0.f; }
      }
    };
    float a0[GK / 2], r0[GK / 2], i0[GK / 2], a1[GK / 2], r1[GK / 2], i1[GK / 2];
    load(0, a0, r0, i0);
    for (int gi = 0; gi < ngroups; gi += 2) {
      load(gi + 1, a1, r1, i1);
      mma(gi, a0, r0, i0);
      load(gi + 2, a0, r0, i0);
      mma(gi + 1, a1, r1, i1);
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) { tre[v] += are[v]; tim[v] += aim[v]; }
    // C layout: col = lane & 31 (bin), row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5) (frame)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int f = (v & 3) + 8 * (v >> 2) + 4 * h;
      Ps[f * g.ldp + bt * 32 + l32] = tre[v] * tre[v] + tim[v] * tim[v];
    }
  }
  __syncthreads();

  // mel projection: lane = mel, each wave FT / NW frames; the power values are LDS broadcasts
  constexpr int FW = FT / NW;
  const float* fb = table + (size_t)g.wr * g.ldt + lane;
  float mel[FW];
#pragma unroll
  for (int i = 0; i < FW; ++i) mel[i] = 0.f;
  const float* pr = Ps + wave * FW * g.ldp;
#pragma unroll 8
  for (int k = 0; k < g.K; ++k) {
    const float wk = fb[(size_t)k * MELP];
#pragma unroll
    for (int i = 0; i < FW; ++i) mel[i] = fmaf(pr[i * g.ldp + k], wk, mel[i]);
  }
#pragma unroll
  for (int i = 0; i < FW; ++i) {
    const int t = t0 + wave * FW + i;
    if (lane < g.n_mels && t < Tb)
      ws_log[((size_t)b * Tmax + t) * g.n_mels + lane] = logf(fmaxf(mel[i], FLT_EPSILON));
  }
}

__global__ __launch_bounds__(NT) void kaldi_finish_kernel(
    Geo g, int Nmax, int Tmax, int deltas, const int* __restrict__ n_samples,
    const float* __restrict__ ws_log, float* __restrict__ out, int ldo, int* __restrict__ frames) {
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int Nb = clampi(n_samples[b], 0, Nmax);
  const int Tb = (int)(((long long)Nb + g.shift / 2) / g.shift);
  if (tile == 0 && tid == 0) frames[b] = Tb;
  const int t0 = tile * FT;
  const int M = g.n_mels;
  const float* lg = ws_log + (size_t)b * Tmax * M;
  auto stat = [&](int u, int m) { return lg[(size_t)clampi(u, 0, Tb - 1) * M + m]; };
  for (int idx = tid; idx < FT * M; idx += NT) {
    const int f = idx / M, m = idx - f * M, t = t0 + f;
    if (t >= Tmax) break;
    float* o = out + ((size_t)b * Tmax + t) * ldo;
    float x = 0.f, d = 0.f, dd = 0.f;
    if (t < Tb) {
      x = stat(t, m);
      if (deltas) {
        float xs[9];
#pragma unroll
        for (int j = -4; j <= 4; ++j) xs[j + 4] = stat(t + j, m);
        float s = 0.f;
#pragma unroll
        for (int j = -2; j <= 2; ++j) s += (float)j * xs[j + 4];
        d = s / 10.f;
        constexpr float c9[9] = {4.f, 4.f, 1.f, -4.f, -10.f, -4.f, 1.f, 4.f, 4.f};
        s = 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) s += c9[j] * xs[j];
        dd = s / 100.f;
      }
    }
    o[m] = x;
    if (deltas) { o[M + m] = d; o[2 * M + m] = dd; }
  }
}

// stats [S, 2 D + 1] float64 = (sum x | sum x^2 | n).  One workgroup per speaker; a thread owns
// columns tid, tid + NT, ... and keeps their running sums in registers over the whole batch.
constexpr int CMVN_COLS = 4;  // columns per thread: D <= CMVN_COLS * NT

__global__ __launch_bounds__(NT) void cmvn_accumulate_kernel(
    int B, int T, int D, int S, const float* __restrict__ feats, int ld, const int* __restrict__ frames,
    const int* __restrict__ spk, double* __restrict__ stats, int* __restrict__ err) {
  const int s = blockIdx.x, tid = threadIdx.x;
  double sx[CMVN_COLS], sq[CMVN_COLS];
#pragma unroll
  for (int c = 0; c < CMVN_COLS; ++c) { sx[c] = 0.0; sq[c] = 0.0; }
  long long n = 0;
  for (int b = 0; b < B; ++b) {
    const int id = spk[b];  // uniform
    if (id < 0 || id >= S) {
      if (s == 0 && tid == 0) atomicOr(err, MLVAE_CMVN_ERR_SPEAKER);
      continue;
    }
    if (id != s) continue;
    const int Tb = clampi(frames[b], 0, T);
    const float* x = feats + (size_t)b * T * ld;
    for (int t = 0; t < Tb; ++t) {
#pragma unroll
      for (int c = 0; c < CMVN_COLS; ++c) {
        const int d = tid + c * NT;
        if (d < D) {
          const double v = (double)x[(size_t)t * ld + d];
          sx[c] += v;
          sq[c] += v * v;
        }
      }
    }
    n += Tb;
  }
  double* row = stats + (size_t)s * (2 * D + 1);
#pragma unroll
  for (int c = 0; c < CMVN_COLS; ++c) {
    const int d = tid + c * NT;
    if (d < D) { row[d] += sx[c]; row[D + d] += sq[c]; }
  }
  if (tid == 0) row[2 * D] += (double)n;
}

constexpr int CMVN_ROWS = 16;  // frames per workgroup of the apply kernel

__global__ __launch_bounds__(NT) void cmvn_apply_kernel(
    int T, int D, int S, float* __restrict__ feats, int ld, const int* __restrict__ frames,
    const int* __restrict__ spk, const double* __restrict__ stats, int* __restrict__ err) {
  const int b = blockIdx.y, t0 = blockIdx.x * CMVN_ROWS, tid = threadIdx.x;
  const int Tb = clampi(frames[b], 0, T);
  if (t0 >= Tb) return;  // uniform
  const int id = spk[b];
  if (id < 0 || id >= S) {
    if (tid == 0) atomicOr(err, MLVAE_CMVN_ERR_SPEAKER);
    return;
  }
  const double* row = stats + (size_t)id * (2 * D + 1);
  const double n = row[2 * D];
  if (!(n > 0.0)) {  // a speaker nothing was accumulated for
    if (tid == 0) atomicOr(err, MLVAE_CMVN_ERR_NO_STATS);
    return;
  }
  const int t1 = t0 + CMVN_ROWS < Tb ? t0 + CMVN_ROWS : Tb;
  for (int d = tid; d < D; d += NT) {
    const double mean = row[d] / n;
    const double var = fmax(row[D + d] / n - mean * mean, VAR_FLOOR);
    const float mf = (float)mean, sd = (float)sqrt(var);
    for (int t = t0; t < t1; ++t) {
      float* p = feats + ((size_t)b * T + t) * ld + d;
      *p = (*p - mf) / sd;
    }
  }
}

double hz_to_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

}  // namespace

extern "C" size_t mlvae_kaldi_fbank_table_size(int L, int P, int n_mels) {
  if (!geo_ok("mlvae_kaldi_fbank_table_size", 1, L, P, n_mels)) return 0;
  return table_floats(make_geo(1, L, P, n_mels)) * sizeof(float);
}

extern "C" size_t mlvae_kaldi_fbank_workspace_size(int B, int Nmax, int hop, int n_mels) {
  if (B < 0 || Nmax < 0 || hop < 1 || n_mels < 1) return 0;
  return (size_t)B * (size_t)frames_of(Nmax, hop) * n_mels * sizeof(float);
}

extern "C" int mlvae_kaldi_fbank_table(int sample_rate, int L, int P, int n_mels, float* host_table,
                                       size_t table_bytes) {
  if (!geo_ok("mlvae_kaldi_fbank_table", 1, L, P, n_mels)) return 1;
  if (sample_rate < 1 || sample_rate / 2.0 <= LOW_HZ) {
    mlvae_set_error("mlvae_kaldi_fbank_table: sample_rate = %d: the filters span %g Hz to sample_rate / 2",
                    sample_rate, LOW_HZ);
    return 1;
  }
  const Geo g = make_geo(1, L, P, n_mels);
  if (!host_table || table_bytes < table_floats(g) * sizeof(float)) {
    mlvae_set_error("mlvae_kaldi_fbank_table: host_table must hold %zu bytes", table_floats(g) * sizeof(float));
    return 1;
  }
  const double two_pi = 6.283185307179586476925286766559;
  // row n (frame sample n): hamming[n] cos / hamming[n] sin of 2 pi k n / P
  for (int n = 0; n < g.wr; ++n) {
    const double wn = n < L ? 0.54 - 0.46 * cos(two_pi * n / (L - 1)) : 0.0;
    float* row = host_table + (size_t)n * g.ldt;
    for (int bt = 0; bt < g.nbt; ++bt)
      for (int j = 0; j < 32; ++j) {
        const int k = bt * 32 + j;
        double c = 0.0, s = 0.0;
        if (k < g.K && n < L) {
          const int r = (int)(((long long)k * n) % P);  // the angle reduced in integers
          c = wn * cos(two_pi * r / P);
          s = wn * sin(two_pi * r / P);
        }
        row[bt * 64 + j] = (float)c;
        row[bt * 64 + 32 + j] = (float)s;
      }
  }
  // the triangular filters, [K][MELP]: bin k sits at mel(k sample_rate / P)
  float* fb = host_table + (size_t)g.wr * g.ldt;
  const double m_lo = hz_to_mel(LOW_HZ), m_hi = hz_to_mel(sample_rate / 2.0);
  const double step = (m_hi - m_lo) / (n_mels + 1);
  for (int k = 0; k < g.K; ++k) {
    const double m = hz_to_mel((double)k * ((double)sample_rate / P));
    for (int j = 0; j < MELP; ++j) {
      double wgt = 0.0;
      if (j < n_mels) {
        const double left = m_lo + step * j, centre = m_lo + step * (j + 1), right = m_lo + step * (j + 2);
        if (m > left && m <= centre) wgt = (m - left) / (centre - left);
        else if (m > centre && m < right) wgt = (right - m) / (right - centre);
      }
      fb[(size_t)k * MELP + j] = (float)wgt;
    }
  }
  return 0;
}

extern "C" int mlvae_kaldi_fbank(int B, int Nmax, const float* wav, int ld, const int* n_samples, int hop,
                                 int L, int P, int n_mels, int deltas, const float* table, float* out,
                                 int ldo, int* frames, void* ws, size_t ws_bytes, void* stream) {
  if (!geo_ok("mlvae_kaldi_fbank", hop, L, P, n_mels)) return 1;
  if (B < 0 || Nmax < 0 || ld < Nmax || ldo < (deltas ? 3 : 1) * n_mels) {
    mlvae_set_error("mlvae_kaldi_fbank: B, Nmax must be >= 0, ld >= Nmax and ldo >= the output columns");
    return 1;
  }
  if (B == 0) return 0;
  if (B > 65535) { mlvae_set_error("mlvae_kaldi_fbank: B = %d utterances, at most 65535 per call", B); return 1; }
  const long long Tmax_ll = frames_of(Nmax, hop);
  if (Tmax_ll > (1ll << 30)) { mlvae_set_error("mlvae_kaldi_fbank: %lld frames per row", Tmax_ll); return 1; }
  const int Tmax = (int)Tmax_ll;
  if ((!wav && Nmax > 0) || !n_samples || !table || !frames || ((!out || !ws) && Tmax > 0)) {
    mlvae_set_error("mlvae_kaldi_fbank: null pointer");
    return 1;
  }
  const size_t need = mlvae_kaldi_fbank_workspace_size(B, Nmax, hop, n_mels);
  if (ws_bytes < need) {
    mlvae_set_error("mlvae_kaldi_fbank: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return 1;
  }
  const Geo g = make_geo(hop, L, P, n_mels);
  const int ntiles = Tmax > 0 ? (Tmax + FT - 1) / FT : 1;  // one tile writes frames[] when Tmax = 0
  const size_t lds = lds_bytes(g);
  if (lds > 64 * 1024) {  // only the largest geometries pass the default dynamic-LDS limit
    if (hipFuncSetAttribute((const void*)kaldi_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess) {
      mlvae_set_error("mlvae_kaldi_fbank: cannot reserve %zu B LDS", lds);
      return 2;
    }
  }
  const dim3 grid(ntiles, B);
  if (Tmax > 0) {
    kaldi_tile_kernel<<<grid, NT, lds, (hipStream_t)stream>>>(g, Nmax, Tmax, wav, ld, n_samples, table,
                                                              (float*)ws);
    MLVAE_CHECK_LAUNCH();
  }
  kaldi_finish_kernel<<<grid, NT, 0, (hipStream_t)stream>>>(g, Nmax, Tmax, deltas ? 1 : 0, n_samples,
                                                            (const float*)ws, out, ldo, frames);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

static bool cmvn_ok(const char* who, int B, int T, int D, int S, int ld) {
  if (B < 0 || T < 0 || D < 1 || S < 1 || ld < D) {
    mlvae_set_error("%s: B, T must be >= 0, D, S >= 1 and ld >= D", who);
    return false;
  }
  if (D > CMVN_COLS * NT) { mlvae_set_error("%s: D = %d columns, at most %d", who, D, CMVN_COLS * NT); return false; }
  if (B > 65535) { mlvae_set_error("%s: B = %d utterances, at most 65535 per call", who, B); return false; }
  return true;
}

extern "C" int mlvae_cmvn_accumulate(int B, int T, int D, int S, const float* feats, int ld,
                                     const int* frames, const int* spk, double* stats, int* err,
                                     void* stream) {
  if (!cmvn_ok("mlvae_cmvn_accumulate", B, T, D, S, ld)) return 1;
  if (B == 0) return 0;
  if ((!feats && T > 0) || !frames || !spk || !stats || !err) {
    mlvae_set_error("mlvae_cmvn_accumulate: null pointer");
    return 1;
  }
  cmvn_accumulate_kernel<<<S, NT, 0, (hipStream_t)stream>>>(B, T, D, S, feats, ld, frames, spk, stats, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_cmvn_apply(int B, int T, int D, int S, float* feats, int ld, const int* frames,
                                const int* spk, const double* stats, int* err, void* stream) {
  if (!cmvn_ok("mlvae_cmvn_apply", B, T, D, S, ld)) return 1;
  if (B == 0 || T == 0) return 0;
  if (!feats || !frames || !spk || !stats || !err) {
    mlvae_set_error("mlvae_cmvn_apply: null pointer");
    return 1;
  }
  const dim3 grid((T + CMVN_ROWS - 1) / CMVN_ROWS, B);
  cmvn_apply_kernel<<<grid, NT, 0, (hipStream_t)stream>>>(T, D, S, feats, ld, frames, spk, stats, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
