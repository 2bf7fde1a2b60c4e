// Waveform -> log-mel filterbank + deltas + delta-deltas on gfx950: SpeechBrain 0.5's
// Fbank(deltas=True, context=False) (ref:src/config/run.yaml:39-44, applied per utterance at
// ref:src/utils/data_io.py:187-214) restated; SpeechBrain is not among the pinned references, so the
// pin is the float64 restatement tests/fbank_ref.py.  Per utterance b with N_b valid samples:
//
//   T_b = 1 + N_b / hop frames; frame t covers samples [t hop - n_fft/2, t hop + n_fft/2), zero
//   outside [0, N_b) (torch.stft center=True, pad_mode="constant"; the padding of a padded batch is
//   never read); periodic Hamming window of `win` points centred in n_fft; |X_k|^2, k = 0..n_fft/2;
//   triangular HTK-mel filters; dB = 10 log10(max(mel, 1e-10)), clamped from below at the
//   utterance's own maximum - 80; delta_t = sum_{k=-2..2} k x_{clamp(t+k, 0, T_b-1)} / 10, applied
//   twice.  out [B, Tmax, 3 n_mels] = (static | delta | delta-delta), rows t >= T_b exact zeros.
//
//   fbank_tile_kernel   one workgroup per (utterance, 32-frame tile): the frame tile [32, win] goes
//                       to LDS, X = frames . table (the windowed twiddles win[n] cos / win[n] sin,
//                       fp32 from a float64 host fill) on the exact-f32 MFMA, re and im of a bin in
//                       the same lane so |X|^2 forms in registers; |X|^2 to LDS, the mel projection
//                       and the log from there.  Only the unclamped dB tile and the tile's maximum
//                       leave the workgroup (workspace).
//   fbank_finish_kernel the utterance's maximum over its tiles, the clamp, both delta passes, the
//                       output rows and the zero rows.
//
// fp32 operands and accumulation throughout (the features span 70-80 dB: a bf16 rounding of the
// strongest bin would land on top of the weak ones).  The MFMA is a k-ordered fmaf chain; as in
// gemm.hip's fp32 mode the chain runs over KBLK samples and is then folded into a second
// accumulator.  No floating-point atomics, tiles are per utterance: an utterance's rows do not
// depend on the rest of the batch and a rerun is bit-identical.
#include <math.h>
#include "common.h"

namespace {

constexpr int FT = 32;        // frames per tile (one 32-row MFMA tile)
constexpr int NT = 256;       // threads
constexpr int NW = NT / 64;   // waves
constexpr int KBLK = 128;     // samples per MFMA chain before the fold
constexpr int GK = 16;        // samples per operand group of the DFT loop (double-buffered registers)
constexpr int MAX_FFT = 512;
constexpr int MAX_MELS = 64;
constexpr int MELP = 64;      // mel columns of the filter table (zero past n_mels)

struct Geo {
  int hop, win, n_fft, n_mels;
  int wr;    // window rows of the table: win rounded up to even (a zero row)
  int padl;  // first window sample inside the n_fft frame
  int K;     // bins n_fft/2 + 1
  int nbt;   // 32-bin tiles
  int ldt;   // table row: nbt x (32 re | 32 im)
  int lda;   // LDS frame row (odd: conflict-free column reads)
  int ldp;   // LDS power row
};

Geo make_geo(int hop, int win, int n_fft, int n_mels) {
  Geo g;
  g.hop = hop; g.win = win; g.n_fft = n_fft; g.n_mels = n_mels;
  g.wr = (win + 1) & ~1;
  g.padl = (n_fft - win) / 2;
  g.K = n_fft / 2 + 1;
  g.nbt = (g.K + 31) / 32;
  g.ldt = g.nbt * 64;
  g.lda = g.wr + 1;
  g.ldp = g.nbt * 32 + 1;
  return g;
}

bool geo_ok(const char* who, int hop, int win, int n_fft, int n_mels) {
  if (n_fft < 2 || (n_fft & 1) || n_fft > MAX_FFT) {
    mlvae_set_error("%s: n_fft = %d must be even and in [2, %d]", who, n_fft, MAX_FFT);
    return false;
  }
  if (win < 1 || win > n_fft) {
    mlvae_set_error("%s: the window (%d samples) must be in [1, n_fft = %d]", who, win, n_fft);
    return false;
  }
  if (n_mels < 1 || n_mels > MAX_MELS) {
    mlvae_set_error("%s: n_mels = %d must be in [1, %d]", who, n_mels, MAX_MELS);
    return false;
  }
  if (hop < 1) {
    mlvae_set_error("%s: hop = %d samples must be >= 1", who, hop);
    return false;
  }
  return true;
}

size_t table_floats(const Geo& g) { return (size_t)g.wr * g.ldt + (size_t)g.K * MELP; }
size_t lds_bytes(const Geo& g) { return ((size_t)FT * g.lda + (size_t)FT * g.ldp) * sizeof(float); }

__global__ __launch_bounds__(NT) void fbank_tile_kernel(
    Geo g, int Nmax, int Tmax, int ntiles, const float* __restrict__ wav, int ld,
    const int* __restrict__ n_samples, const float* __restrict__ table, float* __restrict__ ws_db,
    float* __restrict__ ws_max) {
  extern __shared__ float lds[];
  __shared__ float wmax[NW];
  float* As = lds;                // [FT][lda] the frames' window samples
  float* Ps = lds + FT * g.lda;   // [FT][ldp] |X|^2
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Nb = clampi(n_samples[b], 0, Nmax);
  const int Tb = 1 + Nb / g.hop;
  const int t0 = tile * FT;
  if (t0 >= Tb) return;  // uniform: the finish kernel reads tiles below ceil(T_b / FT) only

  // the frame tile: sample (t hop - n_fft/2 + padl + n) of the utterance, 0 outside [0, N_b)
  // (a wave per frame, the lanes along the window: up to MAX_FFT / 64 loads in flight per lane)
  const float* w = wav + (size_t)b * ld;
  for (int f = wave; f < FT; f += NW) {
    const long long s0 = (long long)(t0 + f) * g.hop - g.n_fft / 2 + g.padl;
    const bool live = t0 + f < Tb;
    float v[MAX_FFT / 64];
#pragma unroll
    for (int j = 0; j < MAX_FFT / 64; ++j) {
      const int n = lane + 64 * j;
      const long long s = s0 + n;
      v[j] = (live && n < g.win && s >= 0 && s < (long long)Nb) ? w[s] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < MAX_FFT / 64; ++j) {
      const int n = lane + 64 * j;
      if (n < g.wr) As[f * g.lda + n] = v[j];
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
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < FW; ++i) {
    const int t = t0 + wave * FW + i;
    if (lane < g.n_mels && t < Tb) {
      const float db = 10.f * log10f(fmaxf(mel[i], 1e-10f));
      ws_db[((size_t)b * Tmax + t) * g.n_mels + lane] = db;
      mx = fmaxf(mx, db);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < NW; ++i) mx = fmaxf(mx, wmax[i]);
    ws_max[(size_t)b * ntiles + tile] = mx;
  }
}

__global__ __launch_bounds__(NT) void fbank_finish_kernel(
    Geo g, int Nmax, int Tmax, int ntiles, const int* __restrict__ n_samples,
    const float* __restrict__ ws_db, const float* __restrict__ ws_max, float* __restrict__ out, int ldo,
    int* __restrict__ frames) {
  __shared__ float wmax[NW];
  const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Nb = clampi(n_samples[b], 0, Nmax);
  const int Tb = 1 + Nb / g.hop;
  if (tile == 0 && tid == 0) frames[b] = Tb;
  const int t0 = tile * FT;
  const int M = g.n_mels;
  float floor_db = 0.f;
  if (t0 < Tb) {  // uniform
    // the utterance's maximum over its own tiles (a maximum: exact in any order)
    const int nt = (Tb + FT - 1) / FT;
    float mx = -INFINITY;
    for (int i = tid; i < nt; i += NT) mx = fmaxf(mx, ws_max[(size_t)b * ntiles + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    mx = wmax[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) mx = fmaxf(mx, wmax[i]);
    floor_db = mx - 80.f;
  }
  const float* db = ws_db + (size_t)b * Tmax * M;
  auto stat = [&](int u, int m) { return fmaxf(db[(size_t)clampi(u, 0, Tb - 1) * M + m], floor_db); };
  auto delta = [&](int u, int m) {
    u = clampi(u, 0, Tb - 1);
    float s = 0.f;
#pragma unroll
    for (int k = -2; k <= 2; ++k) s += (float)k * stat(u + k, m);
    return s / 10.f;
  };
  for (int idx = tid; idx < FT * M; idx += NT) {
    const int f = idx / M, m = idx - f * M, t = t0 + f;
    if (t >= Tmax) break;
    float* o = out + ((size_t)b * Tmax + t) * ldo;
    float x = 0.f, d = 0.f, dd = 0.f;
    if (t < Tb) {
      x = stat(t, m);
      d = delta(t, m);
      float s = 0.f;
#pragma unroll
      for (int k = -2; k <= 2; ++k) s += (float)k * delta(t + k, m);
      dd = s / 10.f;
    }
    o[m] = x; o[M + m] = d; o[2 * M + m] = dd;
  }
}

double hz_to_mel(double f) { return 2595.0 * log10(1.0 + f / 700.0); }
double mel_to_hz(double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); }

}  // namespace

extern "C" size_t mlvae_fbank_table_size(int win, int n_fft, int n_mels) {
  if (!geo_ok("mlvae_fbank_table_size", 1, win, n_fft, n_mels)) return 0;
  return table_floats(make_geo(1, win, n_fft, n_mels)) * sizeof(float);
}

extern "C" size_t mlvae_fbank_workspace_size(int B, int Nmax, int hop, int n_mels) {
  if (B < 0 || Nmax < 0 || hop < 1 || n_mels < 1) return 0;
  const size_t Tmax = 1 + (size_t)Nmax / hop, ntiles = (Tmax + FT - 1) / FT;
  return ((size_t)B * Tmax * n_mels + (size_t)B * ntiles) * sizeof(float);
}

extern "C" int mlvae_fbank_table(int sample_rate, int win, int n_fft, int n_mels, float f_min,
                                 float f_max, float* host_table, size_t table_bytes) {
  if (!geo_ok("mlvae_fbank_table", 1, win, n_fft, n_mels)) return 1;
  if (sample_rate < 1 || !(f_min >= 0.f) || !(f_max > f_min)) {
    mlvae_set_error("mlvae_fbank_table: sample_rate = %d must be >= 1 and 0 <= f_min < f_max (%g, %g)",
                    sample_rate, (double)f_min, (double)f_max);
    return 1;
  }
  const Geo g = make_geo(1, win, n_fft, n_mels);
  if (!host_table || table_bytes < table_floats(g) * sizeof(float)) {
    mlvae_set_error("mlvae_fbank_table: host_table must hold %zu bytes", table_floats(g) * sizeof(float));
    return 1;
  }
  const double two_pi = 6.283185307179586476925286766559;
  // row n (window sample n, frame sample padl + n): win[n] cos / win[n] sin of 2 pi k (padl + n) / n_fft
  for (int n = 0; n < g.wr; ++n) {
    const double wn = n < win ? 0.54 - 0.46 * cos(two_pi * n / win) : 0.0;
    float* row = host_table + (size_t)n * g.ldt;
    for (int bt = 0; bt < g.nbt; ++bt)
      for (int j = 0; j < 32; ++j) {
        const int k = bt * 32 + j;
        double c = 0.0, s = 0.0;
        if (k < g.K && n < win) {
          // the angle reduced in integers: k (padl + n) mod n_fft
          const int r = (int)(((long long)k * (g.padl + n)) % n_fft);
          c = wn * cos(two_pi * r / n_fft);
          s = wn * sin(two_pi * r / n_fft);
        }
        row[bt * 64 + j] = (float)c;
        row[bt * 64 + 32 + j] = (float)s;
      }
  }
  // the triangular filters, [K][MELP]
  float* fb = host_table + (size_t)g.wr * g.ldt;
  const double m_lo = hz_to_mel(f_min), m_hi = hz_to_mel(f_max);
  double hz[MAX_MELS + 2];
  for (int i = 0; i < n_mels + 2; ++i) hz[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
  const double top = (double)(sample_rate / 2);
  for (int k = 0; k < g.K; ++k) {
    const double f = g.K > 1 ? top * k / (g.K - 1) : 0.0;
    for (int m = 0; m < MELP; ++m) {
      double wgt = 0.0;
      if (m < n_mels) {
        const double s = (f - hz[m + 1]) / (hz[m + 1] - hz[m]);
        wgt = fmax(0.0, fmin(s + 1.0, 1.0 - s));
      }
      fb[(size_t)k * MELP + m] = (float)wgt;
    }
  }
  return 0;
}

extern "C" int mlvae_fbank(int B, int Nmax, const float* wav, int ld, const int* n_samples, int hop,
                           int win, int n_fft, int n_mels, const float* table, float* out, int ldo,
                           int* frames, void* ws, size_t ws_bytes, void* stream) {
  if (!geo_ok("mlvae_fbank", hop, win, n_fft, n_mels)) return 1;
  if (B < 0 || Nmax < 0 || ld < Nmax || ldo < 3 * n_mels) {
    mlvae_set_error("mlvae_fbank: B, Nmax must be >= 0, ld >= Nmax and ldo >= 3 n_mels");
    return 1;
  }
  if (B == 0) return 0;
  if (B > 65535) { mlvae_set_error("mlvae_fbank: B = %d utterances, at most 65535 per call", B); return 1; }
  if ((!wav && Nmax > 0) || !n_samples || !table || !out || !frames || !ws) {
    mlvae_set_error("mlvae_fbank: null pointer");
    return 1;
  }
  const size_t need = mlvae_fbank_workspace_size(B, Nmax, hop, n_mels);
  if (ws_bytes < need) {
    mlvae_set_error("mlvae_fbank: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return 1;
  }
  const Geo g = make_geo(hop, win, n_fft, n_mels);
  const long long Tmax_ll = 1 + (long long)Nmax / hop;
  if (Tmax_ll > (1ll << 30)) { mlvae_set_error("mlvae_fbank: %lld frames per row", Tmax_ll); return 1; }
  const int Tmax = (int)Tmax_ll, ntiles = (Tmax + FT - 1) / FT;
  const size_t lds = lds_bytes(g);
  if (lds > 64 * 1024) {  // only the largest geometries pass the default dynamic-LDS limit
    if (hipFuncSetAttribute((const void*)fbank_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess) {
      mlvae_set_error("mlvae_fbank: cannot reserve %zu B LDS", lds);
      return 2;
    }
  }
  float* ws_db = (float*)ws;
  float* ws_max = ws_db + (size_t)B * Tmax * n_mels;
  const dim3 grid(ntiles, B);
  fbank_tile_kernel<<<grid, NT, lds, (hipStream_t)stream>>>(g, Nmax, Tmax, ntiles, wav, ld, n_samples,
                                                            table, ws_db, ws_max);
  MLVAE_CHECK_LAUNCH();
  fbank_finish_kernel<<<grid, NT, 0, (hipStream_t)stream>>>(g, Nmax, Tmax, ntiles, n_samples, ws_db,
                                                            ws_max, out, ldo, frames);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
