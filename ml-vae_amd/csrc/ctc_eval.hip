// The evaluation half of the CRDNN_CTC recipes (ref:src/models/CRDNN_CTC/model.py:60-176) on
// gfx950: greedy CTC decode, edit-distance alignment of the decoded sequence to the pronounced and
// the canonical phonemes, the MD / PER counts behind it, Viterbi over the CTC topology for the
// phoneme boundaries, and the plain log-softmax in front.  The reference runs these per utterance
// on the host on every batch of every stage (SpeechBrain's ctc_greedy_decode and edit_distance, the
// ctc_segmentation package); here they are members of the sequence-lattice family of align.hip.
//
// Form ("The CTC evaluation kernels").  One WAVE per utterance (edit_align:
// per utterance and reference), lane shifts instead of LDS exchange, no workgroup barrier inside a
// recursion.  Integers, or float64 sums of the fp32 emissions in frame order: a host oracle
// (tests/ctc_np.py) reproduces every output bit for bit, and a rerun is bit-identical (no atomics
// but the OR into the error word).  Workspaces belong to the caller.
//
// Greedy decode.  Lane l takes frame t0 + l of a 64-frame chunk and scans its C classes (strict >,
// so a tie keeps the lowest class); the class of the frame before comes over a lane shift (across
// chunks: carried from lane 63); kept frames (class != blank, != the frame before's) are compacted
// in frame order by a ballot and a prefix popcount.
//
// Edit alignment.  Levenshtein with unit costs over the (L_a + 1) x (L_b + 1) table, walked by
// anti-diagonals: lane l keeps rows [l RPL + 1, (l + 1) RPL] (row 0 is j, column 0 is i), of every
// row its value on the last two diagonals in registers; the row above a lane's first comes over a
// lane shift.  Tie rule at (i, j): the diagonal only if strictly below both others, else the
// deletion (from (i - 1, j)) if strictly below the insertion, else the insertion.  Two bits per
// cell (0 match, 3 substitution, 1 deletion, 2 insertion) go to the workspace, one word per lane
// and diagonal; the backtrace from (L_a, L_b) walks 64 diagonals at a time in LDS.
//
// CTC Viterbi.  align.hip's hmm_viterbi_kernel on the blank-interleaved chain of 2 L_b + 1 nodes:
// float64 delta, stay / next / skip (over a blank between two different classes), a tie keeps the
// earlier of that order; of the two end nodes a tie keeps the final blank.  Two backpointer bits
// per node and frame.
#include <math.h>
#include "common.h"

namespace {

constexpr int CE_MAX_REF = 1024;    // reference tokens of one alignment: 64 lanes x at most 16 rows
constexpr int CE_MAX_NODES = 1024;  // nodes of one CTC chain, as align.hip's
constexpr int CE_PF = 4;            // frames of gathered emissions in flight
constexpr float NINF = -INFINITY;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------ greedy decode
// grid B, one wave.  pred[b, :] = the kept classes in frame order, -1 behind them.
__global__ __launch_bounds__(64) void ctc_greedy_kernel(int T, int C, const float* __restrict__ pout, int ld,
                                                        const float* __restrict__ lens, int blank,
                                                        int* __restrict__ pred, int* __restrict__ pred_len) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = round_len(lens[b], T);
  const float* rows = pout + (size_t)b * T * ld;
  int* prow = pred + (size_t)b * T;
  int base = 0, carry = -1;  // wave-uniform: tokens written so far, the class of the frame before the chunk
  for (int t0 = 0; t0 < Tb; t0 += 64) {
    const int t = t0 + lane;
    int cls = -1;
    if (t < Tb) {
      const float* row = rows + (size_t)t * ld;
      float best = row[0];
      cls = 0;
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > best) {  // a tie keeps the lowest class
          best = v;
          cls = c;
        }
      }
    }
    int prev = __shfl_up(cls, 1, 64);
    if (lane == 0) prev = carry;
    const bool keep = t < Tb && cls != blank && cls != prev;
    const unsigned long long m = __ballot(keep);
    if (keep) prow[base + __popcll(m & ((1ull << lane) - 1ull))] = cls;  // < the frames seen <= T
    base += __popcll(m);
    carry = __shfl(cls, 63, 64);
  }
  for (int i = base + lane; i < T; i += 64) prow[i] = -1;
  if (lane == 0) pred_len[b] = base;
}

// ------------------------------------------------------------------ edit alignment
// grid (B, 2), one wave.  bt[b, r, d, lane]: bits 2k, 2k + 1 = the operation of cell
// (i = lane RPL + k + 1, j = d - i).
template <int RPL>
__global__ __launch_bounds__(64) void edit_align_kernel(int L, int Tp, const long long* __restrict__ refs,
                                                        const float* __restrict__ ref_lens,
                                                        const int* __restrict__ pred,
                                                        const int* __restrict__ pred_len, int* __restrict__ ali,
                                                        int* __restrict__ opsout, unsigned* __restrict__ bt) {
  __shared__ unsigned sh[64][65];
  __shared__ int sal[CE_MAX_REF];
  const int b = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
  const size_t br = (size_t)b * 2 + r;
  const long long* a = refs + br * L;
  const int* hyp = pred + (size_t)b * Tp;
  const int La = round_len(ref_lens[br], L);
  int Lb = pred_len[b];
  Lb = Lb < 0 ? 0 : (Lb > Tp ? Tp : Lb);
  int* arow = ali + br * L;
  unsigned* btrow = bt + br * (size_t)(L + Tp + 1) * 64;

  long long av[RPL];
  bool rowok[RPL];
#pragma unroll
  for (int k = 0; k < RPL; ++k) {
    const int i = lane * RPL + k + 1;
    rowok[k] = i <= La;
    av[k] = rowok[k] ? a[i - 1] : 0;
  }
  int p1[RPL], p2[RPL];  // D[i][d - 1 - i], D[i][d - 2 - i]
#pragma unroll
  for (int k = 0; k < RPL; ++k) p1[k] = p2[k] = 0;

  const int D = La + Lb;
  for (int d = 1; d <= D; ++d) {
    // the row above this lane's first on the last two diagonals; above row 1 is row 0: D[0][j] = j
    int up1 = __shfl_up(p1[RPL - 1], 1, 64), up2 = __shfl_up(p2[RPL - 1], 1, 64);
    if (lane == 0) {
      up1 = d - 1;
      up2 = d - 2;
    }
    unsigned word = 0;
    int cur[RPL];
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
      const int i = lane * RPL + k + 1, j = d - i;
      cur[k] = p1[k];
      if (rowok[k] && j >= 0 && j <= Lb) {
        if (j == 0) {
          cur[k] = i;  // column 0: deletions
        } else {
          const int up = k ? p1[k ? k - 1 : 0] : up1, dg = k ? p2[k ? k - 1 : 0] : up2, left = p1[k];
          const bool ne = av[k] != (long long)hyp[j - 1];
          const int sub = dg + (ne ? 1 : 0), del = up + 1, ins = left + 1;
          unsigned op;
          if (sub < del && sub < ins) {
            op = ne ? 3u : 0u;
            cur[k] = sub;
          } else if (del < ins) {
            op = 1u;
            cur[k] = del;
          } else {
            op = 2u;
            cur[k] = ins;
          }
          word |= op << (2 * k);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RPL; ++k) {
      p2[k] = p1[k];
      p1[k] = cur[k];
    }
    btrow[(size_t)d * 64 + lane] = word;
  }
  __syncthreads();  // the table of every lane is visible to the wave

  // backtrace from (L_a, L_b), 64 diagonals at a time; sal[i - 1] = the hypothesis position
  // aligned to reference position i - 1, -1 for a deletion; insertions are dropped
  int i = La, j = Lb, nI = 0, nD = 0, nS = 0;  // lane 0's
  for (int dc = (D / 64) * 64; dc >= 0; dc -= 64) {
    for (int q = 0; q < 64; ++q)
      if (dc + q >= 1 && dc + q <= D) sh[q][lane] = btrow[(size_t)(dc + q) * 64 + lane];
    __syncthreads();
    if (lane == 0) {
      while (i + j >= dc && (i > 0 || j > 0)) {
        if (i == 0) {
          --j;
          ++nI;
        } else if (j == 0) {
          sal[--i] = -1;
          ++nD;
        } else {
          const unsigned op = (sh[i + j - dc][(i - 1) / RPL] >> (2 * ((i - 1) % RPL))) & 3u;
          if (op == 1u) {
            sal[--i] = -1;
            ++nD;
          } else if (op == 2u) {
            --j;
            ++nI;
          } else {
            nS += op == 3u;
            sal[--i] = --j;
          }
        }
      }
    }
    __syncthreads();
  }
  for (int n = lane; n < L; n += 64) {
    int v = -1;
    if (n < La) {
      const int at = sal[n];
      v = at < 0 ? -1 : hyp[at];
    }
    arow[n] = v;
  }
  if (lane == 0) {
    int* o = opsout + br * 4;
    o[0] = nI;
    o[1] = nD;
    o[2] = nS;
    o[3] = La;
  }
}

// ------------------------------------------------------------------ MD / PER counts
// grid B, one wave.  counts[b] = (both correct, both mispronounced, missed, false alarm,
// positions pronounced canonically, of them recognised wrongly, positions mispronounced, of them
// recognised wrongly), over the alignment to the pronounced sequence (ali[b, 0, :]).
__global__ __launch_bounds__(64) void ctc_md_counts_kernel(int L, const long long* __restrict__ refs,
                                                           const float* __restrict__ ref_lens,
                                                           const int* __restrict__ ali, int* __restrict__ counts,
                                                           int* err) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long* phn = refs + (size_t)b * 2 * L;
  const long long* cn = phn + L;
  const int* al = ali + (size_t)b * 2 * L;
  const int Lp = round_len(ref_lens[2 * (size_t)b], L), Lc = round_len(ref_lens[2 * (size_t)b + 1], L);
  const int n = Lp < Lc ? Lp : Lc;
  int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = lane; i < n; i += 64) {
    const long long p = phn[i], q = cn[i], h = al[i];
    const bool pm = h != q, gm = p != q, wrong = h != p;
    c[0] += !pm && !gm;
    c[1] += pm && gm;
    c[2] += !pm && gm;
    c[3] += pm && !gm;
    c[4] += !gm;
    c[5] += !gm && wrong;
    c[6] += gm;
    c[7] += gm && wrong;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = wave_sum_i(c[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) counts[(size_t)b * 8 + k] = c[k];
    if (Lp != Lc) atomicOr(err, MLVAE_ERR_CTC_PAIR);
  }
}

// ------------------------------------------------------------------ Viterbi (CTC topology)
// grid B, one wave.  bp[b, t, lane] bits 2j, 2j + 1 = how node lane NPL + j at frame t was reached:
// 0 stay, 1 from the node below, 2 from two below (the skip).
template <int NPL>
__global__ __launch_bounds__(64) void ctc_viterbi_kernel(
    int T, int C, int L, const float* __restrict__ pout, int ld, const float* __restrict__ lens,
    const long long* __restrict__ phns, const float* __restrict__ phn_lens, int blank,
    float* __restrict__ vscore, int* __restrict__ boundary, int* __restrict__ infeasible,
    unsigned* __restrict__ bp, int* err) {
  __shared__ unsigned sh[64][65];
  __shared__ int bd[64];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = round_len(lens[b], T), Lb = round_len(phn_lens[b], L);
  const int N = 2 * Lb + 1;
  const long long* ph = phns + (size_t)b * L;
  int* brow = boundary + (size_t)b * T;

  bool bad = false, blk = false;
  for (int l = lane; l < Lb; l += 64) {
    const long long p = ph[l];
    bad |= p < 0 || p >= C;
    blk |= p == blank;
  }
  const int bits = (__any(bad) ? MLVAE_ERR_ALIGN_CLASS : 0) | (__any(blk) ? MLVAE_ERR_ALIGN_BLANK : 0);
  if (bits || Tb == 0) {  // a bad id is an error; no frames is a chain without a path
    for (int t = lane; t < T; t += 64) brow[t] = -1;
    if (lane == 0) {
      vscore[b] = 0.f;
      infeasible[b] = bits ? 0 : 1;
      if (bits) atomicOr(err, bits);
    }
    return;
  }

  int cl[NPL];
  bool valid[NPL], skip[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    const int n = lane * NPL + j;
    valid[j] = n < N;
    cl[j] = blank;
    skip[j] = false;
    if (valid[j] && (n & 1)) {
      cl[j] = (int)ph[n >> 1];  // in [0, C): checked above
      skip[j] = n >= 3 && ph[n >> 1] != ph[(n >> 1) - 1];
    }
  }
  const float* rows = pout + (size_t)b * T * ld;
  unsigned* bprow = bp + (size_t)b * T * 64;

  float e[CE_PF][NPL];
  auto gather = [&](float (&dst)[NPL], int t) {
    const float* row = rows + (size_t)t * ld;
#pragma unroll
    for (int j = 0; j < NPL; ++j) dst[j] = valid[j] ? row[cl[j]] : NINF;
  };
#pragma unroll
  for (int k = 0; k < CE_PF; ++k)
    if (k < Tb) gather(e[k], k);

  double d[NPL];
  const double DNINF = -INFINITY;
  for (int s0 = 0; s0 < Tb; s0 += CE_PF) {
#pragma unroll
    for (int k = 0; k < CE_PF; ++k) {
      const int t = s0 + k;
      if (t >= Tb) break;  // wave-uniform
      float cur[NPL];
#pragma unroll
      for (int j = 0; j < NPL; ++j) cur[j] = e[k][j];
      if (t + CE_PF < Tb) gather(e[k], t + CE_PF);
      unsigned word = 0;
      if (t == 0) {
#pragma unroll
        for (int j = 0; j < NPL; ++j) d[j] = (valid[j] && lane * NPL + j < 2) ? (double)cur[j] : DNINF;
      } else {
        double q1 = __shfl_up(d[NPL - 1], 1, 64);
        double q2 = NPL >= 2 ? __shfl_up(d[NPL >= 2 ? NPL - 2 : 0], 1, 64) : __shfl_up(d[0], 2, 64);
        if (lane == 0) q1 = q2 = DNINF;
        if (NPL == 1 && lane == 1) q2 = DNINF;
#pragma unroll
        for (int j = NPL - 1; j >= 0; --j) {
          // descending j: d[j - 1] and d[j - 2] still hold the previous frame
          const double one = j >= 1 ? d[j >= 1 ? j - 1 : 0] : q1;
          const double two = j >= 2 ? d[j >= 2 ? j - 2 : 0] : (j == 1 ? q1 : q2);
          double best = d[j];
          unsigned code = 0;  // a tie keeps stay, then next
          if (one > best) {
            best = one;
            code = 1;
          }
          if (skip[j] && two > best) {
            best = two;
            code = 2;
          }
          word |= valid[j] ? code << (2 * j) : 0u;
          d[j] = valid[j] ? best + (double)cur[j] : DNINF;
        }
      }
      bprow[(size_t)t * 64 + lane] = word;
    }
  }
  // the end nodes: the final blank N - 1 and the last phoneme N - 2; a tie keeps the blank
  auto node_value = [&](int n) {
    const int owner = n / NPL, slot = n % NPL;
    double v = DNINF;
#pragma unroll
    for (int j = 0; j < NPL; ++j) v = (j == slot) ? d[j] : v;
    return __shfl(v, owner, 64);
  };
  const double vb = node_value(N - 1);
  const double vp = N >= 2 ? node_value(N - 2) : DNINF;
  const bool last_phn = vp > vb;
  const double best = last_phn ? vp : vb;
  if (!(best > DNINF)) {  // no path: T_b too short for the chain
    const int m = Lb < Tb ? Lb : Tb;
    for (int t = lane; t < T; t += 64) brow[t] = t < m ? 1 : (t < Tb ? 0 : -1);
    if (lane == 0) {
      vscore[b] = 0.f;
      infeasible[b] = 1;
    }
    return;  // wave-uniform
  }
  if (lane == 0) {
    vscore[b] = (float)best;
    infeasible[b] = 0;
  }
  __syncthreads();  // the backpointers of every lane are visible to the wave
  int u = last_phn ? N - 2 : N - 1;  // lane 0's
  for (int tc = ((Tb - 1) / 64) * 64; tc >= 0; tc -= 64) {
    for (int r = 0; r < 64; ++r)
      if (tc + r < Tb) sh[r][lane] = bprow[(size_t)(tc + r) * 64 + lane];
    __syncthreads();
    if (lane == 0) {
      for (int r = 63; r >= 0; --r) {
        const int t = tc + r;
        if (t >= Tb) continue;
        const int code = t > 0 ? (int)((sh[r][u / NPL] >> (2 * (u % NPL))) & 3u) : 0;
        // frame 0 opens phoneme 0; phoneme k >= 1 opens where the path enters node 2 k + 1
        bd[r] = t == 0 ? (Lb >= 1) : (code != 0 && (u & 1) && u >= 3);
        u -= code;
      }
    }
    __syncthreads();
    if (tc + lane < Tb) brow[tc + lane] = bd[lane];
    __syncthreads();
  }
  for (int t = Tb + lane; t < T; t += 64) brow[t] = -1;
}

// ------------------------------------------------------------------ log-softmax over the last axis
// one wave per row, four rows per workgroup
__global__ __launch_bounds__(256) void lsm_fwd_kernel(int rows, int C, const float* __restrict__ x,
                                                      float* __restrict__ y) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* xr = x + (size_t)r * C;
  float* yr = y + (size_t)r * C;
  float m = NINF;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(xr[c] - m);
  s = wave_sum(s);
  const float lz = m + logf(s);
  for (int c = lane; c < C; c += 64) yr[c] = xr[c] - lz;
}

// dx[r, :] = dy[r, :] - exp(y[r, :]) sum_c dy[r, c]
__global__ __launch_bounds__(256) void lsm_bwd_kernel(int rows, int C, const float* __restrict__ dy,
                                                      const float* __restrict__ y, float* __restrict__ dx) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* gr = dy + (size_t)r * C;
  const float* yr = y + (size_t)r * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += gr[c];
  s = wave_sum(s);
  for (int c = lane; c < C; c += 64) dx[(size_t)r * C + c] = gr[c] - expf(yr[c]) * s;
}

// ------------------------------------------------------------------ host side
int pick_per_lane(int n) {
  int k = 1;
  while (64 * k < n) k *= 2;
  return k;  // 1, 2, 4, 8 or 16 for n <= 1024
}

}  // namespace

extern "C" int mlvae_ctc_greedy_decode(int B, int T, int C, const float* pout, int ld, const float* lens,
                                       int blank, int* pred, int* pred_len, void* stream) {
  if (B < 0 || T < 0 || C < 1 || ld < C) {
    mlvae_set_error("mlvae_ctc_greedy_decode: B, T must be >= 0, C >= 1 and ld >= C");
    return 1;
  }
  if (blank < 0 || blank >= C) {
    mlvae_set_error("mlvae_ctc_greedy_decode: blank %d outside [0, %d)", blank, C);
    return 1;
  }
  if (B == 0) return 0;
  if (!lens || !pred_len || (T > 0 && (!pout || !pred))) {
    mlvae_set_error("mlvae_ctc_greedy_decode: null pointer");
    return 1;
  }
  ctc_greedy_kernel<<<B, 64, 0, (hipStream_t)stream>>>(T, C, pout, ld, lens, blank, pred, pred_len);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_edit_align_max_ref(void) { return CE_MAX_REF; }

extern "C" size_t mlvae_edit_align_workspace_size(int B, int L, int Tp) {
  if (B < 0 || L < 0 || Tp < 0 || L > CE_MAX_REF) return 0;
  return (size_t)B * 2 * ((size_t)L + Tp + 1) * 64 * sizeof(unsigned);
}

extern "C" int mlvae_edit_align(int B, int L, int Tp, const long long* refs, const float* ref_lens,
                                const int* pred, const int* pred_len, int* ali, int* ops, void* ws,
                                size_t ws_bytes, void* stream) {
  if (B < 0 || L < 0 || Tp < 0) {
    mlvae_set_error("mlvae_edit_align: B, L, Tp must be >= 0");
    return 1;
  }
  if (L > CE_MAX_REF) {
    mlvae_set_error("mlvae_edit_align: a reference of %d tokens, the kernel holds at most %d (one wave keeps "
                    "the rows in registers)", L, CE_MAX_REF);
    return 1;
  }
  if (B == 0) return 0;
  if (!ref_lens || !pred_len || !ops || !ws || (L > 0 && (!refs || !ali)) || (Tp > 0 && !pred)) {
    mlvae_set_error("mlvae_edit_align: null pointer");
    return 1;
  }
  const size_t need = mlvae_edit_align_workspace_size(B, L, Tp);
  if (ws_bytes < need) {
    mlvae_set_error("mlvae_edit_align: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return 1;
  }
#define CE_EDIT(N_)                                                                                  \
  edit_align_kernel<N_><<<dim3(B, 2), 64, 0, (hipStream_t)stream>>>(L, Tp, refs, ref_lens, pred,    \
                                                                      pred_len, ali, ops, (unsigned*)ws)
  switch (pick_per_lane(L)) {
    case 1: CE_EDIT(1); break;
    case 2: CE_EDIT(2); break;
    case 4: CE_EDIT(4); break;
    case 8: CE_EDIT(8); break;
    default: CE_EDIT(16); break;
  }
#undef CE_EDIT
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_ctc_md_counts(int B, int L, const long long* refs, const float* ref_lens, const int* ali,
                                   int* counts, int* err, void* stream) {
  if (B < 0 || L < 0) {
    mlvae_set_error("mlvae_ctc_md_counts: B, L must be >= 0");
    return 1;
  }
  if (B == 0) return 0;
  if (!ref_lens || !counts || !err || (L > 0 && (!refs || !ali))) {
    mlvae_set_error("mlvae_ctc_md_counts: null pointer");
    return 1;
  }
  ctc_md_counts_kernel<<<B, 64, 0, (hipStream_t)stream>>>(L, refs, ref_lens, ali, counts, err);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t mlvae_ctc_viterbi_workspace_size(int B, int T) {
  if (B < 0 || T < 0) return 0;
  return (size_t)B * T * 64 * sizeof(unsigned);
}

extern "C" int mlvae_ctc_viterbi(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                                 const long long* phns, const float* phn_lens, int blank, float* vscore,
                                 int* boundary, int* infeasible, void* ws, size_t ws_bytes, int* err,
                                 void* stream) {
  if (B < 0 || T < 0 || L < 0 || C < 1 || ld < C) {
    mlvae_set_error("mlvae_ctc_viterbi: B, T, L must be >= 0, C >= 1 and ld >= C");
    return 1;
  }
  if (blank < 0 || blank >= C) {
    mlvae_set_error("mlvae_ctc_viterbi: blank %d outside [0, %d)", blank, C);
    return 1;
  }
  if (2 * (long long)L + 1 > CE_MAX_NODES) {
    mlvae_set_error("mlvae_ctc_viterbi: L = %d phonemes give a chain of more than %d nodes (one wave holds "
                    "the chain in registers)", L, CE_MAX_NODES);
    return 1;
  }
  if (B == 0) return 0;
  if (!lens || !phn_lens || !vscore || !infeasible || !err || (T > 0 && (!pout || !boundary || !ws)) ||
      (L > 0 && !phns)) {
    mlvae_set_error("mlvae_ctc_viterbi: null pointer");
    return 1;
  }
  const size_t need = mlvae_ctc_viterbi_workspace_size(B, T);
  if (ws_bytes < need) {
    mlvae_set_error("mlvae_ctc_viterbi: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return 1;
  }
#define CE_VIT(N_)                                                                                  \
  ctc_viterbi_kernel<N_><<<B, 64, 0, (hipStream_t)stream>>>(T, C, L, pout, ld, lens, phns, phn_lens, \
                                                             blank, vscore, boundary, infeasible,    \
                                                             (unsigned*)ws, err)
  switch (pick_per_lane(2 * L + 1)) {
    case 1: CE_VIT(1); break;
    case 2: CE_VIT(2); break;
    case 4: CE_VIT(4); break;
    case 8: CE_VIT(8); break;
    default: CE_VIT(16); break;
  }
#undef CE_VIT
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_log_softmax_fwd(int rows, int C, const float* x, float* y, void* stream) {
  if (rows < 0 || C < 1) {
    mlvae_set_error("mlvae_log_softmax_fwd: rows must be >= 0 and C >= 1");
    return 1;
  }
  if (rows == 0) return 0;
  if (!x || !y) {
    mlvae_set_error("mlvae_log_softmax_fwd: null pointer");
    return 1;
  }
  lsm_fwd_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(rows, C, x, y);
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_log_softmax_bwd(int rows, int C, const float* dy, const float* y, float* dx, void* stream) {
  if (rows < 0 || C < 1) {
    mlvae_set_error("mlvae_log_softmax_bwd: rows must be >= 0 and C >= 1");
    return 1;
  }
  if (rows == 0) return 0;
  if (!dy || !y || !dx) {
    mlvae_set_error("mlvae_log_softmax_bwd: null pointer");
    return 1;
  }
  lsm_bwd_kernel<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(rows, C, dy, y, dx);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
