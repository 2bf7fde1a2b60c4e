// The Hierarchical VAE's latent stretch as one streaming pass, forward and backward (DESIGN.md
// section 4, "The fused H-VAE latent kernel").
//
//   HierarchicalVAE.forward   ref:src/modules/h_vae.py:21-72
//   VanillaVAE.reparameterize / compute_kld_loss   ref:src/modules/vanilla_vae.py:37-45
//   GMMVAE.forward            ref:src/modules/gmm_vae.py:24-67
//   apply_weight              ref:src/utils/data_utils.py:32-64
//
// The composed path (elbo.hip reparam_kl, gmm.hip gmm_latent + apply_weight, torch.stack) writes
// the per-component z and kl [rows, N Z] and four stacked pairs to memory and reads them back; here
// a row's inputs are read once and only the collapsed, mixed outputs are written:
//   v      = (mean_v, log_var_v, eps_v e^{lv_v / 2} + mean_v, KL_v)            as reparam_kl_fwd
//   g[n]   = (m[n], lv[n], eps_g[n] e^{lv[n] / 2} + m[n], KL_g[n])             as gmm_latent_fwd
//   w      = (hard - y) + y,  y = softmax((logits + Gumbel) / tau)             as gmm_latent_fwd
//   G      = sum_n w[n] g[n]   (n ascending, from 0)                           as apply_weight_fwd
//   out    = pi0 v + pi1 G     (from 0)                                        as apply_weight_fwd
// ml == NULL && pi == NULL is the GMM-only mode: h = G_z, kl = G_kl, nothing else but w and ysoft.
//
// Rows to lanes.  A row is taken by a group of G lanes, G = the power of two >= min(Z, 64); a
// wave holds 64 / G rows (two at Z = 32), lane l of a group the columns l, l + G, ...: each group's
// loads and stores are consecutive.  The Gumbel-softmax of a row (N values) is evaluated by every
// lane of its group in gmm_latent_fwd's own order, so the weights are that kernel's bit for bit; it
// keeps no per-component array (the draws are recomputed per pass).  The backward's sums over the
// columns are xor-butterflies inside a group: a fixed order, no atomics.
#include "common.h"

namespace {

constexpr int GMM_MAX_N = 64;  // as gmm.hip

struct HvaeArgs {
  int rows, N, Z, ldml, ldp;
  const float* ml;     // [rows, ldml] = [mean_v | log_var_v]; NULL with pi: the GMM-only mode
  const float* P;      // [rows, ldp]  = [pm | plv | m | lv | logits]
  const float* pi;     // [rows, 2]
  const float* eps_v;  // [rows, Z]
  const float* eps_g;  // [rows, N*Z]
  const float* expo;   // [rows, N] Exp(1) draws, or NULL: Philox(seed, offset + r*N + n)
  unsigned long long seed, offset;
  float tau;
  float *mean, *log_var, *h, *kl;  // [rows, Z]
  float *w, *ysoft;                // [rows, N] (the backward reads them)
  // backward
  const float *d_mean, *d_log_var, *d_h, *d_kl;  // [rows, Z], NULL = 0
  const float* d_w;                              // [rows, N], NULL = 0
  float* dml;  // [rows, 2Z]
  float* dP;   // [rows, lddp]
  float* dpi;  // [rows, 2] or NULL
  int lddp;
  UttMap m; unsigned T;  // MAP: rows = B T frames of a shard (common.h UttMap)
};

// (logit + Gumbel) / tau of component n of row r (gr = the row's index in the draw stream)
__device__ __forceinline__ float gumbel_u(const HvaeArgs& a, const float* lg, size_t r,
                                          unsigned long long gr, int n) {
  const float e = a.expo ? a.expo[r * a.N + n] : exp1(a.seed, a.offset + gr * a.N + n);
  return (lg[n] + -logf(e)) / a.tau;
}

__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool MAP, bool HIER>
__global__ __launch_bounds__(256) void hvae_latent_fwd_kernel(HvaeArgs a, int G) {
  const int N = a.N, Z = a.Z, NZ = N * Z;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), sub = lane / G, rpw = 64 / G;
  const size_t nw = (size_t)gridDim.x * 4;
  for (size_t r0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw; r0 < (size_t)a.rows;
       r0 += nw * rpw) {
    const size_t r = r0 + sub;
    if (r >= (size_t)a.rows) continue;
    const float* p = a.P + r * a.ldp;
    const float* lg = p + 4 * NZ;
    // Gumbel-softmax in gmm_latent_fwd_kernel's order: max, sum (n ascending), first maximum
    const unsigned long long gr = MAP ? frame_global(a.m, r, a.T) : r;
    float mx = -INFINITY;
    for (int n = 0; n < N; ++n) {
      const float u = gumbel_u(a, lg, r, gr, n);
      if (u > mx) mx = u;
    }
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += expf(gumbel_u(a, lg, r, gr, n) - mx);
    float best = -1.f;
    int arg = 0;
    for (int n = 0; n < N; ++n) {
      const float y = expf(gumbel_u(a, lg, r, gr, n) - mx) / s;
      if (y > best) { best = y; arg = n; }
    }
    for (int n = gl; n < N; n += G) {
      const float y = expf(gumbel_u(a, lg, r, gr, n) - mx) / s;
      const float hard = n == arg ? 1.f : 0.f;
      a.w[r * N + n] = (hard - y) + y;
      a.ysoft[r * N + n] = y;
    }
    // the weights the collapse reads: (0 - y) + y of a finite y is 0, so only the chosen
    // component's needs its y
    const float yarg = expf(gumbel_u(a, lg, r, gr, arg) - mx) / s;
    const float warg = (1.f - yarg) + yarg;
    float pi0 = 0.f, pi1 = 0.f;
    if (HIER) { pi0 = a.pi[2 * r]; pi1 = a.pi[2 * r + 1]; }
    for (int c = gl; c < Z; c += G) {
      float gm = 0.f, gv = 0.f, gz = 0.f, gk = 0.f;
      for (int n = 0; n < N; ++n) {
        const int k = n * Z + c;
        const float pm = p[k], plv = p[NZ + k], m = p[2 * NZ + k], lv = p[3 * NZ + k];
        const float z = a.eps_g[r * NZ + k] * expf(0.5f * lv) + m;
        const float d = m - pm;
        const float kl = -0.5f * (1.f + lv - plv - (expf(lv) + d * d) / (expf(plv) + 1e-5f));
        const float wn = n == arg ? warg : 0.f;
        if (HIER) { gm += wn * m; gv += wn * lv; }
        gz += wn * z;
        gk += wn * kl;
      }
      if (HIER) {
        const float mu = a.ml[r * a.ldml + c], lv = a.ml[r * a.ldml + Z + c];
        const float zv = a.eps_v[r * Z + c] * expf(0.5f * lv) + mu;
        const float klv = -0.5f * (1.f + lv - mu * mu - expf(lv));
        float o;
        o = 0.f; o += pi0 * mu;  o += pi1 * gm; a.mean[r * Z + c] = o;
        o = 0.f; o += pi0 * lv;  o += pi1 * gv; a.log_var[r * Z + c] = o;
        o = 0.f; o += pi0 * zv;  o += pi1 * gz; a.h[r * Z + c] = o;
        o = 0.f; o += pi0 * klv; o += pi1 * gk; a.kl[r * Z + c] = o;
      } else {
        a.h[r * Z + c] = gz;
        a.kl[r * Z + c] = gk;
      }
    }
  }
}

// Recomputes v and g[n] from the saved inputs.  With D_key the cotangent of output `key`:
//   d v_key = pi0 D_key;  d g_key[n] = w[n] pi1 D_key;  t[n] = sum_key sum_c D_key[c] g_key[n, c]
//   dw[n] = d_w[n] + pi1 t[n] -> the logits through y (straight-through, as gmm_latent_bwd)
//   dpi0 = sum_key sum_c D_key[c] v_key[c];  dpi1 = sum_n w[n] t[n]
// Every lane of a wave runs every shuffle (rows past the end and columns past Z add zeros).
template <bool HIER>
__global__ __launch_bounds__(256) void hvae_latent_bwd_kernel(HvaeArgs a, int G) {
  const int N = a.N, Z = a.Z, NZ = N * Z;
  const int lane = threadIdx.x & 63, gl = lane & (G - 1), sub = lane / G, rpw = 64 / G;
  const size_t nw = (size_t)gridDim.x * 4;
  for (size_t r0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw; r0 < (size_t)a.rows;
       r0 += nw * rpw) {
    const size_t r = r0 + sub;
    const bool live = r < (size_t)a.rows;
    float pi0 = 0.f, pi1 = 1.f;
    if (HIER && live) { pi0 = a.pi[2 * r]; pi1 = a.pi[2 * r + 1]; }
    float dp0 = 0.f;
    if (HIER) {
      for (int c0 = 0; c0 < Z; c0 += G) {
        const int c = c0 + gl;
        if (live && c < Z) {
          const size_t i = r * Z + c;
          const float mu = a.ml[r * a.ldml + c], lv = a.ml[r * a.ldml + Z + c], ev = expf(lv);
          const float sd = expf(0.5f * lv), e = a.eps_v[i];
          const float Dm = a.d_mean ? a.d_mean[i] : 0.f, Dv = a.d_log_var ? a.d_log_var[i] : 0.f;
          const float Dh = a.d_h ? a.d_h[i] : 0.f, Dk = a.d_kl ? a.d_kl[i] : 0.f;
          dp0 += Dm * mu + Dv * lv + Dh * (e * sd + mu) + Dk * (-0.5f * (1.f + lv - mu * mu - ev));
          const float g = pi0 * Dh, sk = pi0 * Dk;
          a.dml[r * 2 * Z + c] = pi0 * Dm + g + sk * mu;
          a.dml[r * 2 * Z + Z + c] = pi0 * Dv + g * 0.5f * e * sd + sk * 0.5f * (ev - 1.f);
        }
      }
      dp0 = group_sum(dp0, G);
    }
    float sg = 0.f, dp1 = 0.f;
    for (int n = 0; n < N; ++n) {
      const float wn = live ? a.w[r * N + n] : 0.f, yn = live ? a.ysoft[r * N + n] : 0.f;
      const float sc = wn * pi1;
      float t = 0.f;
      for (int c0 = 0; c0 < Z; c0 += G) {
        const int c = c0 + gl;
        if (live && c < Z) {
          const size_t i = r * Z + c;
          const int k = n * Z + c;
          const float* p = a.P + r * a.ldp;
          const float pm = p[k], plv = p[NZ + k], m = p[2 * NZ + k], lv = p[3 * NZ + k];
          const float e = a.eps_g[r * NZ + k], sd = expf(0.5f * lv), ev = expf(lv), ep = expf(plv);
          const float D = ep + 1e-5f, d = m - pm;
          const float Dh = a.d_h ? a.d_h[i] : 0.f, Dk = a.d_kl ? a.d_kl[i] : 0.f;
          float Dm = 0.f, Dv = 0.f;
          if (HIER) { Dm = a.d_mean ? a.d_mean[i] : 0.f; Dv = a.d_log_var ? a.d_log_var[i] : 0.f; }
          t += Dm * m + Dv * lv + Dh * (e * sd + m) +
               Dk * (-0.5f * (1.f + lv - plv - (ev + d * d) / D));
          const float g = sc * Dh, sk = sc * Dk;
          float* q = a.dP + r * a.lddp;
          q[k] = -sk * d / D;                                          // d/d prior_mean
          q[NZ + k] = sk * 0.5f * (1.f - (ev + d * d) * ep / (D * D));   // d/d prior_log_var
          q[2 * NZ + k] = sc * Dm + g + sk * d / D;                      // d/d mean
          q[3 * NZ + k] = sc * Dv + g * 0.5f * e * sd - sk * 0.5f * (1.f - ev / D);  // d/d log_var
        }
      }
      t = group_sum(t, G);
      const float dwn = ((live && a.d_w) ? a.d_w[r * N + n] : 0.f) + pi1 * t;
      dp1 += wn * t;
      sg += dwn * yn;
      // parked in its own dP slot until sg is whole: written and read back by this one lane
      if (live && gl == 0) a.dP[r * a.lddp + 4 * NZ + n] = dwn;
    }
    if (live && gl == 0) {
      float* q = a.dP + r * a.lddp + 4 * NZ;
      const float* y = a.ysoft + r * N;
      for (int n = 0; n < N; ++n) q[n] = y[n] * (q[n] - sg) / a.tau;
      if (HIER && a.dpi) { a.dpi[2 * r] = dp0; a.dpi[2 * r + 1] = dp1; }
    }
  }
}

// the lanes of a row: the power of two >= min(Z, 64)
int group_of(int Z) {
  int G = 1;
  while (G < Z && G < 64) G <<= 1;
  return G;
}

int grid_of(int rows, int G) {
  const size_t per_block = (size_t)4 * (64 / G);
  size_t g = ((size_t)rows + per_block - 1) / per_block;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

bool bad_shape(const char* who, long long rows, int N, int Z, int ldp, const void* ml, int ldml,
               const void* pi) {
  if (rows < 0 || rows > 0x7fffffffll || N < 1 || N > GMM_MAX_N || Z < 1 || ldp < 4 * N * Z + N ||
      (ml && ldml < 2 * Z)) {
    mlvae_set_error("%s: bad shape rows=%lld N=%d Z=%d ldp=%d ldml=%d", who, rows, N, Z, ldp, ldml);
    return true;
  }
  if ((ml == nullptr) != (pi == nullptr)) {
    mlvae_set_error("%s: ml and pi go together (both NULL: the GMM-only mode)", who);
    return true;
  }
  return false;
}

int launch_fwd(const char* who, bool mapped, HvaeArgs& a, float* mean, float* log_var,
               void* stream) {
  const bool hier = a.ml != nullptr;
  if (!a.P || !a.eps_g || !a.h || !a.kl || !a.w || !a.ysoft ||
      (hier && (!a.eps_v || !mean || !log_var))) {
    mlvae_set_error("%s: null pointer", who);
    return 1;
  }
  if (a.rows == 0) return 0;
  a.mean = mean; a.log_var = log_var;
  const int G = group_of(a.Z), grid = grid_of(a.rows, G);
  hipStream_t st = (hipStream_t)stream;
  if (mapped) {
    if (hier) hvae_latent_fwd_kernel<true, true><<<grid, 256, 0, st>>>(a, G);
    else hvae_latent_fwd_kernel<true, false><<<grid, 256, 0, st>>>(a, G);
  } else {
    if (hier) hvae_latent_fwd_kernel<false, true><<<grid, 256, 0, st>>>(a, G);
    else hvae_latent_fwd_kernel<false, false><<<grid, 256, 0, st>>>(a, G);
  }
  return 0;
}

}  // namespace

extern "C" int mlvae_hvae_latent_fwd(int rows, int N, int Z, const float* ml, int ldml,
                                     const float* P, int ldp, const float* pi, const float* eps_v,
                                     const float* eps_g, const float* expo, unsigned long long seed,
                                     unsigned long long offset, float tau, float* mean,
                                     float* log_var, float* h, float* kl, float* w, float* ysoft,
                                     void* stream) {
  if (bad_shape("hvae_latent_fwd", rows, N, Z, ldp, ml, ldml, pi)) return 1;
  HvaeArgs a{};
  a.rows = rows; a.N = N; a.Z = Z; a.ldml = ldml; a.ldp = ldp; a.ml = ml; a.P = P; a.pi = pi;
  a.eps_v = eps_v; a.eps_g = eps_g; a.expo = expo; a.seed = seed; a.offset = offset; a.tau = tau;
  a.h = h; a.kl = kl; a.w = w; a.ysoft = ysoft;
  if (int rc = launch_fwd("hvae_latent_fwd", false, a, mean, log_var, stream)) return rc;
  MLVAE_CHECK_LAUNCH();
  return 0;
}

// The same over the rows = B T frames of a data-parallel shard (map: mlvae_gmm_latent_fwd_rows').
// The backward reads w and ysoft: it redraws nothing and needs no map.
extern "C" int mlvae_hvae_latent_fwd_rows(int B, int T, int N, int Z, const float* ml, int ldml,
                                          const float* P, int ldp, const float* pi,
                                          const float* eps_v, const float* eps_g, const float* expo,
                                          unsigned long long seed, const long long* map, float tau,
                                          float* mean, float* log_var, float* h, float* kl, float* w,
                                          float* ysoft, void* stream) {
  if (B < 0 || T < 0) {
    mlvae_set_error("hvae_latent_fwd_rows: bad shape B=%d T=%d", B, T);
    return 1;
  }
  if (bad_shape("hvae_latent_fwd_rows", (long long)B * T, N, Z, ldp, ml, ldml, pi)) return 1;
  HvaeArgs a{};
  if (!utt_map_load(map, B, &a.m, "hvae_latent_fwd_rows")) return 1;
  a.T = (unsigned)T;
  a.rows = B * T; a.N = N; a.Z = Z; a.ldml = ldml; a.ldp = ldp; a.ml = ml; a.P = P; a.pi = pi;
  a.eps_v = eps_v; a.eps_g = eps_g; a.expo = expo; a.seed = seed; a.offset = 0; a.tau = tau;
  a.h = h; a.kl = kl; a.w = w; a.ysoft = ysoft;
  if (int rc = launch_fwd("hvae_latent_fwd_rows", true, a, mean, log_var, stream)) return rc;
  MLVAE_CHECK_LAUNCH();
  return 0;
}

extern "C" int mlvae_hvae_latent_bwd(int rows, int N, int Z, const float* ml, int ldml,
                                     const float* P, int ldp, const float* pi, const float* eps_v,
                                     const float* eps_g, const float* w, const float* ysoft,
                                     float tau, const float* d_mean, const float* d_log_var,
                                     const float* d_h, const float* d_kl, const float* d_w,
                                     float* dml, float* dP, int lddp, float* dpi, void* stream) {
  if (bad_shape("hvae_latent_bwd", rows, N, Z, ldp, ml, ldml, pi)) return 1;
  if (lddp < 4 * N * Z + N) {
    mlvae_set_error("hvae_latent_bwd: bad shape lddp=%d", lddp);
    return 1;
  }
  const bool hier = ml != nullptr;
  if (!P || !eps_g || !w || !ysoft || !dP || (hier && (!eps_v || !dml))) {
    mlvae_set_error("hvae_latent_bwd: null pointer");
    return 1;
  }
  if (rows == 0) return 0;
  HvaeArgs a{};
  a.rows = rows; a.N = N; a.Z = Z; a.ldml = ldml; a.ldp = ldp; a.ml = ml; a.P = P; a.pi = pi;
  a.eps_v = eps_v; a.eps_g = eps_g; a.w = const_cast<float*>(w);
  a.ysoft = const_cast<float*>(ysoft); a.tau = tau;
  a.d_mean = d_mean; a.d_log_var = d_log_var; a.d_h = d_h; a.d_kl = d_kl; a.d_w = d_w;
  a.dml = dml; a.dP = dP; a.lddp = lddp; a.dpi = dpi;
  const int G = group_of(Z), grid = grid_of(rows, G);
  if (hier) hvae_latent_bwd_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(a, G);
  else hvae_latent_bwd_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(a, G);
  MLVAE_CHECK_LAUNCH();
  return 0;
}
