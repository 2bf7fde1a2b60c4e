/* mlvae.h -- C ABI of libmlvae.so, the MI355X (gfx950) kernels of the ML-VAE training step.
 *
 * Conventions
 *   - Every entry point returns int: 0 ok, 1 bad argument, 2 HIP launch/runtime error;
 *     the text of the last error of the calling thread is mlvae_last_error().
 *   - The caller owns every device buffer and workspace; the library never allocates.
 *   - Calls are stream-ordered on `stream` (a hipStream_t passed as void*) and reentrant.
 *   - Tensors are fp32, row-major [B*T, C] with row n = b*T + t (the reference's batch_first
 *     [B,T,C] layout, ref:src/modules/decoder.py:14), leading dimension in elements.
 *   - prec: 0 = fp32 (exact f32 MFMA, the parity mode), 1 = bf16 operands / fp32 accumulate.
 *
 * The reference is pure Python (SURVEY.md section 0): it has no FFI.  Each entry below names
 * the reference code whose work it replaces; the Python drop-in layer (ml-vae_amd/modules,
 * ml-vae_amd/models) binds these through ctypes (INTEGRATION.md).
 */
#ifndef MLVAE_H
#define MLVAE_H
#include <stddef.h>
#include "mlvae_err.h" /* the bits of the device error words, by name */
#ifdef __cplusplus
extern "C" {
#endif

const char* mlvae_last_error(void);
int mlvae_abi_version(void);
int mlvae_device_check(char* arch_out, int len);

/* C = epi(alpha*op(A).op(B) + bias1 + bias2 + beta*C).  trans_a: A stored [K][M];
 * trans_b: B stored [N][K].  epi 0 none, 1 LeakyReLU(0.01), 2 multiply by lrelu'(aux).
 * kshift/kshift_T (trans_b = 0): B row k reads row k+kshift when 0 <= k%T + kshift < T, else 0.
 * Replaces nn.Linear forward/backward (ref:src/modules/fc_block.py:10-16,
 * ref:src/modules/vanilla_vae.py:18-24) and the LSTM input projections and weight
 * gradients (ref:src/modules/decoder.py:14-15,22). */
size_t mlvae_gemm_workspace_size(int M, int N, int K);
int mlvae_gemm(int prec, int trans_a, int trans_b, int M, int N, int K, float alpha,
               const float* A, int lda, const float* B, int ldb, float beta, float* C, int ldc,
               const float* bias1, const float* bias2, int epi, const float* aux, int ldaux,
               int kshift_T, int kshift, float* ws, size_t ws_bytes, void* stream);

/* bf16-MFMA GEMM over bf16 or fp32 operands (a_bf16 / b_bf16: operand stored as bf16),
 * fp32 C, same epilogues / kshift / split-K as mlvae_gemm.  The bf16 precision mode's GEMMs:
 * the step keeps bf16 copies of its GEMM operands (h, dropout output, dG, weights).  Operand
 * rows along the contiguous dimension must be 16-byte aligned. */
size_t mlvae_gemm_ex_workspace_size(int M, int N, int K);
int mlvae_gemm_ex(int trans_a, int trans_b, int M, int N, int K, float alpha, const void* A,
                  int a_bf16, int lda, const void* B, int b_bf16, int ldb, float beta, float* C,
                  int ldc, const float* bias1, const float* bias2, int epi, const float* aux,
                  int ldaux, int kshift_T, int kshift, float* ws, size_t ws_bytes, void* stream);
/* The same with epilogue 3 = inter-layer dropout backward: C *= mask(drop_seed, drop_offset +
 * row*ldc + col)
 * with the mask of mlvae_dropout_ex (keep prob 1 - drop_p, scale 1/(1 - drop_p)), so the dgrad
 * of the layer above writes the gradient of the dropout input directly
 * (ref:src/modules/decoder.py:14, nn.LSTM dropout between layers in train mode). */
int mlvae_gemm_ex_drop(int trans_a, int trans_b, int M, int N, int K, float alpha,
                       const void* A, int a_bf16, int lda, const void* B, int b_bf16, int ldb,
                       float beta, float* C, int ldc, const float* bias1, const float* bias2,
                       int epi, const float* aux, int ldaux, int kshift_T, int kshift,
                       unsigned long long drop_seed, unsigned long long drop_offset, float drop_p,
                       float* ws, size_t ws_bytes, void* stream);
/* Large bf16 GEMMs (256 x 256 tiles, LDS-DMA staging, bf16 operands only, fp32 C):
 *   C_b = epi( op(A_b) op(B_b) + bias1 + bias2 + beta C_b ),  b = 0 .. batch-1
 * A_b = A + b*a_bstride (elements; strides may be negative), likewise B_b, C_b.  trans_a = 0: A [M,K] k-contiguous;
 * trans_a = 1: A stored [K,M].  trans_b = 1: B stored [N,K]; trans_b = 0: B stored [K,N].
 * kshift (+ b*kshift_bstep) time-shifts the rows of a [K,N] B operand as mlvae_gemm does.
 * epi as mlvae_gemm_ex_drop; 3 = dropout: C[row, col] of EVERY batch entry is multiplied by the
 * mlvae_dropout_ex mask of element drop_offset + row*ldc + col (ldc in elements of C; the index
 * does not depend on the batch entry).  drop_offset must be a multiple of 4 (the vector epilogues
 * take one mask quad per 4 columns); any other value is refused with status 1.  epi | 16
 * (EPI_OUT_F16) stores C as IEEE fp16 (C then points at fp16; beta 0, epi 0 or 3, N, ldc and
 * c_bstride multiples of 4 / 8, aligned C and biases): the input projection into the wide
 * recurrence's fp16 gate buffer (mlvae_lstm_gates_fp16).  epi | 32 (EPI_OUT_BF16) stores C as
 * bf16 (round to nearest even) under the same conditions with epi 0, 1 (LeakyReLU) or 3 (dropout):
 * the wav2vec2 layers' activations and the wide BPTT's dY; with N and ldc multiples of 8 a lane
 * stores 8 columns, else 4.  ldc and c_bstride count elements of C's type.  A 16-bit C with
 * beta != 0, another epilogue, N or ldc % 4 != 0, c_bstride % 8 != 0, or C / bias1 / bias2 off a
 * 16-byte boundary is refused with status 1 and C untouched.  Operands need
 * 16-byte aligned bases, lda/ldb and the contiguous extent multiples of 8.  Long-K products
 * split K into fp32 partial slabs (workspace: mlvae_gemm_bf16_workspace_size) reduced in a fixed
 * order.  Replaces the LSTM input projection, its dgrad and the weight gradients
 * (ref:src/modules/decoder.py:14-15,22). */
size_t mlvae_gemm_bf16_workspace_size(int M, int N, int K, int batch);
/* split-K planning target of mlvae_gemm_bf16 in workgroups (default 256, one per CU); returns
 * the previous value (values < 1 only query).  Host-side launch planning state: set it on the
 * launching thread right before the launches it should shape (the engine lowers it for weight
 * gradients that overlap a recurrence).  Workspace sizes assume the default or lower. */
int mlvae_gemm_bf16_set_split_target(int workgroups);
/* main-loop variant of mlvae_gemm_bf16 (0 = the default per operand layout; others are the
 * kernel's measured alternatives, for same-process A/B timing); returns the previous value
 * (values < 0 only query).  Initialised from MLVAE_GEMM_VAR.  Host-side planning state. */
int mlvae_gemm_bf16_set_variant(int var);
int mlvae_gemm_bf16(int trans_a, int trans_b, int M, int N, int K, int batch, const void* A,
                    int lda, long long a_bstride, const void* B, int ldb, long long b_bstride,
                    float* C, int ldc, long long c_bstride, float beta, const float* bias1,
                    const float* bias2, int epi, const float* aux, int ldaux, int kshift_T,
                    int kshift, int kshift_bstep, unsigned long long drop_seed,
                    unsigned long long drop_offset, float drop_p, float* ws, size_t ws_bytes,
                    void* stream);
/* y (bf16) = round-to-nearest-even(x), n elements. */
int mlvae_cast_bf16(size_t n, const float* x, void* y, void* stream);
/* y [cols, rows] (bf16) = transpose of x [rows, cols] (fp32, row-major): the k-contiguous copy of
 * an LSTM input weight that the dgrad dX = dG W_ih reads (ref:src/modules/decoder.py:14-15). */
int mlvae_cast_bf16_t(int rows, int cols, const float* x, void* y, void* stream);

/* Bidirectional LSTM layer recurrence, both directions in one persistent launch.
 * gates [B*T, 8H]: in = x W_ih^T + b_ih + b_hh (cols [0,4H) forward, [4H,8H) reverse);
 *                  out = activated gates i,f,g,o (saved for the backward).
 * cells [B*T, 2H], y [B*T, 2H] (forward half | reverse half) = nn.LSTM output.
 * xbuf: exchange workspace (size from mlvae_lstm_workspace_size); err: device int set to 1
 * if a hand-off wait timed out (the launch then completes with undefined outputs).
 * Replaces the recurrent part of nn.LSTM (ref:src/modules/decoder.py:22). */
int mlvae_lstm_workspace_size(int B, int H, int prec, size_t* xbytes);
int mlvae_lstm_fwd(int prec, int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev,
                   float* gates, float* cells, float* y, void* xbuf, size_t xbytes, int* err,
                   void* stream);
/* BPTT: gates in = activated gates from mlvae_lstm_fwd, out = pre-activation gate grads dG.
 * dy = gradient wrt the layer output y.  Weight/input grads follow as GEMMs on dG. */
int mlvae_lstm_bwd(int prec, int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev,
                   float* gates, const float* cells, const float* dy, void* xbuf, size_t xbytes,
                   int* err, void* stream);
/* _ex variants: the forward also writes h as bf16 (y_bf16 [B*T, 2H], may be NULL); the
 * backward writes dG as bf16 into dg_bf16 [B*T, 8H] instead of into gates (NULL: into gates).
 * The bf16 copies are the operands of the bf16-mode GEMMs (mlvae_gemm_ex). */
int mlvae_lstm_fwd_ex(int prec, int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev,
                      float* gates, float* cells, float* y, void* y_bf16, void* xbuf,
                      size_t xbytes, int* err, void* stream);
int mlvae_lstm_bwd_ex(int prec, int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev,
                      float* gates, const float* cells, const float* dy, void* dg_bf16,
                      void* xbuf, size_t xbytes, int* err, void* stream);
/* Unidirectional layer, nn.LSTM(bidirectional=False, batch_first=True): the phoneme
 * recogniser's and boundary detector's LSTMs (ref:src/modules/phoneme_recognizer.py:13,
 * ref:src/modules/boundary_detector.py:19) and the MD-VAE's 512-unit RNN (ref:src/models/MD_VAE/
 * model.yaml:78-83).  gates [B*T, 4H] fp32 (in: x W_ih^T + b_ih + b_hh; out: activated i,f,g,o;
 * the backward overwrites them with dG unless dg_bf16 != NULL), cells / y / dy [B*T, H].  Same
 * workspace, err word and batch chunking as mlvae_lstm_fwd. */
int mlvae_lstm1_fwd(int prec, int B, int T, int H, const float* w_hh, float* gates, float* cells,
                    float* y, void* y_bf16, void* xbuf, size_t xbytes, int* err, void* stream);
int mlvae_lstm1_bwd(int prec, int B, int T, int H, const float* w_hh, float* gates,
                    const float* cells, const float* dy, void* dg_bf16, void* xbuf, size_t xbytes,
                    int* err, void* stream);
/* A pair of independent unidirectional stacks of one shape in ONE launch (the joint recipes'
 * recogniser and detector LSTMs): the layout of mlvae_lstm_fwd_ex / _bwd_ex -- gates [B*T, 8H]
 * fp32 with stack a in columns [0,4H) and stack b in [4H,8H), cells / y / dy [B*T, 2H] with a
 * left and b right -- but both halves run forward in time: each half is exactly what
 * mlvae_lstm1_fwd / _bwd compute for its own w_hh.  Batch-group kernels, same workspace, err
 * word and batch chunking as mlvae_lstm_fwd. */
int mlvae_lstm_pair_fwd(int prec, int B, int T, int H, const float* w_hh_a, const float* w_hh_b,
                        float* gates, float* cells, float* y, void* y_bf16, void* xbuf,
                        size_t xbytes, int* err, void* stream);
int mlvae_lstm_pair_bwd(int prec, int B, int T, int H, const float* w_hh_a, const float* w_hh_b,
                        float* gates, const float* cells, const float* dy, void* dg_bf16,
                        void* xbuf, size_t xbytes, int* err, void* stream);
/* Wide-batch recurrence (csrc/lstm_wide.hip): one launch per layer for the whole batch when B is
 * past one batch-group launch (bf16, H = 512).  mlvae_lstm_gates_fp16(B, H, prec) = 1 for such
 * shapes; their gate buffer is IEEE fp16 [B*T, 8H] (half the projection's write and the
 * recurrences' reads) and they run only through the _ex2 entry points with gates_fp16 = 1.
 * gates_fp16 = 0 (and every entry point above) always runs the batch-group kernels on fp32
 * gates, batch-chunked.
 * fwd_ex2: y (fp32) may be NULL on the wide path; y_bf16 as _ex; y_drop_bf16 (wide path only,
 *   may be NULL) = bf16 dropout(h) for the next layer, mask of element drop_offset + row*2H + col
 *   from Philox(drop_seed) with keep 1 - drop_p -- the same mask mlvae_dropout_ex and the
 *   dropout epilogues (epi 3) draw, so the dgrad GEMM's epilogue recomputes it.
 * bwd_ex2: gates are the forward's (fp16 when gates_fp16); the wide backward writes dG only as
 *   bf16 into dg_bf16 (required) and, when dbias_rows != NULL (wide path only), the fp32 sums of
 *   dG over each batch group's 16 utterances and all T steps: dbias_rows [ceil(B/16)][8H], whose
 *   column sums are the layer's b_ih / b_hh gradients (ref:src/modules/decoder.py:14-15). */
int mlvae_lstm_gates_fp16(int B, int H, int prec);
/* The same for sequence length T: also 0 where T exceeds the wide kernels' 32-bit batch-group
 * addressing (16 T 8H fp16 gates >= 4 GB); the engine picks its gate buffer with it. */
int mlvae_lstm_gates_fp16_t(int B, int T, int H, int prec);
int mlvae_lstm_fwd_ex2(int prec, int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev,
                       void* gates, int gates_fp16, float* cells, float* y, void* y_bf16,
                       void* y_drop_bf16, unsigned long long drop_seed,
                       unsigned long long drop_offset, float drop_p, void* xbuf, size_t xbytes,
                       int* err, void* stream);
int mlvae_lstm_bwd_ex2(int prec, int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev,
                       void* gates, int gates_fp16, const float* cells, const float* dy,
                       void* dg_bf16, float* dbias_rows, void* xbuf, size_t xbytes, int* err,
                       void* stream);
/* bwd_ex3: bwd_ex2 with dy given as bf16 [B*T, 2H] when dy_bf16 = 1 (wide path only: gates_fp16 = 1;
 *   not with the fp8 BPTT) -- the fused engine's heads and dgrad GEMMs write dY in bf16, halving
 *   its bytes in their epilogues and in the BPTT's cell-input stream.  dy_bf16 = 0: bwd_ex2. */
int mlvae_lstm_bwd_ex3(int prec, int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev,
                       void* gates, int gates_fp16, const float* cells, const void* dy, int dy_bf16,
                       void* dg_bf16, float* dbias_rows, void* xbuf, size_t xbytes, int* err,
                       void* stream);
/* fp8 mode (BASELINE.json configs[4]) of the wide-batch recurrences (gates_fp16 shapes, bf16):
 *   fwd: as mlvae_lstm_fwd_ex2 without the fp32 h, plus y_drop_fp8 = e4m3(dropout(h) * x8_scale):
 *        the next layer's fp8 input-projection operand, written by the recurrence itself
 *        (replaces a cast pass over the bf16 copy; ref:src/modules/decoder.py:14-15,22);
 *        y_drop_bf16 may be NULL (the e4m3 copy alone: a step whose weight gradient of the next
 *        layer runs on e4m3 too reads no bf16 dropout(h))
 *   bwd: as mlvae_lstm_bwd_ex2, plus dg_fp8 = e4m3(dG * *dg8_scale) (NULL: none) -- the fp8
 *        dgrad's operand under delayed scaling -- and max |dG| max-ed into *dg_amax (float bits) */
int mlvae_lstm_fwd_fp8(int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev, void* gates,
                       float* cells, void* y_bf16, void* y_drop_bf16, void* y_drop_fp8, float x8_scale,
                       unsigned long long drop_seed, unsigned long long drop_offset, float drop_p,
                       void* xbuf, size_t xbytes, int* err, void* stream);
/* Wide forward of the bottom layer with its input projection fused (replaces the skinny
 * projection + mlvae_lstm_fwd_ex2 pair for ref:src/modules/decoder.py:22, nn.LSTM layer 0 whose
 * input is the 32-wide latent z): each step's gate inputs z_t W_ih^T + b_ih + b_hh are computed
 * inside the recurrence from z (bf16 [B*T rows, ldz], Z = 32), so the 8H-wide projection is
 * never written or read; gates receives the activated gates (fp16) as from mlvae_lstm_fwd_ex2.
 * y (fp32 h), y_drop_bf16 and y_drop_fp8 (with x8_scale > 0) are optional, each on its own. */
int mlvae_lstm_fwd_z(int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev, const void* z_bf16,
                     int ldz, int Z, const float* w_ih_fwd, const float* w_ih_rev, const float* b_ih_fwd,
                     const float* b_hh_fwd, const float* b_ih_rev, const float* b_hh_rev, void* gates,
                     float* cells, float* y, void* y_bf16, void* y_drop_bf16, void* y_drop_fp8, float x8_scale,
                     unsigned long long drop_seed, unsigned long long drop_offset, float drop_p, void* xbuf,
                     size_t xbytes, int* err, void* stream);
/* mlvae_lstm_fwd_z with y_bf16_prev = 1: y_bf16 row t receives the h ENTERING step t (h_{t-1} in
 * the forward direction, h_{t+1} in the reverse one, zeros at each utterance's first step) instead
 * of h_t -- the time-shifted operand of dW_hh_l0 = sum_t dG_t^T h_{t-/+1} pre-shifted, so that the
 * weight gradient runs as a plain (unshifted) product.  For a y_bf16 no other product reads (the
 * next layer's input is the dropout copy). */
int mlvae_lstm_fwd_z2(int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev, const void* z_bf16,
                      int ldz, int Z, const float* w_ih_fwd, const float* w_ih_rev, const float* b_ih_fwd,
                      const float* b_hh_fwd, const float* b_ih_rev, const float* b_hh_rev, void* gates,
                      float* cells, float* y, void* y_bf16, int y_bf16_prev, void* y_drop_bf16, void* y_drop_fp8,
                      float x8_scale, unsigned long long drop_seed, unsigned long long drop_offset, float drop_p,
                      void* xbuf, size_t xbytes, int* err, void* stream);
int mlvae_lstm_bwd_fp8(int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev, void* gates,
                       const float* cells, const float* dy, void* dg_bf16, float* dbias_rows,
                       void* dg_fp8, const float* dg8_scale, unsigned* dg_amax, void* xbuf,
                       size_t xbytes, int* err, void* stream);
/* mlvae_lstm_bwd_fp8 with dy as bf16 [B*T, 2H] when dy_bf16 = 1 (as mlvae_lstm_bwd_ex3).  Both
 * forms: dg_bf16 may be NULL when dg_fp8 is given (every dG reader on e4m3: the dgrad, dW_ih and
 * dW_hh through mlvae_gemm_fp8_tn_ex); the bias rows still come from the fp32 dG. */
int mlvae_lstm_bwd_fp8_ex(int B, int T, int H, const float* w_hh_fwd, const float* w_hh_rev, void* gates,
                          const float* cells, const void* dy, int dy_bf16, void* dg_bf16,
                          float* dbias_rows, void* dg_fp8, const float* dg8_scale, unsigned* dg_amax,
                          void* xbuf, size_t xbytes, int* err, void* stream);
/* Workgroups (one per CU, co-resident) of the recurrence launch for this shape as the engine
 * runs it (fp16 gates where mlvae_lstm_gates_fp16): the wide kernels fill the chip. */
int mlvae_lstm_launch_workgroups(int B, int H, int prec, int fwd);
/* Diagnostics: record per-step phase stamps of workgroup 0 into buf (NULL disables). */
int mlvae_lstm_set_debug(void* buf);

/* MD-VAE upstream-LSTM losses (csrc/md.hip).
 * mlvae_phn_bce: PhonemeRecognizer.compute_losses (ref:src/modules/phoneme_recognizer.py:35-81).
 *   logits [B,T,C] (row stride ldl), feat_lens / phn_lens [B] relative, phn [B,L] int64 ids,
 *   boundary [B,T] 0/1 (float).  Frame t < T_i = round(T feat_len) gets target one-hot(phn[b, k])
 *   with k = (boundaries in [0, t]) - 1; loss [B,T,C] = BCE-with-logits, 0 past T_i (may be NULL);
 *   with dloss given, dlogits = dloss (sigmoid(x) - y).  The reference's asserts set *err bits:
 *   MLVAE_ERR_MD_SEGMENTS = boundaries do not give L_i = round(L phn_len) segments from frame 0,
 *   MLVAE_ERR_MD_CLASS = phoneme id outside [0, C).
 * mlvae_boundary_fwd / _bwd: BoundaryDetector after its FC heads (ref:src/modules/boundary_detector.py:
 *   42-97).  za, zb [n] = pre-Softplus head outputs, y [n] boundary targets, u [10][n] U(0,1) draws
 *   (NULL: Philox(seed) at element offset + s*n + i).  Forward: v = mean of the ten clamped
 *   Kumaraswamy draws, bce = their mean BCE, kld = KL(Beta(alpha, beta) || Beta(1, 9)) (any output
 *   may be NULL).  Backward: dza, dzb from the cotangents dv, dbce, dkld (NULL = 0). */
int mlvae_phn_bce(int B, int T, int C, const float* logits, int ldl, const float* feat_lens,
                  const long long* phn, int L, const float* phn_lens, const float* boundary,
                  float* loss, const float* dloss, float* dlogits, int* err, void* stream);
int mlvae_boundary_fwd(size_t n, const float* za, const float* zb, const float* y, const float* u,
                       unsigned long long seed, unsigned long long offset, float* v, float* bce,
                       float* kld, void* stream);
int mlvae_boundary_bwd(size_t n, const float* za, const float* zb, const float* y, const float* u,
                       unsigned long long seed, unsigned long long offset, const float* dv,
                       const float* dbce, const float* dkld, float* dza, float* dzb, void* stream);

/* MD-VAE pi path (csrc/pi.hip; ref:src/models/MD_VAE/model.py:119-150).  logits [n,2] fp32,
 * contiguous and 8-byte aligned; n = B T frames; n == 0 is a no-op.
 * mlvae_pi_sample: sampled_pi [n,2] = the one-hot row [1 - label, label] of
 *   Categorical(logits = logits).  train != 0: label = (u >= p0), p0 = 1 / (1 + expf(l1 - l0)), u [n]
 *   the U(0,1) draws (NULL: the 24-bit Philox(seed) draw of element offset + i) -- label 1 with
 *   probability softmax(l)[1], exact at saturation (|l1 - l0| >= 160 never flips).  train == 0:
 *   label = (l1 > l0), torch.argmax (a tie gives 0).
 * mlvae_pi_nll_fwd: nll [n] = logsumexp(l0, l1) - l[label] = -Categorical.log_prob(label).  labels
 *   [n] int32 are mlvae_viterbi_md's flvl_out; -1 (past T_i) counts as 0 (pad_sequence's zero
 *   fill; the length mask removes those frames).  Any other label outside {0, 1} sets
 *   MLVAE_ERR_PI_LABEL in *err (log_prob raises for it) and counts as 0.
 * mlvae_pi_nll_bwd: dlogits [n,2], dlogits_k = dnll (softmax(l)_k - [k == label]). */
int mlvae_pi_sample(size_t n, const float* logits, const float* u, unsigned long long seed,
                    unsigned long long offset, int train, float* sampled_pi, void* stream);
int mlvae_pi_nll_fwd(size_t n, const float* logits, const int* labels, float* nll, int* err,
                     void* stream);
int mlvae_pi_nll_bwd(size_t n, const float* logits, const int* labels, const float* dnll,
                     float* dlogits, void* stream);

/* MD_VAE_sfl, the score-function (REINFORCE) estimator of the pi network (csrc/pi.hip;
 * ref:src/models/MD_VAE_sfl/model.py:139-187).  K = pi_mcmc_num draws per frame; every [K,n,..]
 * array is draw-major (draw k of frame i at index k n + i), fp32, contiguous.  n == 0 is a no-op.
 * mlvae_pi_sample_k: sampled_pi [K,n,2], K one-hot draws per frame.  Draw k of frame i uses
 *   u[k n + i] (u [K,n]; NULL: the Philox(seed) draw of element offset + k n + i): K = 1 is
 *   mlvae_pi_sample bit for bit.  train == 0 is the argmax and requires K == 1 (status 1 otherwise).
 * mlvae_sfl_fwd: with lp = log_softmax(logits[i]) and p = softmax(logits[i]),
 *     reward[k,i]      = -(w_recon mean_F(recon[k,i,:]) + w_kld mean_Z(kld[k,i,:]) + w_nll pi_nll[i])
 *     rif[i]           = (1/K) sum_k (reward[k,i] - baseline[i]) (-sum_c sampled_pi[k,i,c] lp_c)
 *     baseline_loss[i] = (1/K) sum_k (baseline[i] - reward[k,i])^2
 *     neg_entropy[i]   = sum_c p_c lp_c   (lp clamped to -FLT_MAX: exactly 0 at saturation)
 *   recon [K,n,F], kld [K,n,Z], any F, Z >= 1 (float4 reads when F % 4 == Z % 4 == 0 and both are
 *   16-byte aligned).  Fixed summation order, no atomics: a rerun is bit-identical.
 * mlvae_sfl_bwd: d_rif, d_ent, d_bl [n] are the gradients of rif, neg_entropy, baseline_loss;
 *     dlogits[i,c] = (d_rif/K) sum_k (reward[k,i] - baseline[i]) (p_c - sampled_pi[k,i,c])
 *                    + d_ent p_c (lp_c - sum_j p_j lp_j)
 *     dbaseline[i] = (2 d_bl/K) sum_k (baseline[i] - reward[k,i])
 *   The reward and the baseline inside rif are constants (the reference detaches them): recon,
 *   kld and pi_nll get no gradient. */
int mlvae_pi_sample_k(size_t n, int K, const float* logits, const float* u, unsigned long long seed,
                      unsigned long long offset, int train, float* sampled_pi, void* stream);
int mlvae_sfl_fwd(size_t n, int K, int F, int Z, const float* logits, const float* sampled_pi,
                  const float* recon, const float* kld, const float* pi_nll, const float* baseline,
                  float w_recon, float w_kld, float w_nll, float* reward, float* rif,
                  float* neg_entropy, float* baseline_loss, void* stream);
int mlvae_sfl_bwd(size_t n, int K, const float* logits, const float* sampled_pi, const float* reward,
                  const float* baseline, const float* d_rif, const float* d_ent, const float* d_bl,
                  float* dlogits, float* dbaseline, void* stream);

/* The LSTM_FC baseline's frame-level MD head (csrc/flvl.hip; ref:src/models/LSTM_FC/model.py:29-67):
 * the FCBlock's final Linear (two classes), the class-weighted BCE, the argmax and the MD counts,
 * for N = B T frames.  All arrays fp32 and contiguous unless said otherwise; any E >= 1 (float4
 * rows when E % 4 == 0 and h, w, dh are 16-byte aligned, scalar otherwise).  B, T < 0 or E < 1,
 * a null pointer and a workspace that is too small give status 1; B == 0 or T == 0 (N == 0) is a
 * no-op that returns 0.
 * mlvae_flvl_head_fwd: h [N,E], w [2,E], bias [2], labels [B,T] (floats, 0 or 1), lens [B]
 *   relative lengths (frame t of utterance b is valid iff (float)t < fp32(lens[b] T), as every
 *   masked mean here).  With x = logits[i,:] = h[i,:] w^T + bias and y = [1 - label, label]:
 *     loss_e[i,c] = pos_w_c y_c softplus(-x_c) + (1 - y_c) softplus(x_c)
 *       = F.binary_cross_entropy_with_logits(x, y, reduction='none', pos_weight=[pos_w0, pos_w1]),
 *       softplus(x) = max(x, 0) + log1pf(expf(-|x|)): finite at any logit; computed for padded
 *       frames too (the masked mean drops them);
 *     pred[b,t] int32 = (x_1 > x_0), torch.argmax (a tie gives 0); -1 past the utterance's length;
 *     counts[b,:] int32 = over the valid frames of utterance b: both correct (pred 0, label 0),
 *       both mispronounced (1, 1), missed (0, 1), false alarm (1, 0).  The entry zeroes counts
 *       on the stream first; integer atomics, exact in any order.
 *   A valid frame whose label is neither 0 nor 1 sets MLVAE_ERR_FLVL_LABEL in *err (it counts as 0); labels of
 *   padded frames are not looked at.
 * mlvae_flvl_head_bwd: logits [N,2] as the forward wrote them, dloss_e [N,2] the gradient of
 *   loss_e.  dlogits[i,c] = dloss_e[i,c] ((1 - y_c) sigma(x_c) - pos_w_c y_c (1 - sigma(x_c)));
 *   dh [N,E] = dlogits w, dw [2,E] = dlogits^T h, db [2] = sum_i dlogits[i,:].  dw and db are
 *   per-workgroup partial sums in ws (mlvae_flvl_head_workspace_size bytes, at most
 *   256 (2 E + 2) floats) added by a second kernel in workgroup order: no floating-point atomics,
 *   a rerun is bit-identical. */
size_t mlvae_flvl_head_workspace_size(int B, int T, int E);
int mlvae_flvl_head_fwd(int B, int T, int E, const float* h, const float* w, const float* bias,
                        const float* labels, const float* lens, float pos_w0, float pos_w1,
                        float* logits, float* loss_e, int* pred, int* counts, int* err, void* stream);
int mlvae_flvl_head_bwd(int B, int T, int E, const float* h, const float* w, const float* logits,
                        const float* labels, const float* dloss_e, float pos_w0, float pos_w1,
                        float* dh, float* dw, float* db, void* ws, size_t ws_bytes, void* stream);

/* MD-VAE Viterbi decode (csrc/decode.hip): decode_plvl_md_lbl_seqs_full
 * (ref:src/utils/decode_utils.py:374-565, run in the MD-VAE forward at ref:src/models/MD_VAE/
 * model.py:133-141).  logits [B,T,N] (phoneme recogniser output, row stride ldl), boundary_v
 * [B,T], pi_logits [B,T,2], prior [N], seqs [B,L] int64 canonical ids, feat_lens / seq_lens [B]
 * relative, weight = dec_weight.  Outputs (int32): boundary_out [B,T] decoded boundaries (0/1),
 * flvl_out [B,T] frame-level and plvl_out [B,L] phoneme-level mispronunciation labels (-1 past
 * T_i / L_i), lens_out [B,2] = (T_i, L_i).  ws: mlvae_viterbi_workspace_size(B,T,L) bytes (the
 * argmax path map).  *err bits: MLVAE_ERR_DECODE_BACKTRACK = the backtrack did not end at (l, t) =
 * (0, 0) (the reference's assert), MLVAE_ERR_DECODE_EMPTY = T_i or L_i empty / L_i > 1024.  L <= 1024. */
size_t mlvae_viterbi_workspace_size(int B, int T, int L);
int mlvae_viterbi_md(int B, int T, int N, int L, const float* logits, int ldl, const float* boundary_v,
                     const float* pi_logits, const float* prior, const long long* seqs,
                     const float* feat_lens, const float* seq_lens, float weight, void* ws,
                     size_t ws_bytes, int* boundary_out, int* flvl_out, int* plvl_out, int* lens_out,
                     int* err, void* stream);

int mlvae_viterbi_md_ex(int B, int T, int N, int L, const float* logits, int ldl,
                        const float* boundary_v, const float* pi_logits, const float* prior,
                        const long long* seqs, const float* feat_lens, const float* seq_lens,
                        float weight, int skip_empty, void* ws, size_t ws_bytes, int* boundary_out,
                        int* flvl_out, int* plvl_out, int* lens_out, int* err, void* stream);

/* Data-parallel shards of the MD recipes: the random streams over an utterance map.
 * Every stream above is indexed over the utterances of the single-process batch.  A shard names
 * the ones it holds with map = four values (utt_offset, seg_utts, seg_stride, total_utts), a host
 * pointer, NULL = the identity: local utterance u of the shard's B is utterance
 *     g(u) = (u / seg_utts) seg_stride + utt_offset + u % seg_utts
 * of total_utts.  Rank r holding B_l of B_g utterances: (r B_l, B_l, B_l, B_g); MD_VAE_sfl's folded
 * [K B_l, T, .] batch: (r B_l, B_l, B_g, K B_g).  With T frames per utterance the element counters
 * are g T + t (frame streams), s total_utts T + g T + t (draw-major: the ten boundary draws, the K
 * pi draws) and (g T + t) C + c (row-major [.., C]), so a shard draws bit for bit the slice of
 * what the single process draws, and with the identity map each entry equals the one it extends
 * (at offset 0).  Draws are per element: any C, any shard boundary.  Injected draws (u, expo) are
 * the shard's own arrays, indexed locally.  seg_utts < 1, seg_stride < 1, utt_offset < 0 or
 * total_utts < 1 give status 1; g(u) >= total_utts is allowed (the zero-length fillers of a short
 * rank slice: their draws repeat counters of real utterances and are masked out by the lengths).
 * B T C == 0 is a no-op.
 * mlvae_randn_rows: out [B,T,C], the mlvae_randn stream.
 * mlvae_dropout_rows: y = x * mask [B,T,C], the mlvae_dropout mask (the LSTM's inter-layer
 *   dropout, rows 2H or H wide; the backward applies it to the gradient, y == x allowed).
 * mlvae_pi_sample_rows: mlvae_pi_sample_k over logits [B,T,2], sampled_pi [K,B,T,2].
 * mlvae_boundary_fwd_rows / _bwd_rows: mlvae_boundary_fwd / _bwd over [B,T], u [10,B,T].
 * mlvae_gmm_latent_fwd_rows: mlvae_gmm_latent_fwd over rows = B T (B T <= INT_MAX); the backward
 *   redraws nothing (it reads ysoft) and takes no map.
 * mlvae_viterbi_md_ex (declared above): skip_empty != 0 makes a row with T_i == 0 and L_i == 0 --
 *   the zero-length filler of a short rank slice -- write -1 everywhere and lens_out (0, 0)
 *   without an error bit; every other empty or oversized row still sets MLVAE_ERR_DECODE_EMPTY.  skip_empty == 0
 *   is mlvae_viterbi_md. */
int mlvae_randn_rows(int B, int T, int C, unsigned long long seed, const long long* map, float* out,
                     void* stream);
int mlvae_dropout_rows(int B, int T, int C, const float* x, float* y, unsigned long long seed, float p,
                       const long long* map, void* stream);
int mlvae_pi_sample_rows(int B, int T, int K, const float* logits, const float* u,
                         unsigned long long seed, const long long* map, int train, float* sampled_pi,
                         void* stream);
int mlvae_boundary_fwd_rows(int B, int T, const float* za, const float* zb, const float* y,
                            const float* u, unsigned long long seed, const long long* map, float* v,
                            float* bce, float* kld, void* stream);
int mlvae_boundary_bwd_rows(int B, int T, const float* za, const float* zb, const float* y,
                            const float* u, unsigned long long seed, const long long* map,
                            const float* dv, const float* dbce, const float* dkld, float* dza,
                            float* dzb, void* stream);
int mlvae_gmm_latent_fwd_rows(int B, int T, int N, int Z, const float* P, int ldp, const float* eps,
                              const float* expo, unsigned long long seed, const long long* map,
                              float tau, float* z, float* kl, float* w, float* ysoft, void* stream);

/* fp8 GEMM mode (BASELINE.json configs[4], csrc/gemm_fast.hip VAR 8 + csrc/fp8.hip): the decoder's
 * layer-1 input projection (ref:src/modules/decoder.py:14-15,22, nn.LSTM's x W_ih^T) on fp8 e4m3
 * (OCP) operands with per-tensor scales, v_mfma_scale_f32_16x16x128_f8f6f4, fp32 accumulate.
 *   gemm_fp8:  C = (*alpha) * A . B^T + bias1 + bias2, A [M][K], B [N][K] fp8 (k-contiguous,
 *              K, lda, ldb % 16, 16-byte aligned); C fp32, or fp16 with epi = 16 (EPI_OUT_F16).
 *   fp8_scale: out[0] = q = 448 / max|x| (1 if 0 / non-finite), out[1] = 1 / (q * other_scale).
 *   cast_fp8:  dst = e4m3(clamp(src * scale, +-448)), RNE; scale = *scale_p if non-null. */
int mlvae_gemm_fp8(int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                   const float* alpha, const float* bias1, const float* bias2, int epi, void* stream);
/* As mlvae_gemm_fp8 with epi = EPI_DROPOUT allowed (fp32 or, with the EPI_OUT_BF16 flag 32, bf16
 * C): C *= the inter-layer dropout mask of element drop_offset + row * ldc + col (drop_offset a
 * multiple of 4, as mlvae_gemm_bf16: any other value is refused) -- the fp8
 * layer-1 dgrad with the dropout backward fused (ref:src/modules/decoder.py:14-15: the dropout
 * between the LSTM layers); bf16 C is the wide BPTT's dY input (mlvae_lstm_bwd_ex3). */
int mlvae_gemm_fp8_ex(int M, int N, int K, const void* A, int lda, const void* B, int ldb, void* C,
                      int ldc, const float* alpha, const float* bias1, const float* bias2, int epi,
                      unsigned long long drop_seed, unsigned long long drop_offset, float drop_p,
                      void* stream);
/* C [M][N] (fp32) = (*alpha) * A^T B over fp8 e4m3 operands stored [K][M] and [K][N] (m- and
 * n-contiguous rows of lda / ldb bytes): the layer-1 weight gradient dW_ih = dG^T X over the K
 * frames (ref:src/modules/decoder.py:14-15,22, nn.LSTM's W_ih gradient) on the e4m3 dG the fp8
 * BPTT writes and the e4m3 layer input the forward writes.  M, N, lda, ldb % 16, 16-byte aligned
 * operands; deterministic split-K through ws (mlvae_gemm_fp8_tn_workspace_size bytes). */
size_t mlvae_gemm_fp8_tn_workspace_size(int M, int N, int K);
int mlvae_gemm_fp8_tn(int M, int N, int K, const void* A, int lda, const void* B, int ldb, float* C, int ldc,
                      const float* alpha, float* ws, size_t ws_bytes, void* stream);
/* mlvae_gemm_fp8_tn batched (A + z a_bstride, B + z b_bstride bytes, C + z c_bstride floats) with
 * time-shifted B rows: row k of B_z is read at k + sh_z, sh_z = kshift + z kshift_bstep, when
 * 0 <= k % kshift_T + sh_z < kshift_T, else as zeros (K % kshift_T == 0): the recurrent weight
 * gradients dW_hh = sum_t dG_t^T h_{t-1} (forward) / h_{t+1} (reverse) of both directions in one
 * launch on e4m3 dG and h (ref:src/modules/decoder.py:14-15,22; the bf16 form: mlvae_gemm_bf16's
 * kshift arguments).  Strides % 16; workspace mlvae_gemm_fp8_tn_ex_workspace_size bytes. */
size_t mlvae_gemm_fp8_tn_ex_workspace_size(int M, int N, int K, int batch);
int mlvae_gemm_fp8_tn_ex(int M, int N, int K, int batch, const void* A, int lda, long long a_bstride,
                         const void* B, int ldb, long long b_bstride, float* C, int ldc, long long c_bstride,
                         const float* alpha, int kshift_T, int kshift, int kshift_bstep, float* ws,
                         size_t ws_bytes, void* stream);
size_t mlvae_fp8_scale_workspace_size(void);
int mlvae_fp8_scale(size_t n, const float* x, float other_scale, float* out, float* ws, size_t ws_bytes,
                    void* stream);
int mlvae_cast_fp8(size_t n, const void* src, int src_bf16, const float* scale_p, float scale, void* dst,
                   void* stream);
/* Delayed (previous-step) scaling: from an amax word a producer max-ed (float bits),
 * out[0] = q = 448 / (margin * amax_prev) (1 without a usable amax), out[1] = 1 / (q * *other_q)
 * (the fp8 GEMM's alpha); *amax_next (distinct word, optional) is cleared for this step's producer. */
int mlvae_fp8_delayed_scale(const unsigned* amax_prev, unsigned* amax_next, const float* other_q,
                            float margin, float* out, void* stream);

/* Conv1d encoder layers (csrc/conv.hip), BASELINE.json configs[3]'s "Conv1d encoder variant":
 * the reference has none (SURVEY.md Appendix A); semantics = torch.nn.Conv1d(Cin, Cout, K,
 * padding=(K-1)/2) over each utterance of the batch-first frames [B, T, C] (row b*T + t), zero
 * outside [0, T).  This replaces the encoder's Linear layers (ref:src/modules/vanilla_vae.py:13-16,
 * FCBlock ref:src/modules/fc_block.py:4-21) in modules/conv_vae.py.  w: torch layout
 * [Cout][Cin][K] fp32; activations fp32, bf16 MFMA operands, fp32 accumulate.
 *   fwd:   y = act(conv(x) + bias)                      act: 1 = LeakyReLU(0.01)
 *   dgrad: dx = conv^T(dy) [* lrelu'(aux)]              (aux = the layer input's LReLU output)
 *   wgrad: dw = sum over frames, db = column sums of dy  (overwritten; deterministic)
 * Limits: K odd <= 9, Cin % 4 == 0 and <= 128, Cout % 16 == 0 and <= 128, 16-byte aligned
 * rows; wgrad: Cout in {16, 32, 64}, K * roundup(Cin, 16) <= 512 (mlvae_conv1d_supported). */
int mlvae_conv1d_supported(int Cin, int Cout, int K);
int mlvae_conv1d_fwd(int B, int T, int Cin, int Cout, int K, const float* x, int ldx, const float* w,
                     const float* bias, int act, float* y, int ldy, void* stream);
int mlvae_conv1d_dgrad(int B, int T, int Cin, int Cout, int K, const float* dy, int lddy, const float* w,
                       const float* aux, int ldaux, float* dx, int lddx, void* stream);
size_t mlvae_conv1d_wgrad_workspace_size(int B, int T, int Cin, int Cout, int K);
int mlvae_conv1d_wgrad(int B, int T, int Cin, int Cout, int K, const float* dy, int lddy, const float* x,
                       int ldx, float* dw, float* db, void* ws, size_t ws_bytes, void* stream);
/* The CRDNN's convolutional front end (csrc/conv2d.hip): the Conv2d / LayerNorm / pooling blocks
 * the CRDNN_CTC recipes' yaml asks of SpeechBrain's CRDNN lobe (ref:src/models/CRDNN_CTC/model.yaml:23-35).
 * Activations channels-last [B][T][F][C], contiguous fp32, 16-byte aligned; no utterance lengths
 * (the convolution runs over the padded batch).
 *   conv2d: 3x3, stride 1, "same", reflect padding 1 on T and F (x[-1] = x[1], x[T] = x[T-2]);
 *     w torch layout [Cout][Cin][3 (time)][3 (freq)] fp32; bf16 MFMA operands, fp32 accumulate.
 *     fwd:   y = conv(x) + bias          dgrad: dx = conv^T(dy) (border rows folded onto their sources)
 *     wgrad: dw, db (db optional) overwritten; deterministic (fixed-order sums, no atomics)
 *     Limits: Cin, Cout multiples of 16 in [16, 256] (mlvae_conv2d_supported), T >= 2, F >= 2.
 *     workspace_size(op, ...): op 0 = fwd, 1 = dgrad, 2 = wgrad.
 *   conv2d_first: the Cin = 1 layer on x [B][T][F]: direct fp32 kernels, forward and weight + bias
 *     gradient (w [Cout][1][3][3]); Cout a multiple of 16 up to 256.
 *   ln_fc_act: y = LeakyReLU_0.01(LayerNorm_(F,C)(x) * gamma + beta), one row per (b, t), rows =
 *     B T, gamma / beta [F][C], biased variance; mean / rstd [rows] saved.  pool = 1: then the
 *     frequency max-pool 2 (stride 2, floor: y [rows][F/2][C]; a tie keeps the lower bin) and the
 *     Dropout2d factor keep [B][F/2] (0 or 1/(1-p); NULL = none; b = row / T).  bwd: dx, dgamma,
 *     dbeta (overwritten, deterministic) from dy, the saved x, mean, rstd.  C % 4 == 0.
 *   time_pool: max over frame pairs, y [B][T/2][D] of x [B][T][D] (floor; D % 4 == 0); bwd routes
 *     dy to the pair's maximum (a tie: the earlier frame). */
int mlvae_conv2d_supported(int Cin, int Cout);
size_t mlvae_conv2d_workspace_size(int op, int B, int T, int F, int Cin, int Cout);
int mlvae_conv2d_fwd(int B, int T, int F, int Cin, int Cout, const float* x, const float* w, const float* bias,
                     float* y, void* ws, size_t ws_bytes, void* stream);
int mlvae_conv2d_dgrad(int B, int T, int F, int Cin, int Cout, const float* dy, const float* w, float* dx,
                       void* ws, size_t ws_bytes, void* stream);
int mlvae_conv2d_wgrad(int B, int T, int F, int Cin, int Cout, const float* dy, const float* x, float* dw,
                       float* db, void* ws, size_t ws_bytes, void* stream);
/* the forward's first launch alone: xp = the reflect-padded bf16 copy [B][T+2][F+2][C] of x */
int mlvae_conv2d_pad_bf16(int B, int T, int F, int C, const float* x, void* xp, void* stream);
int mlvae_conv2d_first_fwd(int B, int T, int F, int Cout, const float* x, const float* w, const float* bias,
                           float* y, void* stream);
size_t mlvae_conv2d_first_wgrad_workspace_size(int B, int T, int F, int Cout);
int mlvae_conv2d_first_wgrad(int B, int T, int F, int Cout, const float* dy, const float* x, float* dw,
                             float* db, void* ws, size_t ws_bytes, void* stream);
int mlvae_ln_fc_act_fwd(long long rows, int T, int F, int C, const float* x, const float* gamma,
                        const float* beta, const float* keep, int pool, float eps, float* y, float* mean,
                        float* rstd, void* stream);
size_t mlvae_ln_fc_act_bwd_workspace_size(long long rows, int F, int C);
int mlvae_ln_fc_act_bwd(long long rows, int T, int F, int C, const float* dy, const float* x,
                        const float* gamma, const float* beta, const float* keep, int pool, const float* mean,
                        const float* rstd, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                        void* stream);
int mlvae_time_pool_fwd(int B, int T, int D, const float* x, float* y, void* stream);
int mlvae_time_pool_bwd(int B, int T, int D, const float* dy, const float* x, float* dx, void* stream);
/* ELBO: reparameterise + KL (ref:src/modules/vanilla_vae.py:37-45) with masked partial
 * sums; ml = [mu | log_var] rows of width 2Z (leading dim ldml). */
int mlvae_elbo_partials_count(int B, int T, int C);
int mlvae_reparam_kl_fwd(int B, int T, int Z, const float* ml, int ldml, const float* eps,
                         const float* lens, float* z, float* kl_out, float* partials,
                         void* stream);
int mlvae_reparam_kl_bwd(int B, int T, int Z, const float* ml, int ldml, const float* eps,
                         const float* lens, const int* count, const float* dz, const float* dkl,
                         float kl_scale, float* dml, int lddml, void* stream);
/* Reconstruction term (ref:src/modules/decoder.py:37-53; loss_type 0 likelihood, 1 mse)
 * with masked partial sums and, when dmux != NULL, its gradient. */
int mlvae_recon(int B, int T, int F, int loss_type, const float* mux, int ldmu, const float* lvx,
                int ldlv, const float* x, int ldx, const float* lens, const int* count,
                float* rec_out, float* partials, const float* drec, float rec_scale, float* dmux,
                float* dlvx, void* stream);
/* Fused decoder heads (bf16 mode): both FCBlock([2H, C, C, F]) heads forward, the recon loss
 * (masked partial sums into partials[mlvae_heads_partials_count(B, T)], read by
 * mlvae_elbo_finalize) and, when train, its gradient (scale rec_scale / (count * F)), both heads
 * backward and dy = d loss / d rnn_out [B*T, 2H], in one launch.  y_bf16 [B*T, 2H] bf16 rnn output;
 * w1_bf16 [2C, 2H] the two heads' stacked first-layer weights (bf16), w1t_bf16 its transpose
 * [2H, 2C] (train); b1 [2C]; w2*/w3* fp32 [C, C] / [F, C].  Outputs fp32: p1 [B*T, 2C], p2m/p2v
 * [B*T, C], mux/lvx [B*T, F]; train: dmux/dlvx (dlvx NULL for mse), dp2m/dp2v, dp1, dy.
 * mlvae_heads_supported(C, F, 2H): C == 64, F in {64, 80}, 2H % 128 == 0.  Replaces
 * ref:src/modules/decoder.py:24-25,37-53 + ref:src/modules/fc_block.py:9-16 and their autograd. */
int mlvae_heads_partials_count(int B, int T);
int mlvae_heads_supported(int C, int F, int H2);
int mlvae_heads_fused(int B, int T, int F, int C, int H2, int loss_type, int train,
                      const void* y_bf16, const void* w1_bf16, const void* w1t_bf16, const float* b1,
                      const float* w2m, const float* b2m, const float* w3m, const float* b3m,
                      const float* w2v, const float* b2v, const float* w3v, const float* b3v,
                      const float* x, const float* lens, const int* count, float rec_scale,
                      float* p1, float* p2m, float* p2v, float* mux, float* lvx, float* dmux,
                      float* dlvx, float* dp2m, float* dp2v, float* dp1, float* dy,
                      float* partials, void* stream);
/* mlvae_heads_fused plus, when bias_ws is given (train only), the five head bias gradients from
 * in-kernel column sums: per-workgroup sums into bias_ws (>= mlvae_heads_bias_workspace_size
 * bytes), then a fixed-order reduce into db3m / db3v (mean_fc / log_var_fc blocks.4.bias [F]),
 * db2m / db2v (blocks.2.bias [C]) and db1 (the stacked blocks.0 biases [2C]; mse: the log_var
 * head gets no gradient, so db3v, db2v and db1[C:] are not written).  Replaces the autograd
 * bias sums of ref:src/modules/fc_block.py:9-16 without re-reading dOUT / dP2 / dP1.
 * saved_bf16: p1, p2m/p2v, dmux/dlvx, dp2m/dp2v and dp1 are written as bf16 (packed rows, the
 * weight-gradient GEMMs' operand precision) instead of fp32; mux / lvx / dy stay fp32.
 * With bias_ws and saved_bf16 in train mode the work runs in split form: P1 and dY as 256^2
 * GEMMs (bias + LReLU + bf16 epilogue; fp32 dY) around a persistent kernel for the middle stages
 * (same outputs).  saved_bf16 bit 1 (value 3): the split form writes
 * dY as bf16 [N, 2H] (mlvae_lstm_bwd_ex3's dy_bf16 input); an error without the split form. */
size_t mlvae_heads_bias_workspace_size(int B, int T, int F, int C);
int mlvae_heads_fused_ex(int B, int T, int F, int C, int H2, int loss_type, int train,
                         const void* y_bf16, const void* w1_bf16, const void* w1t_bf16, const float* b1,
                         const float* w2m, const float* b2m, const float* w3m, const float* b3m,
                         const float* w2v, const float* b2v, const float* w3v, const float* b3v,
                         const float* x, const float* lens, const int* count, float rec_scale,
                         float* p1, float* p2m, float* p2v, float* mux, float* lvx, float* dmux,
                         float* dlvx, float* dp2m, float* dp2v, float* dp1, float* dy,
                         float* partials, float* bias_ws, size_t bias_ws_bytes, float* db3m,
                         float* db3v, float* db2m, float* db2v, float* db1, int saved_bf16,
                         void* stream);
/* mlvae_heads_fused_ex plus, when wg_ws is given, the four small weight gradients of the heads
 * (ref:src/modules/fc_block.py:9-16 blocks.2 / blocks.4 of mean_fc and log_var_fc, the products
 * autograd forms for decoder.py:24-25): dw3m / dw3v = dOUT_h^T P2_h [F, C] and dw2m / dw2v =
 * dP2_h^T P1_h [C, C], accumulated inside the heads' middle kernel over its 64-frame tiles (the
 * frame rows as K, read transposed from the LDS images it already holds), per-workgroup slabs
 * reduced in a fixed order -- replacing four split-K GEMM launches over the saved intermediates.
 * Needs the split form (train, bias_ws, saved_bf16 bit 0) and wg_ws_bytes >=
 * mlvae_heads_wgrad_workspace_size(B, T, F, C); under mse (loss_type 1) dw3v / dw2v may be NULL
 * and are not written.  P2 / dOUT / dP2 (p2m, p2v, dmux, dlvx, dp2m, dp2v) are then not written. */
size_t mlvae_heads_wgrad_workspace_size(int B, int T, int F, int C);
/* The split form's two first-layer products (P1 = LReLU(Y W1^T + b1), dY = dP1 W1) run on a
 * 128-row kernel (mode 1, the default: from 64K frames; 2: at every size; 0: on the 256² GEMM).
 * Both compute each output with the same k-order, so the modes agree bit for bit. */
int mlvae_heads_set_nt_mode(int mode);
int mlvae_heads_fused_ex2(int B, int T, int F, int C, int H2, int loss_type, int train,
                          const void* y_bf16, const void* w1_bf16, const void* w1t_bf16, const float* b1,
                          const float* w2m, const float* b2m, const float* w3m, const float* b3m,
                          const float* w2v, const float* b2v, const float* w3v, const float* b3v,
                          const float* x, const float* lens, const int* count, float rec_scale,
                          float* p1, float* p2m, float* p2v, float* mux, float* lvx, float* dmux,
                          float* dlvx, float* dp2m, float* dp2v, float* dp1, float* dy,
                          float* partials, float* bias_ws, size_t bias_ws_bytes, float* db3m,
                          float* db3v, float* db2m, float* db2v, float* db1, int saved_bf16,
                          float* wg_ws, size_t wg_ws_bytes, float* dw3m, float* dw3v, float* dw2m,
                          float* dw2v, void* stream);
/* mlvae_heads_fused_ex2 with the split-bf16 forward when w1_split is given (split form only): the
 * forward products of ref:src/modules/fc_block.py:9-16 as bf16 hi + lo operand pairs -- P1 = LReLU(Y
 * (W1_hi + W1_lo)^T + b1) on the 128-row kernel, P2 = LReLU(P1 (W2_hi + W2_lo)^T + b2) and OUT =
 * P2_hi (W3_hi + W3_lo)^T + P2_lo W3_hi^T + b3 -- so mu_x / log_var_x (and the ELBO) carry no bf16
 * rounding of the heads' weights.  w1_split = mlvae_bf16_split_rows(W1 [2C, 2H], chunk 64).  The
 * backward products stay bf16. */
int mlvae_heads_fused_ex3(int B, int T, int F, int C, int H2, int loss_type, int train,
                          const void* y_bf16, const void* w1_bf16, const void* w1t_bf16, const float* b1,
                          const float* w2m, const float* b2m, const float* w3m, const float* b3m,
                          const float* w2v, const float* b2v, const float* w3v, const float* b3v,
                          const float* x, const float* lens, const int* count, float rec_scale,
                          float* p1, float* p2m, float* p2v, float* mux, float* lvx, float* dmux,
                          float* dlvx, float* dp2m, float* dp2v, float* dp1, float* dy,
                          float* partials, float* bias_ws, size_t bias_ws_bytes, float* db3m,
                          float* db3v, float* db2m, float* db2v, float* db1, int saved_bf16,
                          float* wg_ws, size_t wg_ws_bytes, float* dw3m, float* dw3v, float* dw2m,
                          float* dw2v, const void* w1_split, void* stream);
/* dst [rows][2 cols] bf16 = src [rows][cols] fp32 as split-bf16 pairs: each chunk-wide column block
 * c becomes [hi | lo] at columns 2 c chunk .. 2 (c + 1) chunk - 1 (x = hi + lo to ~2^-17).  cols %
 * chunk == 0. */
int mlvae_bf16_split_rows(const float* src, int rows, int cols, int chunk, void* dst, void* stream);
/* Skinny products of the bottom LSTM layer (bf16; one side is the latent width):
 * mlvae_skinny_nt: C [M, N] (fp32, ldc) = A [M, K] . Bt [N, K]^T, bf16 k-contiguous operands,
 *   N in {16, 32, 48, 64}, K % 32 == 0: dZ = dG W_ih over the k-contiguous W_ih^T copy.  K == 0
 *   reads neither operand and stores C = 0; K < 0 is refused.
 * mlvae_skinny_tn: W [M, nw] (fp32 row-major) = A^T B over K frames, A stored [K, M] (lda), B
 *   stored [K, NB] (ldb), NB in {16..64} % 16, M % 64 == 0; bias1/bias2 [M] (either may be NULL)
 *   = column nw of the product (B's column nw all ones: the bias gradient as MFMA work).  B's
 *   columns beyond nw (beyond nw + 1 with a bias) are read but reach no output: they may hold
 *   any finite values.  Frame splits go to fp32 slabs (workspace:
 *   mlvae_skinny_tn_workspace_size) summed in a fixed order.
 * Replace the autograd of layer 0's input projection (ref:src/modules/decoder.py:14-15,22). */
/* C[M, N] = A[M, K] B[N, K]^T + bias1 + bias2 (bf16 operands, k-contiguous, fp32 C), K in
 * {8, 16, 24, 32}, N % 16 == 0, 16-byte aligned rows; biases may be NULL.  The layer-0 LSTM
 * input projection z W_ih^T + b_ih + b_hh (ref:src/modules/decoder.py:14-15,22), K = latent. */
int mlvae_skinny_proj(int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                      const float* bias1, const float* bias2, float* C, int ldc, void* stream);
/* The same with C fp32 (c_fp16 = 0) or IEEE fp16 (c_fp16 = 1: the wide recurrence's gates). */
int mlvae_skinny_proj_ex(int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                         const float* bias1, const float* bias2, void* C, int ldc, int c_fp16,
                         void* stream);
int mlvae_skinny_nt(int M, int N, int K, const void* A, int lda, const void* Bt, int ldb,
                    float* C, int ldc, void* stream);
size_t mlvae_skinny_tn_workspace_size(int M, int NB, int K);
int mlvae_skinny_tn(int M, int NB, int K, const void* A, int lda, const void* B, int ldb, int nw,
                    float* W, float* bias1, float* bias2, float* ws, size_t ws_bytes, void* stream);
/* fp8 mode (configs[4]), layer 0: the same two products on the e4m3 dG the fp8 BPTT writes (lda in
 * bytes, % 16) -- converted to bf16 in registers (exact), results times *alpha (1 / dG's scale).
 * mlvae_skinny_nt_fp8 needs K > 0, K % 256 == 0 and M >= 4096 (K <= 0 is refused);
 * mlvae_skinny_tn_fp8 mlvae_skinny_tn's workspace. */
int mlvae_skinny_nt_fp8(int M, int N, int K, const void* A8, int lda, const void* Bt, int ldb, float* C, int ldc,
                        const float* alpha, void* stream);
int mlvae_skinny_tn_fp8(int M, int NB, int K, const void* A8, int lda, const void* B, int ldb, int nw, float* W,
                        float* bias1, float* bias2, const float* alpha, float* ws, size_t ws_bytes, void* stream);
/* dZ = dG W_ih_l0 (as mlvae_skinny_nt) and dW_ih_l0 | b_ih = b_hh gradients = dG^T [z | 1] (as
 * mlvae_skinny_tn) from ONE pass over the layer-0 dG (ref:src/modules/decoder.py:14-15,22, the
 * autograd of nn.LSTM's layer-0 input projection): dG [M][lda] bf16 with K8 = 8H columns
 * (K8 % 256 == 0), Wt = W_ih^T [32][ldw] bf16, zb = [z | 1 | 0] [M][ldz >= 48] bf16 (Z = 32), dZ
 * [M][lddz] fp32; W [K8][32], bias1 / bias2 [K8] (optional).  Deterministic (fixed-order slab
 * reduce). */
size_t mlvae_skinny_dzw_workspace_size(int M, int K8);
int mlvae_skinny_dzw(int M, int K8, const void* A, int lda, const void* Wt, int ldw, const void* zb, int ldz, int Z,
                     float* dZ, int lddz, float* W, float* bias1, float* bias2, float* ws, size_t ws_bytes,
                     void* stream);
/* Fused VanillaVAE encoder (bf16; mlvae_encoder_supported: E == 64, Z == 32, F in {64, 80}).
 * Forward: FC(F->E) LReLU FC(E->E) LReLU -> [mu | log_var] -> z = eps exp(lv/2) + mu, with the
 * masked KL sums in kl_partials[mlvae_encoder_partials_count] (read by mlvae_elbo_finalize).
 * eps_in NULL: eps = Philox(seed, offset + n*Z + k) (the mlvae_randn stream) -> eps_out.
 * z_bf16 [B*T, z_ld]: z_ld = Z, or >= Z + 16 with columns Z..Z+15 = [1, 0, ...] (the ones column
 * of mlvae_skinny_tn's bias gradient).  e1/e2 bf16 [B*T, E] are kept for the backward.
 * Backward: from dz (the gradient reaching z) the reparam/KL gradient, both LReLU dgrads and the
 * six encoder weight/bias gradients (overwritten; fixed-order reduce over the workspace
 * mlvae_encoder_workspace_size).  Replaces ref:src/modules/vanilla_vae.py:13-45 and its autograd. */
int mlvae_encoder_supported(int F, int E, int Z);
int mlvae_encoder_partials_count(int B, int T);
size_t mlvae_encoder_workspace_size(int B, int T, int F, int E, int Z);
int mlvae_encoder_fwd(int B, int T, int F, int E, int Z, const float* x, const float* w0,
                      const float* b0, const float* w1, const float* b1, const float* wml,
                      const float* bml, const float* eps_in, unsigned long long seed,
                      unsigned long long offset, const float* lens, void* e1_bf16, void* e2_bf16,
                      float* ml, float* z, void* z_bf16, int z_ld, float* eps_out,
                      float* kl_partials, void* stream);
/* mlvae_encoder_fwd with split = 1: every forward product as a_hi W_hi + a_hi W_lo + a_lo W_hi
 * (bf16 hi + lo pairs of the fp32 x, activations and weights: mu / log_var / z / KL to ~1e-5 of
 * fp32 at the same HBM traffic; e1 / e2 are still saved bf16).  split = 0 is mlvae_encoder_fwd. */
int mlvae_encoder_fwd_ex(int B, int T, int F, int E, int Z, const float* x, const float* w0,
                         const float* b0, const float* w1, const float* b1, const float* wml,
                         const float* bml, const float* eps_in, unsigned long long seed,
                         unsigned long long offset, const float* lens, void* e1_bf16, void* e2_bf16,
                         float* ml, float* z, void* z_bf16, int z_ld, float* eps_out,
                         float* kl_partials, int split, void* stream);
int mlvae_encoder_bwd(int B, int T, int F, int E, int Z, const float* dz, const float* ml,
                      const float* eps, const void* e1_bf16, const void* e2_bf16, const float* x,
                      const float* wml, const float* w1, const float* lens, const int* count,
                      float kl_scale, float* dwml, float* dbml, float* dw1, float* db1, float* dw0,
                      float* db0, float* ws, size_t ws_bytes, void* stream);
/* Data parallel: the step's scalars in a 4-float header before the flat gradient, summed by the
 * last gradient bucket's all-reduce (one collective instead of a loss-sum and an err-max).  pack =
 * 1: hdr = [loss3 | err != 0]; pack = 0 (after the sum): loss3 = hdr[0..2], err = 1 when any rank
 * set it.  ref:src/prepare_experiment.py:12,55 (SpeechBrain run_opts data parallel), the loss
 * sync of ref:src/models/md_model.py:77-88 fit_batch. */
int mlvae_dp_scalars(int pack, float* hdr, float* loss3, int* err, void* stream);
/* out[3] = {kld_loss, recon_loss, w_kl*kld + w_rec*recon}
 * (ref:src/utils/data_utils.py:67-104, ref:src/models/md_model.py:189-213). */
int mlvae_elbo_finalize(const float* kl_partials, int nk, const float* rec_partials, int nr,
                        const float* lens, const int* count, int B, int T, int Z, int F,
                        float w_kl, float w_rec, float* out, void* stream);
/* count (optional, device int) overrides the valid-frame count derived from lens: a
 * data-parallel shard passes the all-reduced global count so that its loss/gradients are
 * its exact share of the global masked mean (SURVEY.md 8(e)(i)). */
int mlvae_count_frames(const float* lens, int B, int T, int* out, void* stream);
/* eps ~ N(0,1) from Philox-4x32-10(seed, offset + i): shard-invariant reparameterisation noise
 * (replaces torch.randn_like at ref:src/modules/vanilla_vae.py:39). */
int mlvae_randn(size_t n, unsigned long long seed, unsigned long long offset, float* out,
                void* stream);
/* apply_lens_to_loss(loss[B,T,C], lens, reduction 0 mean / 1 batchmean / 2 batch);
 * out holds 2*B floats (results first). */
int mlvae_masked_mean(int B, int T, int C, const float* loss, const float* lens, int reduction,
                      float* out, void* stream);

/* InputNormalization(norm_type='global') inside the fused step: SpeechBrain's normaliser
 * (un-vendored; parity unpinned, restated in brain/features.py), built at
 * ref:src/models/test_vanilla_vae/model.yaml:14-15 and applied at
 * ref:src/models/test_vanilla_vae/model.py:24-25.  F % 4 == 0, 16-byte aligned buffers.
 *   stats:  per-utterance mean / std over the first round(rel_len*T) frames -> utt_stats [B][2F];
 *           sums [2F+1] = the sums of those over the utterances with frames, and their count
 *           (what a data-parallel run all-reduces before the update)
 *   update: mode 0 keep, 1 set the global statistics to the batch's, 2 running average with
 *           weight w of the batch (epoch < update_until_epoch): g = w_old g + w_new cur
 *   apply:  out = (x - glob_mean) / glob_std over rows x F */
int mlvae_norm_supported(int F);
int mlvae_norm_stats(int B, int T, int F, const float* x, const float* rel_lens, float* utt_stats,
                     float* sums, float eps, void* stream);
int mlvae_norm_update(int F, const float* sums, float* glob_mean, float* glob_std, int mode,
                      float w_old, float w_new, void* stream);  /* mode 2: w_old = 1 - w, w_new = w */
int mlvae_norm_apply(size_t rows, int F, const float* x, const float* glob_mean, const float* glob_std,
                     float* out, void* stream);

/* check_gradients + Adam (ref:src/models/md_model.py:82-86, model.yaml:45-47). */
int mlvae_sumsq_partials_count(size_t n);
int mlvae_grad_sumsq(const float* grads, size_t n, double* partials, void* stream);
/* advance: 1 = single-tensor step (prologue + update + step counter); for a multi-tensor
 * step over several buffers call with 0 for the first, -1 (reuse the prologue's hyp) for the
 * middle ones and 1 for the last (which advances the device step counter). */
int mlvae_adam_step(float* params, float* exp_avg, float* exp_avg_sq, const float* grads,
                    size_t n, const double* partials, int nparts, const float* loss, int* step,
                    int* nonfinite, float lr, float beta1, float beta2, float eps,
                    float max_norm, float* norm_out, float* hyp_scratch, int advance,
                    void* stream);
/* As mlvae_adam_step, plus the persistent recurrences' hand-off timeout word `err` (optional):
 * while *err != 0 the update is skipped (parameters and Adam state untouched, step counter not
 * advanced) and *err_skips (optional) counts the skipped steps, apart from non-finite losses. */
int mlvae_adam_step_ex(float* params, float* exp_avg, float* exp_avg_sq, const float* grads,
                       size_t n, const double* partials, int nparts, const float* loss, int* step,
                       int* nonfinite, const int* err, int* err_skips, float lr, float beta1,
                       float beta2, float eps, float max_norm, float* norm_out, float* hyp_scratch,
                       int advance, void* stream);

/* clip_grad_norm_ over several separately stored grads: every grad's sum-of-squares
 * partials go to one buffer (offsets), then each grad is scaled by min(max/(total+1e-6),1). */
int mlvae_clip_scale(float* grads, size_t n, const double* partials, int nparts, float max_norm,
                     float* norm_out, void* stream);

/* module-level autograd helpers: dx = dy * lrelu'(y); d apply_lens_to_loss / d loss */
int mlvae_lrelu_bwd(size_t n, const float* dy, const float* y, float* dx, void* stream);
int mlvae_masked_mean_bwd(int B, int T, int C, const float* lens, int reduction, const float* g,
                          float* dloss, void* stream);

/* bias gradients: out[c] = beta*out[c] + sum_n in[n][c]; out2 (optional) gets a copy. */
size_t mlvae_colsum_workspace_size(int N, int C);
int mlvae_colsum(int N, int C, const float* in, int ld, float* out, float* out2, float beta,
                 float* ws, size_t ws_bytes, void* stream);
/* the same over an fp32 (in_bf16 = 0) or bf16 (in_bf16 = 1) input */
int mlvae_colsum_ex(int N, int C, const void* in, int in_bf16, int ld, float* out, float* out2,
                    float beta, float* ws, size_t ws_bytes, void* stream);

/* y = x * mask; mask = given (already scaled) or Philox(seed, i) keep-prob 1-p scaled 1/(1-p).
 * Inter-layer dropout of nn.LSTM in train mode (ref:src/modules/decoder.py:14). */
int mlvae_dropout(size_t n, const float* x, float* y, const float* mask,
                  unsigned long long seed, float p, void* stream);
/* the same writing y (fp32, may be NULL) and/or y_bf16 (bf16, may be NULL); element i takes the
 * mask of index offset + i (offset a multiple of 4): a data-parallel shard passes the global
 * index of its first element, so every rank count draws the single-GPU run's masks */
int mlvae_dropout_ex(size_t n, const float* x, float* y, void* y_bf16, const float* mask,
                     unsigned long long seed, unsigned long long offset, float p, void* stream);

/* GMM-VAE latent block (SURVEY 8(f) rank 1; replaces ref:src/modules/gmm_vae.py:24-67).
 * P = the five heads as one stacked GEMM output, rows of width >= 4*N*Z + N:
 * [prior_mean | prior_log_var | mean | log_var] (N*Z each), then the N gmm logits.
 * Forward: z = eps*exp(lv/2) + mean; kl = -0.5(1 + lv - plv - (e^lv + (m-pm)^2)/(e^plv + 1e-5));
 * w = hard Gumbel-softmax(logits, tau) (straight-through value), ysoft = its soft sample.
 * expo = the Exp(1) draws [rows, N] or NULL: Philox(seed, offset + r*N + n) (ref :31).
 * Backward: dP from dz, dkl, dw (each NULL = 0); logits get the straight-through gradient. */
int mlvae_gmm_latent_fwd(int rows, int N, int Z, const float* P, int ldp, const float* eps,
                         const float* expo, unsigned long long seed, unsigned long long offset,
                         float tau, float* z, float* kl, float* w, float* ysoft, void* stream);
int mlvae_gmm_latent_bwd(int rows, int N, int Z, const float* P, int ldp, const float* eps,
                         const float* ysoft, float tau, const float* dz, const float* dkl,
                         const float* dw, float* dP, int lddp, void* stream);
/* apply_weight (ref:src/utils/data_utils.py:32-64): y[r,c] = sum_n w[r,n] x[r, n*C + c];
 * backward dx[r, n*C + c] = w[r,n] dy[r,c] and dw[r,n] = sum_c dy[r,c] x[r, n*C + c]
 * (dx or dw may be NULL). */
int mlvae_apply_weight_fwd(int rows, int N, int C, const float* x, int ldx, const float* w,
                           float* y, int ldy, void* stream);
int mlvae_apply_weight_bwd(int rows, int N, int C, const float* x, int ldx, const float* w,
                           const float* dy, int lddy, float* dx, int lddx, float* dw,
                           void* stream);

/* The Hierarchical VAE's latent stretch in one launch (csrc/hvae.hip; replaces, for the recipes that
 * ask for it, mlvae_reparam_kl_fwd + mlvae_gmm_latent_fwd + the eight mlvae_apply_weight_fwd calls
 * of ref:src/modules/h_vae.py:21-72, and their backwards).  fp32.
 *   ml [rows, ldml] = [mean_v | log_var_v] (ldml >= 2Z), P [rows, ldp] as mlvae_gmm_latent_fwd's,
 *   pi [rows, 2], eps_v [rows, Z], eps_g [rows, N*Z], expo [rows, N] or NULL: Philox(seed,
 *   offset + r*N + n), the draws of mlvae_gmm_latent_fwd.
 * Forward: v = (mean_v, log_var_v, eps_v e^{lv_v/2} + mean_v, KL_v) (mlvae_reparam_kl_fwd's),
 *   g[n] = (m[n], lv[n], z[n], kl[n]) and w, ysoft as mlvae_gmm_latent_fwd's (w bit for bit),
 *   G = sum_n w[n] g[n] (n ascending), (mean, log_var, h, kl) [rows, Z] = pi0 v + pi1 G.
 *   ml == NULL && pi == NULL: the GMM-only mode, h = G_z and kl = G_kl; mean, log_var, eps_v unread.
 * Backward: recomputes v and g from the saved inputs, w and ysoft; cotangents d_mean, d_log_var,
 *   d_h, d_kl [rows, Z] and d_w [rows, N], each NULL = 0 (the GMM-only mode ignores d_mean and
 *   d_log_var); writes dml [rows, 2Z], the 4NZ + N columns of dP [rows, lddp] and dpi [rows, 2]
 *   (dpi may be NULL; dml and dpi are unwritten in the GMM-only mode).  The weight cotangent
 *   d_w[n] + pi1 sum_key sum_c d_key[c] g_key[n,c] reaches the logits through ysoft (straight-
 *   through).  Sums over c are fixed-order reductions inside a wave: a rerun is bit-identical.
 * Any Z >= 1, 1 <= N <= 64, any rows >= 0 (0: a no-op).  Status 1 before any launch: N out of
 * range, ldp (lddp) < 4NZ + N, ldml < 2Z, exactly one of ml / pi NULL, a required pointer NULL.
 * mlvae_hvae_latent_fwd_rows: the forward over the rows = B T frames of a data-parallel shard, map
 *   as mlvae_gmm_latent_fwd_rows' (NULL: the identity, then mlvae_hvae_latent_fwd at offset 0). */
int mlvae_hvae_latent_fwd(int rows, int N, int Z, const float* ml, int ldml, const float* P, int ldp,
                          const float* pi, const float* eps_v, const float* eps_g, const float* expo,
                          unsigned long long seed, unsigned long long offset, float tau, float* mean,
                          float* log_var, float* h, float* kl, float* w, float* ysoft, void* stream);
int mlvae_hvae_latent_fwd_rows(int B, int T, int N, int Z, const float* ml, int ldml, const float* P,
                               int ldp, const float* pi, const float* eps_v, const float* eps_g,
                               const float* expo, unsigned long long seed, const long long* map,
                               float tau, float* mean, float* log_var, float* h, float* kl, float* w,
                               float* ysoft, void* stream);
int mlvae_hvae_latent_bwd(int rows, int N, int Z, const float* ml, int ldml, const float* P, int ldp,
                          const float* pi, const float* eps_v, const float* eps_g, const float* w,
                          const float* ysoft, float tau, const float* d_mean, const float* d_log_var,
                          const float* d_h, const float* d_kl, const float* d_w, float* dml, float* dP,
                          int lddp, float* dpi, void* stream);

/* Per-utterance scoring of the upstream-module recipes (csrc/score.hip): the integer counts behind
 * phn_acc.* and boundary.*, left on the device, one workgroup per utterance -- the reference scores
 * on the host per utterance on every batch (ref:src/models/test_b_ind_classifier/model.py:53-72,
 * ref:src/utils/metric_stats/phn_acc_metric_stats.py:50-85, ref:src/utils/metric_stats/
 * boundary_metric_stats.py:58-86).  T_b = round(T feat_lens[b]) and L_b = round(L phn_lens[b]) in
 * fp32, half to even (undo_padding_tensor's rule, mlvae_phn_bce's); nothing at t >= T_b or l >= L_b
 * is read.  B == 0 or T == 0 is a no-op returning 0; a null pointer or a negative size gives
 * status 1.  Each entry zeroes its outputs on the stream first.  Every output is an integer (no
 * floating-point atomics): a rerun is bit-identical.
 * mlvae_phn_acc: logits [B,T,C] (row stride ldl, any C >= 1), flvl_tgt [B,T] and plvl_tgt [B,L]
 *   int64 (plvl_tgt may be NULL, phn_lens and boundary then too), boundary [B,T] floats.  counts[b] =
 *   (flvl_correct, T_b, plvl_correct, L_b).  flvl_correct: frames t < T_b whose argmax over the
 *   classes equals flvl_tgt[b,t] (torch.argmax: the first maximal index, a NaN is the maximum; a
 *   target outside [0, C) never matches).  plvl_correct: the flags == 1 in [0, T_b) open the
 *   segments, segment k runs to the next flag or T_b; its class sums are fp32 from 0 over the
 *   frames in increasing t; their argmax is compared with plvl_tgt[b,k].  MLVAE_ERR_SCORE_SEGMENTS in *err (the
 *   reference's two asserts): the flags are not L_b many, or the first is not at frame 0 with
 *   T_b > 0; that utterance's plvl_correct is 0.  A row with T_b == 0 and L_b == 0 (the filler of
 *   a short data-parallel slice) gives zeros and no error.  plvl_tgt == NULL: (.., .., 0, 0).
 * mlvae_boundary_topk: v, fa_boundary [B,T] floats.  k_out[b] = k_b = the entries == 1 of the whole
 *   padded row of fa_boundary; pred[b,t] int32 = 1 for the k_b largest of v[b, :T_b], 0 for the
 *   other valid frames, -1 past T_b.  Order: value descending, then index ascending; a NaN ranks
 *   above every number (torch.topk); frame i is chosen iff fewer than k_b frames precede it.  The
 *   row is ranked in LDS: T > mlvae_boundary_topk_max_frames() (12288) gives status 1.  k_b > T_b
 *   sets MLVAE_ERR_SCORE_K in *err (torch.topk raises) and the row gets no ones.
 * mlvae_boundary_score: pred [B,T] int32 (mlvae_boundary_topk's, or the decode's boundary_out),
 *   target [B,T] floats.  counts[b] = (correct, n_pred, n_target) over t < T_b: the frames with
 *   pred == 1 walked in time order against the true segments [start_s, start_{s+1}] (both ends
 *   included, the last one ends at T_b): a prediction before the segment is skipped, one inside
 *   matches and advances both, one past it advances the segment. */
int mlvae_boundary_topk_max_frames(void);
int mlvae_phn_acc(int B, int T, int C, int L, const float* logits, int ldl, const float* feat_lens,
                  const long long* flvl_tgt, const long long* plvl_tgt, const float* phn_lens,
                  const float* boundary, int* counts, int* err, void* stream);
int mlvae_boundary_topk(int B, int T, const float* v, const float* feat_lens,
                        const float* fa_boundary, int* pred, int* k_out, int* err, void* stream);
int mlvae_boundary_score(int B, int T, const int* pred, const float* target, const float* feat_lens,
                         int* counts, void* stream);

/* The sequence lattice of the HMM_DNN_ALI aligner (csrc/align.hip; ref:src/models/HMM_DNN_ALI/
 * model.py:47-91): forward-backward and Viterbi over a per-utterance left-to-right state chain.
 * pout [B,T,C] fp32 log-probabilities (row stride ld), lens / phn_lens [B] relative lengths, phns
 * [B,L] int64.  T_b = rintf(T lens[b]), L_b = rintf(L phn_lens[b]) (fp32, half to even, clamped);
 * nothing at t >= T_b or l >= L_b is read.  Phoneme p expands into spp >= 1 states with emission
 * classes p spp + j: U_b = spp L_b states.  topology 0 (HMM): nodes = states, a path starts in
 * node 0, stays or moves to the next node, ends in node U_b - 1.  topology 1 (CTC): blank, s_0,
 * blank, .., blank (2 U_b + 1 nodes), stay / next / skip over a blank between two different
 * classes, start in node 0 or 1, end in one of the last two.  A path scores the sum of its
 * emissions.  A chain may have mlvae_lattice_max_nodes() (1024) nodes, counted on the padded L:
 * beyond it, status 1.
 * *err bits (device word, OR-ed): MLVAE_ERR_ALIGN_SHORT = HMM chain infeasible (T_b < U_b, U_b = 0
 *   or T_b = 0); MLVAE_ERR_ALIGN_CLASS = a phoneme id whose state class is outside [0, C);
 *   MLVAE_ERR_ALIGN_BLANK = CTC, a target class equal to blank.  Such an utterance scores 0 with gradient 0 and alignment -1.  A CTC chain without a
 *   path is no error: score 0, gradient 0 (torch's zero_infinity).
 * mlvae_lattice_fb: score[b] = log sum over the paths of exp(path score); alpha (and, with
 *   need_beta, beta: the chain run backwards, concurrently) go to the workspace (fp32, renormalised
 *   every few frames; mlvae_lattice_workspace_size bytes), which mlvae_lattice_grad reads.
 * mlvae_lattice_grad: dpout[b,t,c] (row stride ldd) = g[b] sum_{node n of class c} gamma_t(n), gamma
 *   the posterior occupancy: the partial derivative of g . score with respect to pout (not torch's
 *   ctc_loss gradient, which folds the log-softmax in).  The nodes of a class are summed in
 *   ascending node order, no floating-point atomics: a rerun is bit-identical.  Exactly 0 for
 *   classes without a node, frames t >= T_b and utterances without a score.  Same arguments as the
 *   mlvae_lattice_fb call (need_beta = 1) that filled ws.
 * mlvae_hmm_viterbi: HMM topology.  vscore[b] = the best path's score (float64 sums of the fp32
 *   emissions, rounded once), align[b,t] int32 = its state position in [0, U_b), -1 for t >= T_b;
 *   a tie keeps "stay".  ws: mlvae_hmm_viterbi_workspace_size bytes (the backpointers).
 * mlvae_align_counts: counts[b] = (frames correct, T_b): frame t < T_b is correct iff
 *   phns[b, align[b,t] / spp] equals phns[b,k], k the first phoneme with t samples_per_frame <
 *   phn_ends[b,k] (int64 [B,L], exclusive ends in samples), the last one if there is none.
 * mlvae_center_lsm_fwd / _bwd: y = log_softmax(x - mean_t(x), dim = -1) over contiguous [B,T,C],
 *   the mean over all T rows of the padded batch (ref:src/models/HMM_DNN_ALI/model.py:43-44), and
 *   its backward from dy and y.  ws: mlvae_center_lsm_workspace_size bytes. */
int mlvae_lattice_max_nodes(void);
size_t mlvae_lattice_workspace_size(int B, int T, int L, int spp, int topology);
int mlvae_lattice_fb(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                     const long long* phns, const float* phn_lens, int spp, int topology, int blank,
                     int need_beta, float* score, void* ws, size_t ws_bytes, int* err, void* stream);
int mlvae_lattice_grad(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                       const long long* phns, const float* phn_lens, int spp, int topology, int blank,
                       const float* g, const void* ws, size_t ws_bytes, float* dpout, int ldd,
                       void* stream);
size_t mlvae_hmm_viterbi_workspace_size(int B, int T);
int mlvae_hmm_viterbi(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                      const long long* phns, const float* phn_lens, int spp, float* vscore, int* align,
                      void* ws, size_t ws_bytes, int* err, void* stream);
int mlvae_align_counts(int B, int T, int L, const int* align, const float* lens, const long long* phns,
                       const float* phn_lens, int spp, const long long* phn_ends,
                       long long samples_per_frame, int* counts, void* stream);
size_t mlvae_center_lsm_workspace_size(int B, int C);
int mlvae_center_lsm_fwd(int B, int T, int C, const float* x, float* y, void* ws, size_t ws_bytes,
                         void* stream);
int mlvae_center_lsm_bwd(int B, int T, int C, const float* dy, const float* y, float* dx, void* ws,
                         size_t ws_bytes, void* stream);

/* The CTC evaluation kernels of the CRDNN_CTC recipes (csrc/ctc_eval.hip; ref:src/models/CRDNN_CTC/
 * model.py:60-176).  One wave per utterance; integers, or float64 sums of the fp32 emissions in
 * frame order; no atomics but the OR into *err: a rerun is bit-identical and tests/ctc_np.py
 * reproduces every output bit for bit.  Lengths as the lattice's: T_b = rintf(T lens[b]) and so on.
 * mlvae_ctc_greedy_decode: per frame t < T_b the argmax over the C classes of pout [B,T,C] (row
 *   stride ld; a tie keeps the lowest class); frame t is kept iff its class is not blank and differs
 *   from frame t - 1's.  pred [B,T] int32 = the kept classes in frame order, -1 behind them;
 *   pred_len [B] int32.
 * mlvae_edit_align: refs [B,2,L] int64 (the pronounced and the canonical phonemes), ref_lens [B,2]
 *   relative lengths, hypothesis pred[b, :pred_len[b]] (row stride Tp).  Levenshtein with unit costs;
 *   at cell (i, j) the diagonal only if its cost is strictly below both others, else the deletion
 *   (from (i - 1, j)) if strictly below the insertion, else the insertion; row 0 is insertions,
 *   column 0 deletions; the backtrace starts at (L_a, L_b).  ali [B,2,L] int32 = the hypothesis token
 *   aligned to every reference position, -1 for a deletion and past L_a (insertions are dropped);
 *   ops [B,2,4] int32 = (insertions, deletions, substitutions, L_a).  ws:
 *   mlvae_edit_align_workspace_size(B, L, Tp) bytes (two bits per cell).  L above
 *   mlvae_edit_align_max_ref() (1024): status 1.
 * mlvae_ctc_md_counts: counts [B,8] int32 over the alignment to the pronounced sequence, with
 *   pred_md = (ali != canonical) (a deletion counts as mispronounced) and gt_md = (pronounced !=
 *   canonical): (both correct, both mispronounced, missed, false alarm, canonical positions, of
 *   them recognised wrongly, mispronounced positions, of them recognised wrongly).  *err bit MLVAE_ERR_CTC_PAIR:
 *   the two references of an utterance differ in length (the shorter is counted).
 * mlvae_ctc_viterbi: the best path of the CTC chain over phns [B,L] (blank, p_0, blank, .., blank;
 *   stay / next / skip over a blank between two different classes; start in node 0 or 1, end in one
 *   of the last two).  float64 delta; a tie keeps stay, then next, then skip; of the two end nodes a
 *   tie keeps the final blank.  vscore [B] = the path's score rounded once; boundary [B,T] int32 = 1
 *   at frame 0 and at the first frame of phoneme k = 1 .. L_b - 1 (exactly L_b ones), 0 at the other
 *   frames t < T_b, -1 past T_b.  A chain without a path (T_b too short, or T_b = 0) is no error:
 *   vscore 0, infeasible[b] = 1, ones at frames 0 .. min(L_b, T_b) - 1.  *err bits MLVAE_ERR_ALIGN_CLASS / _BLANK as the
 *   lattice's (then vscore 0, boundary -1, infeasible 0).  2 L + 1 above 1024 nodes: status 1.  ws:
 *   mlvae_ctc_viterbi_workspace_size(B, T) bytes (two backpointer bits per node and frame).
 * mlvae_log_softmax_fwd / _bwd: y = log_softmax(x) over the C columns of `rows` contiguous rows, and
 *   dx = dy - exp(y) sum_c dy. */
int mlvae_ctc_greedy_decode(int B, int T, int C, const float* pout, int ld, const float* lens, int blank,
                            int* pred, int* pred_len, void* stream);
int mlvae_edit_align_max_ref(void);
size_t mlvae_edit_align_workspace_size(int B, int L, int Tp);
int mlvae_edit_align(int B, int L, int Tp, const long long* refs, const float* ref_lens, const int* pred,
                     const int* pred_len, int* ali, int* ops, void* ws, size_t ws_bytes, void* stream);
int mlvae_ctc_md_counts(int B, int L, const long long* refs, const float* ref_lens, const int* ali,
                        int* counts, int* err, void* stream);
size_t mlvae_ctc_viterbi_workspace_size(int B, int T);
int mlvae_ctc_viterbi(int B, int T, int C, int L, const float* pout, int ld, const float* lens,
                      const long long* phns, const float* phn_lens, int blank, float* vscore,
                      int* boundary, int* infeasible, void* ws, size_t ws_bytes, int* err, void* stream);
int mlvae_log_softmax_fwd(int rows, int C, const float* x, float* y, void* stream);
int mlvae_log_softmax_bwd(int rows, int C, const float* dy, const float* y, float* dx, void* stream);

/* The feature front end (csrc/fbank.hip): waveform -> log-mel filterbank, deltas, delta-deltas, the
 * reference's compute_features = speechbrain.lobes.features.Fbank(deltas=True, context=False)
 * (ref:src/config/run.yaml:39-44, applied per utterance at ref:src/utils/data_io.py:187-214),
 * restated from SpeechBrain 0.5 (parity unpinned; the pin is tests/fbank_ref.py in float64).
 * wav [B, Nmax] fp32 (row stride ld), n_samples [B] int32 on the device (clamped to [0, Nmax]);
 * hop, win, n_fft in samples.  Per utterance: T_b = 1 + N_b / hop frames; frame t covers samples
 * [t hop - n_fft/2, t hop + n_fft/2), zero outside [0, N_b) (nothing at or past N_b is read: the
 * padding may hold anything); periodic Hamming window of win points centred in n_fft; |X_k|^2 for
 * k = 0 .. n_fft/2; n_mels triangular filters on the HTK mel scale over [f_min, f_max];
 * 10 log10(max(mel, 1e-10)) clamped from below at (the utterance's own maximum) - 80;
 * delta_t = sum_{k=-2..2} k x_{clamp(t+k, 0, T_b-1)} / 10, applied twice.
 * out [B, Tmax, 3 n_mels] (row stride ldo, Tmax = 1 + Nmax / hop) = (static | delta | delta-delta),
 * rows t >= T_b exact zeros; frames [B] int32 = T_b.  N_b = 0 is one frame of -100 dB statics.
 * fp32 operands and accumulation (exact-f32 MFMA); no floating-point atomics and tiles are per
 * utterance: a rerun is bit-identical and an utterance's rows do not depend on the rest of the batch.
 * Limits (status 1): n_fft even and <= 512, 1 <= win <= n_fft, 1 <= n_mels <= 64, hop >= 1,
 * B <= 65535.  B == 0 is a no-op.
 * mlvae_fbank_table fills a HOST buffer of mlvae_fbank_table_size(win, n_fft, n_mels) bytes with the
 * windowed twiddles and the filter weights (computed in float64, rounded to fp32); the caller
 * uploads it once per geometry and passes the device copy as `table` (the library allocates
 * nothing).  ws: mlvae_fbank_workspace_size(B, Nmax, hop, n_mels) bytes (the unclamped dB frames
 * and one maximum per 32-frame tile).  The size functions return 0 for a geometry outside the
 * limits (mlvae_last_error says why). */
size_t mlvae_fbank_table_size(int win, int n_fft, int n_mels);
size_t mlvae_fbank_workspace_size(int B, int Nmax, int hop, int n_mels);
int mlvae_fbank_table(int sample_rate, int win, int n_fft, int n_mels, float f_min, float f_max,
                      float* host_table, size_t table_bytes);
int mlvae_fbank(int B, int Nmax, const float* wav, int ld, const int* n_samples, int hop, int win,
                int n_fft, int n_mels, const float* table, float* out, int ldo, int* frames, void* ws,
                size_t ws_bytes, void* stream);

/* The Kaldi-compatible front end (csrc/kaldi_fbank.hip): what the reference's `kaldi_feat` holds
 * (ref:src/utils/data_io_utils.py:150-206): compute-fbank-feats --window-type=hamming
 * --htk-compat=true --dither=0.0 --energy-floor=1.0 --snip-edges=false, add-deltas, and per-speaker
 * compute-cmvn-stats / apply-cmvn --norm-vars=true, restated from Kaldi's documented behaviour
 * (parity with Kaldi unpinned: no Kaldi binary is among the pinned references; the pin is
 * tests/kaldi_fbank_ref.py in float64).
 * wav [B, Nmax] fp32 (row stride ld), n_samples [B] int32 on the device (clamped to [0, Nmax]);
 * hop and L (the window) in samples, P the power of two at or above L.  Per utterance:
 * T_b = (N_b + hop/2) / hop frames; frame f covers samples hop f + hop/2 - L/2 + i, i = 0..L-1, an
 * index outside [0, N_b) mirrored at the ends until it is inside (nothing at or past N_b is read);
 * per frame the mean is subtracted, then pre-emphasis 0.97 (w[i] -= 0.97 w[i-1], w[0] -= 0.97 w[0]),
 * the symmetric Hamming window, zero padding to P; |X_k|^2 for k = 0 .. P/2 - 1; n_mels triangular
 * filters on the 1127 ln(1 + f/700) mel scale from 20 Hz to sample_rate/2; ln(max(e, FLT_EPSILON));
 * delta_t = sum_{j=-2..2} j x_{clamp(t+j, 0, T_b-1)} / 10; delta-delta = the 9 taps
 * [4 4 1 -4 -10 -4 1 4 4] / 100 on the statics at clamped indices.
 * out [B, Tmax, 3 n_mels] (row stride ldo, Tmax = (Nmax + hop/2) / hop) = (static | delta |
 * delta-delta), or [B, Tmax, n_mels] with deltas = 0; rows t >= T_b exact zeros; frames [B] = T_b.
 * N_b < hop/2 gives no frame.  fp32 operands and accumulation (exact-f32 MFMA); no floating-point
 * atomics and tiles are per utterance: a rerun is bit-identical and an utterance's rows do not
 * depend on the rest of the batch.
 * Limits (status 1): 2 <= L <= P <= 512 with P a power of two, 1 <= n_mels <= 64, hop >= 1,
 * B <= 65535.  B == 0 is a no-op.
 * mlvae_kaldi_fbank_table fills a HOST buffer of mlvae_kaldi_fbank_table_size(L, P, n_mels) bytes
 * (float64 arithmetic, rounded to fp32); the caller uploads it once per geometry.  ws:
 * mlvae_kaldi_fbank_workspace_size(B, Nmax, hop, n_mels) bytes (the log-mel frames).  The size
 * functions return 0 for a geometry outside the limits (mlvae_last_error says why).
 *
 * Per-speaker CMVN over feats [B, T, D] fp32 (row stride ld), frames [B] and spk [B] int32 on the
 * device, stats [S, 2 D + 1] float64 on the device, owned by the caller = (sum x | sum x^2 | n).
 * mlvae_cmvn_accumulate adds the batch's valid rows into stats: one workgroup per speaker walks the
 * utterances in row order and their frames in time order (a fixed order, no floating-point
 * atomics: a rerun is bit-identical).  mlvae_cmvn_apply, in place on rows t < frames[b]:
 * mean = sum x / n, var = max(sum x^2 / n - mean^2, 1e-20), y = (x - mean) / sqrt(var); rows past
 * frames[b] are not touched.  err: a device int32 word of its own the kernels OR into: MLVAE_CMVN_ERR_SPEAKER
 * a speaker id outside [0, S) (that utterance is skipped), MLVAE_CMVN_ERR_NO_STATS (apply) a speaker with
 * n = 0 (left as it is).
 * Limits (status 1): D <= 1024, S >= 1, B <= 65535. */
size_t mlvae_kaldi_fbank_table_size(int L, int P, int n_mels);
size_t mlvae_kaldi_fbank_workspace_size(int B, int Nmax, int hop, int n_mels);
int mlvae_kaldi_fbank_table(int sample_rate, int L, int P, int n_mels, float* host_table,
                            size_t table_bytes);
int mlvae_kaldi_fbank(int B, int Nmax, const float* wav, int ld, const int* n_samples, int hop, int L,
                      int P, int n_mels, int deltas, const float* table, float* out, int ldo,
                      int* frames, void* ws, size_t ws_bytes, void* stream);
int mlvae_cmvn_accumulate(int B, int T, int D, int S, const float* feats, int ld, const int* frames,
                          const int* spk, double* stats, int* err, void* stream);
int mlvae_cmvn_apply(int B, int T, int D, int S, float* feats, int ld, const int* frames,
                     const int* spk, const double* stats, int* err, void* stream);

/* ---- The frozen wav2vec2 encoder, forward only (csrc/w2v.hip; DESIGN.md section 4, "The wav2vec2
 * encoder").  Replaces SpeechBrain's HuggingFaceWav2Vec2(freeze=True) as the reference builds it
 * (ref:src/models/w2v_MD_VAE/model.yaml:11-16) and calls it (ref:src/models/w2v_MD_VAE/model.py:24).
 * The matrix products are mlvae_gemm_bf16 / mlvae_gemm (conv layers 1-6 and the positional conv as
 * GEMMs over overlapping rows: lda < K); these are the kernels between them.  No atomics, fixed
 * reduction orders: a rerun is bit-identical.
 *
 * tensor_stats: stats[0] = mean, stats[1] = 1 / sqrt(biased var + eps) over all n elements of x
 *   (F.layer_norm(x, x.shape) of normalize_wav / output_norm): fp64 partial sums per workgroup in ws
 *   (stats_workspace_size bytes, 8-byte aligned), folded in a fixed order.
 * scale_shift: out = (x - stats[0]) stats[1], n elements (the output norm's apply pass).
 * conv0: wav [B, N] -> out [B, T0, C] channels-last (fp32, or bf16 with out_bf16):
 *   GELU(LN_C(conv(K, stride, Cin = 1)((wav - stats[0]) stats[1]) + bias)); stats NULL = the
 *   waveform as it is; w [C][K].  Limits (conv0_supported): C <= 512, K <= 10; (T0-1) stride + K <= N.
 * rows: per row of x [N, C] (fp32, leading dimension ldx)
 *     y = x + bias (bias NULL: none);  gamma != NULL: y = LN_C(y) gamma + beta (C <= 2048);
 *     (C and the leading dimensions multiples of 4, 16-byte aligned buffers)
 *     gelu: y = GELU(y) (exact erf);  res != NULL: y += res[row] (res may be out_f32: in place)
 *   written to out_f32 and / or out_bf16 (leading dimension ldo).  One kernel: the conv stack's
 *   LN + GELU, the projection's LN, both LNs of a layer, the FFN's GELU, the final LN and the
 *   positional conv's h += GELU(x + bias).
 * regroup: h [B, T, C] fp32 -> out [B, G, T + K, C / G] (fp32 or bf16), rows K/2 .. K/2 + T - 1 of
 *   each group the frames, zeros around them: a positional-conv window is then K C/G contiguous
 *   elements at frame offset t C/G.
 * attention: out [B T, H d] = softmax(scale Q K^T) V per (utterance, head), Q / K / V read in place
 *   from qkv [B T, 3 H d] (fp32, or bf16 with qkv_bf16); no mask; online softmax over streamed
 *   32-key tiles in fp32 (T is not bounded).  f32_math = 0: bf16 MFMA operands, fp32 accumulate;
 *   1: the fp32 MFMA (the parity mode).  Limits (attention_supported): d in {32, 64}, H <= 65535
 *   (and B <= 65535). */
size_t mlvae_w2v_stats_workspace_size(size_t n);
int mlvae_w2v_tensor_stats(size_t n, const float* x, float eps, float* stats, void* ws, size_t ws_bytes,
                           void* stream);
int mlvae_w2v_scale_shift(size_t n, const float* x, const float* stats, float* out, void* stream);
int mlvae_w2v_conv0_supported(int C, int K);
int mlvae_w2v_conv0(int B, int N, int T0, int C, int K, int stride, const float* wav, const float* stats,
                    const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                    void* out, int out_bf16, void* stream);
int mlvae_w2v_rows(int N, int C, const float* x, int ldx, const float* bias, const float* gamma,
                   const float* beta, float eps, int gelu, const float* res, int ldres, float* out_f32,
                   void* out_bf16, int ldo, void* stream);
int mlvae_w2v_regroup(int B, int T, int C, int G, int K, const float* h, void* out, int out_bf16,
                      void* stream);
int mlvae_w2v_attention_supported(int T, int H, int d);
int mlvae_w2v_attention(int B, int T, int H, int d, const void* qkv, int qkv_bf16, int f32_math,
                        float scale, void* out, int out_bf16, void* stream);

/* ---- The wav2vec2 encoder's backward (csrc/w2v.hip; DESIGN.md section 4, "The wav2vec2 encoder",
 * "Backward").  What fine-tuning (SpeechBrain's freeze: False with freeze_feature_extractor: True,
 * ref:src/models/w2v_LSTM_FC/model.yaml) needs above the conv stack.  The matrix products (every
 * Linear's dX and dW, the positional conv's input and weight gradients) are mlvae_gemm_bf16 /
 * mlvae_gemm, bias gradients mlvae_colsum_ex.  Stream-ordered, caller-owned buffers, no atomics, fixed
 * reduction orders: a rerun is bit-identical.
 *
 * attention_train: mlvae_w2v_attention (the same kernel, the same output bits) that also writes the
 *   per-query log-sum-exp of the scaled logits, lse [B, H, T] fp32.
 * attention_bwd: dqkv [B T, 3 H d] from qkv, dout [B T, H d] and lse; bf16 = 1: qkv, dout and dqkv are
 *   bf16, 0: fp32.  delta [B, H, T] fp32 is scratch: D = rowsum(dout o out), once per query, summed
 *   as sum_k P dP from the recomputed probabilities (with a stored bf16 `out` the row sums of dS miss
 *   zero at 2^-9 of their terms; the stored output is therefore not read).  Then two passes: a wave
 *   owns 16 queries and streams the keys (dQ), a wave owns 16 keys and streams the queries (dK, dV);
 *   P is recomputed as exp(scale S - lse).  f32_math as the forward.  dQ and dK
 *   carry `scale`; 1/sqrt(d) folded into the Q rows of a fused weight is the caller's to apply to
 *   those rows' gradients.
 * rows_bwd: the backward of mlvae_w2v_rows through y = [GELU] [LN] (x [+ bias]) (contiguous rows of C):
 *   out = [acc +] dx as fp32 and / or bf16 (acc may be out_f32: the residual stream's gradient
 *   accumulated in place).  LN (gamma != NULL): dgamma [C], dbeta [C] from per-wave partial rows in ws
 *   (rows_bwd_workspace_size bytes) folded in wave order.  x may be NULL when there is neither LN nor GELU.
 * norm_bwd: dx = stats[1] (dy - mean(dy) - xhat mean(dy xhat)) over all n elements, xhat the whole-tensor
 *   norm's OUTPUT and stats its tensor_stats; the two sums as fp64 partials per workgroup in ws
 *   (norm_bwd_workspace_size bytes, 8-byte aligned), folded in a fixed order. */
int mlvae_w2v_attention_train(int B, int T, int H, int d, const void* qkv, int qkv_bf16, int f32_math,
                              float scale, void* out, int out_bf16, float* lse, void* stream);
int mlvae_w2v_attention_bwd(int B, int T, int H, int d, const void* qkv, const void* dout, int bf16,
                            int f32_math, float scale, const float* lse, float* delta, void* dqkv, void* stream);
size_t mlvae_w2v_rows_bwd_workspace_size(int N, int C);
int mlvae_w2v_rows_bwd(int N, int C, const float* dy, const float* x, const float* bias, const float* gamma,
                       const float* beta, float eps, int gelu, const float* acc, float* out_f32,
                       void* out_bf16, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
size_t mlvae_w2v_norm_bwd_workspace_size(size_t n);
int mlvae_w2v_norm_bwd(size_t n, const float* dy, const float* xhat, const float* stats, float* dx, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- The conv stack's backward (csrc/w2v.hip; DESIGN.md section 4, "The wav2vec2 encoder", "Backward",
 * "The conv stack"): what training the feature extractor (SpeechBrain's freeze: False alone) adds.
 * Layers >= 1 are matrix products again -- the input gradient one GEMM per residue of the frame index
 * modulo the stride over overlapping rows of the guarded output gradient, the weight gradient dy^T times
 * the input's windows -- so only two kernels are new.  Stream-ordered, no atomics, fixed reduction
 * orders: a rerun is bit-identical.
 *
 * conv0_bwd: the backward of mlvae_w2v_conv0 (same arguments, same supported sizes) given dout
 *   [B, T0, C] fp32, the gradient at its output: dw [C, K], dbias / dgamma / dbeta [C].  The pre-LN
 *   activation is never stored: a wave recomputes each of its frames from the waveform, keeps its
 *   channels' sums in registers over the consecutive frames it walks and writes one partial row of
 *   (K + 3) C floats into ws (conv0_bwd_workspace_size bytes); a second kernel adds the rows in wave
 *   order (fp64).  dout is read once.  There is no input gradient.  conv0_bwd_set_max_blocks: the cap on
 *   the workgroups (default 256), returns the previous value, values < 1 only query; host-side planning
 *   state for A/B timing -- a workspace sized before a change of the cap does not fit after it.
 * pad_rows: x [B, T, C] fp32 -> out [B, pad_front + T + pad_back, C] as fp32 or bf16 with zero rows
 *   before and after every utterance (C % 4 == 0, 16-byte aligned buffers): the guard rows that keep a
 *   residue GEMM's overlapping rows inside their utterance. */
int mlvae_w2v_conv0_bwd_set_max_blocks(int blocks);
size_t mlvae_w2v_conv0_bwd_workspace_size(int B, int T0, int C, int K);
int mlvae_w2v_conv0_bwd(int B, int N, int T0, int C, int K, int stride, const float* wav, const float* stats,
                        const float* w, const float* bias, const float* gamma, const float* beta, float eps,
                        const float* dout, float* dw, float* dbias, float* dgamma, float* dbeta, void* ws,
                        size_t ws_bytes, void* stream);
int mlvae_w2v_pad_rows(int B, int T, int C, int pad_front, int pad_back, const float* x, void* out, int out_bf16,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
