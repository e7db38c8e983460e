/*
 * stabletriton_amd - C ABI of the MI355X (gfx950) operator library.
 *
 * This is the drop-in boundary for the SDXL-UNet denoise hot path: each entry
 * point is what the reference's fx leaf wrapper for the same operator would
 * bind instead of its Triton/xformers launch.  Plain pointers and sizes only;
 * every pointer is DEVICE memory unless noted; `stream` is a hipStream_t
 * passed as void*.  Launches are asynchronous on `stream`, never synchronise
 * the host and never allocate, so they are legal inside hipGraph capture
 * (reference requirement: optimizers/cuda/graphs.py:72-108 captures on a side
 * stream).  Return value: 0 = launched, non-zero = rejected before launch
 * (see st_last_error()); the Python host turns non-zero into an exception,
 * mirroring the reference's assert/RuntimeError behaviour
 * (kernels/linear.py:181-188, kernels/geglu.py:29-30).
 */
#ifndef STABLETRITON_AMD_H
#define STABLETRITON_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types of activations/weights; accumulation is always fp32.  ST_F16 (IEEE half) is the type the reference's
 * own call site computes in (implementations/Diffusers/load_sdxl_pipeline.py:17-28 passes a .half() module;
 * optimizers/replace_attention.py:91 casts q/k/v to fp16): same matrix-pipe rate as bf16, 10 mantissa bits. */
enum { ST_F32 = 0, ST_BF16 = 1, ST_F16 = 2,
       /* ST_F32S, accepted by the GEMM-shaped entry points only (st_linear, st_ln_linear, st_conv2d, st_conv1x1_cat): the
        * matrix operands x and W are "split fp32" images written by st_split_f32 (or by a producer's epilogue) - every value
        * as two IEEE halves, x ~ hi + lo * 2^-11, 4 bytes per value, row segments of 32 values = [32 hi | 32 lo] - and the
        * product runs as three 16-bit MFMAs per 32 k with fp32 accumulation (22 significant bits per operand); bias,
        * residual, row bias, statistics and y are plain fp32.  The strict (fp32-parity) mode's matrix path. */
       ST_F32S = 3 };

/* activation-tensor layouts for the image-shaped ops */
enum { ST_NCHW = 0, ST_NHWC = 1 };

/* st_linear / st_conv2d epilogue flags (bit-or) */
enum {
    ST_EPI_BIAS      = 1,   /* + bias[n]                                         */
    ST_EPI_SILU      = 2,   /* y = y * sigmoid(y)         (after bias)            */
    ST_EPI_GEGLU     = 4,   /* W has 2F rows; out[m][j] = y[j] * gelu_erf(y[F+j]) */
    ST_EPI_RESIDUAL  = 8,   /* + residual[m][n]           (after activation)      */
    ST_EPI_ROWBIAS   = 16   /* + rowbias[batch(m)][n]     (time-embedding add)    */
};

int         st_abi_version(void);          /* bumps on any signature or contract change; this header is ABI 18
                                              (6: next-weights hint passed per call, st_timestep_sincos; 7: fp8 entry points; 8: GroupNorm partials from the
                                              producer; 9: st_ln_linear_xattn; 10: ST_F16 accepted by every entry point
                                              that takes a dtype, st_ln_linear_xattn takes a dtype; 11: fp8 plan with
                                              delayed per-tensor scaling - st_linear_emit8, st_linear_fp8x, st_fp8_update_scales; 12: readers of a channel
                                              concatenation that is never written - st_group_norm_from_stats_cat, st_conv1x1_cat; 13: ST_F32S split fp32 matrix operands, st_split_f32, st_arm_split_output, st_attention_split; 14: st_attention
                                              takes head_dim 16 / 32 / 128 beside 64; 15: st_timestep_features takes the host's table of the reference's own features for integer timesteps;
                                              16: next_weights_bytes carries the geometry of a strided touch in bits 40-61;
                                              17: st_cfg_euler_step, st_cfg_step_workspace_bytes; also st_dpmpp2m_step, and then
                                              st_sde_step and st_philox_normal, and then st_lora_merge, and then
                                              st_freeu, st_freeu_workspace_bytes and st_freeu_stat_rows, and then st_attention_pag,
                                              st_pag_euler_step, st_pag_dpmpp2m_step and st_pag_sde_step, and then a DoRA and a LoHa / LoKr entry point beside
                                              st_lora_merge, added without a bump: new entry points, no existing signature or contract changed (st_attention_regions, st_attention_segments and st_attention_joint, after 18, likewise);
                                              18: st_lora_merge takes one ST_LORA_FORM_WORDS segment row, the norm pass's tables and `forms`, and is
                                              the only LoRA entry point again: the two beside it are removed) */
const char* st_last_error(void);           /* host string, thread-local     */

/* GroupNorm (+SiLU).  Replaces reference group_norm_wrapper
 * (optimizers/replace_groupnorm.py:18-19 -> kernels/groupnorm.py:128-161).
 * x,y: (N,C,H,W) logical, `layout` physical; gamma,beta: C elements of `dtype`;
 * workspace: st_group_norm_workspace_bytes() bytes of scratch.  Statistics are
 * fp32, biased variance, y = (x-mean)*rsqrt(var+eps)*gamma+beta, then
 * y*sigmoid(y) if `silu`. */
size_t st_group_norm_workspace_bytes(int N, int C, int HW, int groups);
int st_group_norm(const void* x, const void* gamma, const void* beta, void* y,
                  int N, int C, int HW, int groups, float eps, int silu,
                  int layout, int dtype, void* workspace, void* stream);

/* GroupNorm (+SiLU) of an NHWC tensor whose statistics come from its producer: `stats0` (and `stats1` for the second
 * half of a channel concatenation, unet_pt.py:352-357; else NULL / 0 / 0) are the `col_stats` buffers of the st_linear /
 * st_conv2d launches that wrote x - C0 (+ C1 = C) channels, rows0 / rows1 rows per partial.  Same arithmetic contract
 * as st_group_norm (fp32 statistics, biased variance; the partial sums are combined in double precision); the statistics
 * pass over x and its launch are gone.  workspace: st_group_norm_workspace_bytes(). */
int st_group_norm_from_stats(const void* x, const void* gamma, const void* beta, void* y, int N, int C, int HW,
                             int groups, float eps, int silu, int dtype, const float* stats0, int C0, int rows0,
                             const float* stats1, int C1, int rows1, void* workspace, void* stream);

/* The same for x = the channel concatenation [x0 | x1] of two NHWC tensors (C0 / C1 = C - C0 channels, multiples of one
 * 16-byte vector), each with the statistics of its own producer; the concatenated tensor is never written (the decoder's
 * skip connections, unet_pt.py:352-357: torch.cat -> norm1).  Bit-identical to st_group_norm_from_stats on the
 * concatenated tensor. */
int st_group_norm_from_stats_cat(const void* x0, const void* x1, const void* gamma, const void* beta, void* y, int N, int C, int HW,
                                 int groups, float eps, int silu, int dtype, const float* stats0, int C0, int rows0,
                                 const float* stats1, int C1, int rows1, void* workspace, void* stream);

/* LayerNorm over the last dimension.  Replaces layer_norm_wrapper
 * (optimizers/replace_layernorm.py:17-24 -> kernels/layer_norm.py:282-335);
 * eps is used as given (the reference's fp16 clamp to 1.6e-5 is a defect,
 * SURVEY.md section 7).  x,y: (rows, C) contiguous. */
int st_layer_norm(const void* x, const void* gamma, const void* beta, void* y,
                  int rows, int C, float eps, int dtype, void* stream);

/* GEGLU elementwise: out[m][j] = state[m][j] * gelu_erf(gate[m][j]).
 * Replaces geglu_triton (optimizers/replace_geglu.py:23-27 ->
 * kernels/geglu.py:18-35).  Row strides are in elements, so the two halves of
 * one projection output can be passed without copies. */
int st_geglu(const void* state, const void* gate, void* out, int rows, int F,
             long ld_state, long ld_gate, long ld_out, int dtype, void* stream);

/* Linear: y[M,N] = epilogue(x[M,K] * W[N,K]^T).  Replaces linear_wrapper /
 * linear_wrapper_functional (optimizers/replace_linear.py:20-34 ->
 * kernels/linear.py:173-222).  W is (N,K) row-major exactly as nn.Linear
 * stores it.  lda/ldc/ldr are row strides in elements.  With ST_EPI_GEGLU,
 * W has 2N rows and y has N columns.  rows_per_batch is only read with
 * ST_EPI_ROWBIAS (rowbias is (M/rows_per_batch, N) contiguous).
 * `workspace` (may be NULL) is caller-owned scratch of `workspace_bytes` bytes that the
 * caller ZEROES ONCE before its first use (hipMemset) and that concurrent launches must
 * not share: when present, long-K problems with few output tiles are split over K inside
 * the one launch - every K slice stores an fp32 slab there, and the block of a tile that
 * finishes last adds the slabs in slice order and applies the epilogue (bit-reproducible).
 * The first 64 KiB hold per-tile arrival counters, which every call leaves at zero again.
 * `row_stats` (may be NULL): device buffer of M * row_stats_capacity float2; when given, the
 * kernel also writes, per output row and per N tile, (sum, sum of squares) of the values it
 * stored - the LayerNorm partials st_ln_linear consumes; the number of tiles actually used is
 * returned through the HOST pointer `row_stats_chunks` (0 = none written).
 * `col_stats` (may be NULL): device buffer of col_stats_tiles * N float2; when given (with rows_per_batch = rows per
 * image), the kernel also writes, per tile row of the launch and per output column, (sum, sum of squares) of the values
 * it stored - the GroupNorm partials st_group_norm_from_stats consumes; the rows per tile row actually used come back
 * through the HOST pointer `col_stats_rows` (0 = none written: tile rows would straddle images, or the shape takes a
 * kernel that cannot emit them).
 * `next_weights` / `next_weights_bytes` (may be NULL / 0; no reference counterpart): the weight matrix the
 * GEMM-shaped launch AFTER this one will read.  This launch touches it (one dword per 128-byte line, spread
 * over its blocks, during its epilogue or from helper blocks on idle CUs) so that it waits in the memory-side
 * cache when its own GEMM starts; without it cold weights cost every GEMM an HBM round trip in its prologue.
 * The launch waits for its touches before it exits - the matrix's bytes at HBM speed -, so a caller hints small matrices whole
 * and large ones STRIDED: `next_weights_bytes` = byte count (bits 0-39) | row length in 128-byte lines << 40 (bits 40-59,
 * 0 = every line) | s << 60 (bits 60-61): the first 2^s lines of every row are touched - the K tiles the next launch's
 * prologue asks for.  The buffer must stay allocated until this launch has run (also under graph replay). */
int st_linear(const void* x, const void* W, const void* bias, const void* residual,
              const void* rowbias, void* y, int M, int N, int K,
              long lda, long ldc, long ldr, int rows_per_batch,
              int epilogue, int dtype, void* workspace, size_t workspace_bytes,
              float* row_stats, int row_stats_capacity, int* row_stats_chunks,
              float* col_stats, int col_stats_tiles, int* col_stats_rows,
              const void* next_weights, size_t next_weights_bytes, void* stream);

/* LayerNorm folded into the Linear (or GEGLU projection) that consumes it - the pair
 * layer_norm_wrapper -> linear_wrapper of the reference graph (replace_layernorm.py:17-24,
 * replace_linear.py:20-34; unet_pt.py:192-208) as ONE launch:
 *   y = rstd_m * (x W'^T - mean_m * c) + d,   W' = W * diag(gamma)  (rows of `Wg`, dtype),
 *   c[n] = sum_k W'[n][k],  d[n] = sum_k beta[k] W[n][k] + bias[n]   (fp32, host-prepared),
 * mean_m / rstd_m = LayerNorm statistics of row m of x, summed from the `row_stats`
 * partials (M x row_stats_chunks float2) the GEMM that produced x emitted (st_linear).
 * With ST_EPI_GEGLU, Wg has 2N rows and c, d 2N entries. */
int st_ln_linear(const void* x, const float* row_stats, int row_stats_chunks, const void* Wg,
                 const float* c, const float* d, void* y, int M, int N, int K, long lda,
                 long ldc, float eps, int epilogue, int dtype,
                 const void* next_weights, size_t next_weights_bytes, void* stream);

/* The query projection of the text-context attention and that attention as ONE launch - the chain
 * layer_norm_wrapper -> linear_wrapper (attn2.to_q) -> attention_wrapper of a transformer block (unet_pt.py:192-208,
 * 133-142; replace_layernorm.py:17-24, replace_linear.py:20-34, replace_attention.py:60-68):
 *   out[M, H*64] = softmax((LN(x) Wq^T + bias) k^T * scale) v   per head,
 * LayerNorm folded as in st_ln_linear (Wg, c, d, row_stats), k / v the (batch, S, H*64) context projections with token
 * strides ldk / ldv (S < 256), rows_per_batch query rows per batch entry (a multiple of 128).  The query tile never
 * leaves the chip: results are bit-identical to st_ln_linear followed by st_attention.  k / v batches are dense
 * (batch stride = S * ldk / S * ldv).  dtype: ST_BF16 or ST_F16. */
int st_ln_linear_xattn(const void* x, const float* row_stats, int row_stats_chunks, const void* Wg,
                       const float* c, const float* d, const void* k, const void* v, void* out,
                       int M, int N, int K, long lda, long ldo, float eps, int rows_per_batch, int S, int H,
                       long ldk, long ldv, float scale, int dtype,
                       const void* next_weights, size_t next_weights_bytes, void* stream);

/* Fused attention core: out = softmax(q k^T * scale) v per head, no mask.
 * Replaces attention_wrapper (optimizers/replace_attention.py:60-68); inputs
 * keep the (B, T, H*D) / (B, S, H*D) projection layout of unet_pt.py:133-142.
 * ld* are token strides in elements (>= H*D), batch strides are T*ldq etc.
 * D (head_dim) in {16, 32, 64, 128}, the reference operator's set (kernels/attention_fa2.py:118-123); 64 - every SDXL
 * head - runs on the tuned kernels, the other three on one generic kernel (csrc/attention_anyd.hip). */
int st_attention(const void* q, const void* k, const void* v, void* out,
                 int B, int T, int S, int H, int D,
                 long ldq, long ldk, long ldv, long ldo,
                 float scale, int dtype, void* stream);

/* conv2d on NHWC activations as implicit GEMM; W is (Cout, R, S, Cin)
 * contiguous (= channels_last nn.Conv2d weight).  Covers the resnet-block
 * convolutions of unet_pt.py:74-95,246-266,430,467 that the reference leaves
 * to cuDNN (optimizations.txt:5).  `upsample2x` folds a nearest 2x upsample of
 * the input into the gather (unet_pt.py:264-266).  Epilogue flags as for
 * st_linear; rowbias is (N_batch, Cout) (the time-embedding projection,
 * unet_pt.py:82-83), residual is NHWC (N,Hout,Wout,Cout).  workspace, col_stats, next_weights: as st_linear
 * (rows per image = Hout*Wout). */
int st_conv2d(const void* x, const void* W, const void* bias, const void* residual,
              const void* rowbias, void* y, int N, int Hin, int Win, int Cin,
              int Cout, int R, int S, int stride, int pad, int upsample2x,
              int epilogue, int dtype, void* workspace, size_t workspace_bytes,
              float* col_stats, int col_stats_tiles, int* col_stats_rows,
              const void* next_weights, size_t next_weights_bytes, void* stream);

/* 1x1 convolution (stride 1, no padding) of the channel concatenation [x0 | x1] (NHWC, C0 / C1 channels, multiples of a
 * K tile: 64 for 16-bit types, 32 for fp32) without the concatenated tensor: the resnet shortcut behind a skip connection
 * (unet_pt.py:352-357 -> 74-95).  W is (Cout, 1, 1, C0 + C1).  Epilogue flags BIAS / SILU / RESIDUAL; workspace, col_stats,
 * next_weights as st_conv2d.  Bit-identical to st_conv2d on the concatenated tensor. */
int st_conv1x1_cat(const void* x0, int C0, const void* x1, int C1, const void* W, const void* bias, const void* residual, void* y,
                   int N, int H, int Wd, int Cout, int epilogue, int dtype, void* workspace, size_t workspace_bytes,
                   float* col_stats, int col_stats_tiles, int* col_stats_rows,
                   const void* next_weights, size_t next_weights_bytes, void* stream);

/* Euler-discrete update of the fp32 latent and preparation of the next UNet
 * input (restated diffusers EulerDiscreteScheduler, see
 * stabletriton_amd/scheduler.py; the reference leaves this loop to the
 * third-party pipeline, implementations/Diffusers/load_sdxl_pipeline.py:39-46):
 *   i = *step;  latent += eps * dsigma[i];  next_in = latent * in_scale[i+1]
 * (cast to `dtype`).  All three tensors are elementwise-aligned (same layout),
 * n elements.  `step` lives on the device so one captured step graph can be
 * replayed down the table; st_step_advance does *step = (*step + 1) % n_steps. */
int st_euler_step(float* latent, const void* eps, void* next_in, const float* dsigma,
                  const float* in_scale, const int* step, long n, int n_steps,
                  int dtype, void* stream);
int st_step_advance(int* step, int n_steps, void* stream);

/* Classifier-free guidance fused into the Euler update (restated diffusers StableDiffusionXLPipeline.__call__ and its
 * rescale_noise_cfg, see csrc/runtime.hip; the reference leaves this to the third-party pipeline).  With i = *step:
 *   latent: batch x per_sample fp32; eps, next_in: 2*batch x per_sample in `dtype`, rows 0..B-1 the negative conditioning,
 *   rows B..2B-1 the positive one (cat([uncond, cond])); every sample one dense block (channels_last as well);
 *   e = e_neg + guidance[i] * (e_pos - e_neg);
 *   rescale != NULL: phi = rescale[i], per sample e = phi * e * std(e_pos) / std(e) + (1 - phi) * e  (std over the
 *     sample, correction 1; two launches through `workspace`, st_cfg_step_workspace_bytes(batch, per_sample) bytes,
 *     bitwise deterministic);
 *   latent += e * dsigma[i];  both halves of next_in = latent * in_scale[min(i + 1, n_steps - 1)] (cast to `dtype`).
 * guidance / rescale are device tables of n_steps floats, so new values need no new capture.  per_sample % 8 == 0,
 * latent / eps / next_in / workspace 16-byte aligned.  workspace may be NULL without a rescale table. */
size_t st_cfg_step_workspace_bytes(int batch, long per_sample);
int st_cfg_euler_step(float* latent, const void* eps, void* next_in, const float* dsigma, const float* in_scale,
                      const float* guidance, const float* rescale, const int* step, int batch, long per_sample,
                      int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* DPM-Solver++(2M) update (data prediction, second-order multistep; stabletriton_amd/scheduler.py states the arithmetic),
 * optionally with the classifier-free guidance of st_cfg_euler_step.  With i = *step and coef row i = [sigma, a, b, k]
 * (n_steps rows of 4 floats, DPMSolverTables.coefficients()):
 *   e: eps row b of sample b (guidance == NULL: eps and next_in have `batch` rows), or the guided (+ rescaled) eps of st_cfg_euler_step
 *      (guidance != NULL: eps and next_in have 2*batch rows [negative | positive]; rescale needs guidance and uses the same
 *      workspace, st_cfg_step_workspace_bytes(batch, per_sample) bytes);
 *   d = latent - sigma * e;
 *   latent = a * latent + b * ((1 + k) * d - k * history) when i != *start and k != 0, else a * latent + b * d, and then
 *     history is not read at all (the first step after a start, the last step);
 *   history = d;  next_in (both halves when guided) = latent * in_scale[min(i + 1, n_steps - 1)] (cast to `dtype`).
 * latent and history: batch x per_sample fp32, every sample one dense block (channels_last as well).  per_sample % 8 == 0;
 * latent / eps / next_in / history / workspace 16-byte aligned.  coef, in_scale, guidance, rescale are device tables, step
 * and start device ints, so a captured graph reads them by address.  No atomics: bitwise deterministic. */
int st_dpmpp2m_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                    const float* guidance, const float* rescale, const int* step, const int* start, int batch, long per_sample,
                    int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Counter-based Gaussian noise (Philox4x32-10 + Box-Muller; stabletriton_amd/rng.py states the stream and restates it in
 * float64): out[b][j] = the stream of seed seeds[b] at counter word `counter`, element j, for j < per_sample (memory order,
 * one dense block per sample).  A pure function of (seed, counter, j): nothing is stored or advanced, so a captured graph
 * replays the same values.  seeds: a device table of `batch` 64-bit seeds; out 16-byte aligned; per_sample % 4 == 0 and at
 * most 4 * 2^32.  This project's own stream: it does not reproduce torch's generator. */
int st_philox_normal(float* out, const unsigned long long* seeds, int batch, long per_sample, unsigned counter, void* stream);

/* Stochastic update: Euler ancestral and DPM++ 2M SDE in one row form (stabletriton_amd/scheduler.py, SDETables).  The
 * arguments of st_dpmpp2m_step plus `seeds` (a device table of `batch` 64-bit seeds, one per latent sample, also when
 * guided), and coef rows of 5 floats [sigma, a, b, k, c] (SDETables.coefficients()).  With i = *step:
 *   e, d, latent and history exactly as st_dpmpp2m_step (first order when i == *start or k == 0: history unread);
 *   then, only when c != 0, latent += c * z with z the st_philox_normal stream of seeds[b] at counter word i + 1;
 *   next_in (both halves when guided) = latent * in_scale[min(i + 1, n_steps - 1)] (cast to `dtype`).
 * A row with c == 0 (the last step; eta = 0) draws nothing and gives st_dpmpp2m_step's bits.  per_sample % 8 == 0 and at
 * most 4 * 2^32; latent / eps / next_in / history / workspace 16-byte aligned.  No atomics: bitwise deterministic. */
int st_sde_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                const float* guidance, const float* rescale, const int* step, const int* start, const unsigned long long* seeds,
                int batch, long per_sample, int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* LoRA merge: one grouped launch rebuilds every adapted weight from its base snapshot (stabletriton_amd/lora.py owns the
 * tables).  For every target t, elementwise over its row-major (N_t, K_t) weight of `dtype`, fp32 throughout, written in
 * place (W keeps its address), with s_j = scales[slot_j] and acc_j segment j's fp32 delta:
 *   W_t[n][k] = round( (1 + sum_j (g_j[n] - 1)) fp32(Base_t[n][k]) + sum_j g_j[n] s_j acc_j[n][k] )
 *   V_j = fp32(Base_t) + s_j acc_j,   g_j[n] = m_j[n] / ||V_j[n, :]||_2  for a segment with a magnitude m_j (DoRA), else g_j = 1,
 * which is Base + sum_j (g_j (.) V_j - Base): PEFT's DoRA, the scale inside the norm, each adapter normalised against the
 * base alone; without any magnitude it is round( fp32(Base) + sum_j s_j acc_j ).  A segment's kind only decides how acc_j is formed:
 *   ST_LORA_KIND_PLAIN  acc[n][k] = sum_r Up[n][r] DownT[k][r]
 *   ST_LORA_KIND_HADA   acc[n][k] = (sum_r Up1[n][r] DownT1[k][r]) * (sum_r Up2[n][r] DownT2[k][r])      LoHa: one fp32 product of the two sums
 *   ST_LORA_KIND_KRON   acc[n][k] = W1[n / c][j] * W2[n % c][col],  LoKr: W1 (a, b) and W2 (c, d * taps) row-major FP32 tables for
 *                       every `dtype`, 16-byte aligned, a * c = N and b * d * taps = K.  layout 1 (a channels_last conv weight,
 *                       K runs tap-major): k = tap * (b d) + j * d + q, col = tap * d + q.  layout 0 (a contiguous conv weight
 *                       or a Linear, taps = 1): k = (j * d + q) * taps + tap, col = q * taps + tap.  Any scalar (alpha / rank)
 *                       is folded into W1 by the caller.  (Tucker cores are contracted by the caller.)
 * All tables are on the device:
 *   targets:    n_targets rows of 6 int64  [W, Base, N, K, first segment, segments]   (Base never aliases W);
 *   segments:   n_segments rows of ST_LORA_FORM_WORDS int64
 *                 [kind, scale slot, magnitude or 0, workspace offset,  Up1, DownT1, rp1,  Up2, DownT2, rp2,  0, 0]     PLAIN (pair 2 unused, 0) / HADA
 *                 [kind, scale slot, magnitude or 0, workspace offset,  W1, W2,  a, b, c, d, taps, layout]              KRON
 *               Up is (N, rp) and DownT - the down factor TRANSPOSED - (K, rp), both row-major in `dtype`, 16-byte aligned, the
 *               ranks zero-padded to rp, a multiple of 32 (16-bit dtypes: one MFMA k) or of 4 (ST_F32), at most
 *               ST_LORA_MAX_RANK; alpha / rank is folded into Up by the caller.  magnitude is the device address of N fp32
 *               values; the offset (in floats) is where the segment's N * ceil(K / ST_LORA_TILE_K) partial sums of squares
 *               live in `workspace` (unused without a magnitude);
 *   max_rank:   the largest rp of any factor pair in the table (it sizes the kernel's LDS images; a larger segment is
 *               skipped); 0 when nothing is staged: no segment, or every segment is KRON;
 *   tiles:      n_tiles rows of 2 int32 [target, tile]: one workgroup each, tile = row_tile * ceil(K / ST_LORA_TILE_K) +
 *               column_tile over ST_LORA_TILE_N x ST_LORA_TILE_K tiles; a target is rebuilt where its tiles are listed;
 *   norm_tiles: n_norm_tiles rows of [target, tile] listing EVERY tile of every target that has a segment with a magnitude (a
 *               subset of `tiles`; empty, and then NULL is fine, when there is none);
 *   scales:     n_scales floats, one slot per loaded adapter: changing a scale is a copy into this table and one launch;
 *   workspace:  fp32, at least the largest offset + its segment's size (NULL / 0 with n_norm_tiles == 0);
 *   forms:      non-zero when some segment's kind is not PLAIN.  It selects the kernels that can form every kind; they hold
 *               more registers, so a table of PLAIN segments should state 0.  With 0 a segment of another kind is SKIPPED
 *               (never read as a factor pair).  Either value gives a PLAIN table the same bits.
 * One launch on `stream`, or two when n_norm_tiles > 0: the norm pass writes, per segment with a magnitude and a non-zero
 * scale, each row's sum of squares of V over one K-tile (V from the unrounded fp32 product); the merge pass adds a row's
 * partials in a fixed order.  A segment whose scale is 0 is skipped whole, magnitude included, and a weight with no non-zero
 * scale (or no segment) receives its base's bits.  A row of V_j whose sum of squares is exactly 0 takes g_j[n] = 0 (its g V
 * is the zero it was; no inf or NaN is produced).  A HADA segment stages its two pairs one after the other through the same
 * LDS images.  16-byte accesses where K is a multiple of 16 bytes of elements and W / Base are 16-byte aligned, elementwise
 * otherwise; N and K need not be tile multiples.  No atomics, nothing split over the rank, a fixed order per element:
 * bitwise deterministic.  The tables' contents are the caller's contract (they cannot be checked from the host). */
enum { ST_LORA_TILE_N = 64, ST_LORA_TILE_K = 128, ST_LORA_MAX_RANK = 128 };
enum { ST_LORA_KIND_PLAIN = 0, ST_LORA_KIND_HADA = 1, ST_LORA_KIND_KRON = 2, ST_LORA_FORM_WORDS = 12 };
int st_lora_merge(const long long* targets, int n_targets, const long long* segments, int n_segments, int max_rank,
                  const int* tiles, long n_tiles, const int* norm_tiles, long n_norm_tiles, const float* scales, int n_scales,
                  float* workspace, size_t workspace_bytes, int dtype, int forms, void* stream);

/* Sinusoidal timestep features (unet_pt.py:17-36; target of the reference's
 * fuse_timesteps pass, optimizers/replace_timesteps.py:33-58):
 *   out[b][j] = cos(t_b * f_j), out[b][dim/2 + j] = sin(t_b * f_j),
 *   f_j = exp(-ln(1e4) * j / (dim/2)),  t_b = t[(step ? *step : 0) + b*t_stride].
 * t is fp32 on the device; out is (batch, dim) of `dtype`.
 * `table` (optional, device, fp32, table_rows x dim): row i = the features of t = i as the REFERENCE's eager path computes
 * them (the host fills it with the reference's own op sequence).  The function is ill-conditioned - t_b * f_j reaches 1e3 rad,
 * so one ulp of exp() moves a feature by 1.2e-4 and two correct fp32 implementations disagree by that much; a timestep that
 * is an integer in [0, table_rows) (every entry of SDXL's schedules, every size / crop of time_ids) therefore takes its row,
 * anything else is computed.  NULL: always computed. */
int st_timestep_features(const float* t, long t_stride, const int* step, void* out,
                         int batch, int dim, int dtype, const float* table, int table_rows, void* stream);

/* ---- fp8 projection path (BASELINE config #5).  Seed in the reference: fp8-stored projection
 * weights, up-converted before the product (kernels/attention_proj.py:36-39, 105-155); here both operands stay OCP
 * e4m3 ("e4m3fn") down to the matrix pipe - the block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 at twice the bf16 rate, its
 * E8M0 block scales all 2^0 (the scales of this path are per row / per output channel, applied in the epilogue) -
 * accumulation fp32, output bf16.
 *
 * st_quantize_fp8: x (rows, C) of `dtype` (any of the three), row stride ldx elements -> xq (rows, C) e4m3 bytes, contiguous, and
 *   row_scale[m] = max_k |x[m][k]| / 448 (fp32), xq[m][k] = e4m3(x[m][k] / row_scale[m]), round to nearest even.
 * st_layer_norm_quantize_fp8: the same on LayerNorm(x) (the layer_norm_wrapper -> linear_wrapper pair of the
 *   transformer blocks as one pass over x); x (rows, C) contiguous.
 * st_linear_fp8: y[M,N] = epilogue((xq Wq^T) * row_scale[m] * w_scale[n]); Wq is (N, K) e4m3 bytes (2N rows and 2N
 *   scales with ST_EPI_GEGLU), K a multiple of 128, bias / residual / y bf16.  workspace, next_weights: as st_linear. */
int st_quantize_fp8(const void* x, long ldx, void* xq, float* row_scale, int rows, int C, int dtype, void* stream);
int st_layer_norm_quantize_fp8(const void* x, const void* gamma, const void* beta, void* xq, float* row_scale,
                               int rows, int C, float eps, int dtype, void* stream);
int st_linear_fp8(const void* xq, const float* row_scale, const void* Wq, const float* w_scale, const void* bias,
                  const void* residual, void* y, int M, int N, int K, long lda, long ldc, long ldr, int epilogue,
                  void* workspace, size_t workspace_bytes, const void* next_weights, size_t next_weights_bytes,
                  void* stream);

/* ---- fp8 plan of the compiled graph (optimizers/plan_fp8.py): the three big projections of a transformer block (q|k|v, the
 * GEGLU projection, the feed-forward output) run with e4m3 operands and NO quantisation launches.  The launch that produces a
 * projection's input also writes an e4m3 copy of it, scaled by a PER-TENSOR factor derived from the previous denoise step's
 * max |value| ("delayed scaling"); this step's maximum goes to the tensor's `amax` partial slots (256 unsigned ints holding
 * non-negative float bit patterns, combined by atomic max).  st_fp8_update_scales runs once per step before the first launch:
 * for tensor i, scale[i] = margin * max(amax_parts[i][0..255]) / 448, inv_scale[i] = 1 / scale[i], partials cleared; a tensor
 * whose partials are all zero keeps its scale.
 *
 * st_linear_emit8: st_linear whose epilogue also writes q8[m][n] = e4m3(clamp(y[m][n] * *q8_inv_scale, +-448)) (row stride ldq8
 *   bytes, N and ldq8 multiples of 8) and this launch's max |y| to q8_amax.  16-bit dtypes.
 * st_linear_fp8x: y[M,N] = epilogue((xq Wq^T) * a_scale[m * a_scale_stride] * w_scale[n]) - a_scale_stride 0: one scale for the
 *   whole activation tensor (the scale[i] above), 1: per row (st_quantize_fp8's row_scale).  With ln_c / ln_d / ln_stats the
 *   LayerNorm in front of the projection is folded exactly as in st_ln_linear (xq is then the e4m3 copy of the UN-normalised
 *   input, c[n] = sum_k of the dequantised folded weights).  `y` may be NULL, with ST_EPI_GEGLU only, when just the e4m3 copy q8 of the
 *   output is wanted (the GEGLU projection feeding the feed-forward output projection).  row_stats as in st_linear. */
int st_linear_emit8(const void* x, const void* W, const void* bias, const void* residual,
                    const void* rowbias, void* y, int M, int N, int K,
                    long lda, long ldc, long ldr, int rows_per_batch,
                    int epilogue, int dtype, void* workspace, size_t workspace_bytes,
                    float* row_stats, int row_stats_capacity, int* row_stats_chunks,
                    float* col_stats, int col_stats_tiles, int* col_stats_rows,
                    void* q8, long ldq8, const float* q8_inv_scale, unsigned int* q8_amax,
                    const void* next_weights, size_t next_weights_bytes, void* stream);
int st_linear_fp8x(const void* xq, const float* a_scale, int a_scale_stride, const void* Wq, const float* w_scale,
                   const void* bias, const void* residual, void* y, int M, int N, int K, long lda, long ldc, long ldr, int epilogue,
                   const float* ln_stats, int ln_chunks, const float* ln_c, const float* ln_d, float ln_eps,
                   float* row_stats, int row_stats_capacity, int* row_stats_chunks,
                   void* q8, long ldq8, const float* q8_inv_scale, unsigned int* q8_amax,
                   void* workspace, size_t workspace_bytes, const void* next_weights, size_t next_weights_bytes, void* stream);
int st_fp8_update_scales(float* scale, float* inv_scale, unsigned int* amax_parts, int n_tensors, float margin, void* stream);

/* Split fp32 images (ST_F32S above; the matrix operands of the strict mode): x (rows, K) fp32, row stride ldx elements ->
 * xs (rows, K) contiguous, 4 bytes per value: per row and per group of 32 consecutive k one 128-byte segment, bytes [0, 64)
 * hi[k] = f16(x[k]), bytes [64, 128) lo[k] = f16((x[k] - hi[k]) * 2048).  K % 32 == 0.  No reference counterpart: the
 * reference's strict path is torch eager fp32 (optimizers/unet_pt.py:469-542). */
int st_split_f32(const float* x, void* xs, long rows, int K, long ldx, void* stream);
/* Split image from the PRODUCER: arms the next launch on the calling thread - one of st_linear, st_ln_linear, st_conv2d,
 * st_conv1x1_cat, st_group_norm, st_group_norm_from_stats[_cat], st_attention with fp32 outputs (ST_F32 / ST_F32S) - to
 * write, beside its output y of (rows, cols) values (cols % 32 == 0; rows = M, pixels or (batch, token)), the split image
 * of y to ys (rows * cols * 4 bytes), which a following GEMM-shaped launch takes as its ST_F32S operand: no st_split_f32
 * launch, no second read of y.  That launch disarms it.  An armed launch that cannot emit (16-bit element type, other
 * shape) is rejected.  ys == NULL disarms: a caller whose armed launch failed its own argument checks (which run before the arm
 * is looked at) disarms before it frees the image, so that no later launch can write to it.  Thread-local, like st_last_error(). */
int st_arm_split_output(void* ys, long rows, int cols);
/* st_attention (ST_F32) whose K and V the producer left as split images: ks / vs point at row 0, first column of head 0, of the
 * image(s) (rows = B * S), k_cols / v_cols = values per image row (the fused q|k|v projection's image has 3 * H * D);
 * q (B, T, ldq) and out (B, T, ldo) plain fp32.  Same results as st_attention, which splits K / V tiles itself. */
int st_attention_split(const void* q, const void* ks, const void* vs, void* out, int B, int T, int S, int H, int D,
                       long ldq, long k_cols, long v_cols, long ldo, float scale, void* stream);

/* The reference's own timestep operator, elementwise (optimizers/replace_timesteps.py:33-40 ->
 * kernels/timestep.py:13-45): x is fp32 of shape (..., half), n elements in all;
 *   sin_out[i] = sin(x[i] * f_j), cos_out[i] = cos(x[i] * f_j), j = i % half, f_j = exp(-ln(1e4) * j / half). */
int st_timestep_sincos(const float* x, float* sin_out, float* cos_out, long n, int half, void* stream);

/* FreeU at one decoder skip connection (csrc/freeu.hip; no reference counterpart: diffusers' enable_freeu / ComfyUI's FreeU nodes).
 * h (N, H, W, C_h) is the running activation, skip (N, H, W, C_skip) the encoder tensor it is concatenated with; NHWC, dense,
 * 16-byte aligned, channel counts multiples of 16 bytes, H and W >= 2.  params is a DEVICE row of five floats
 * (b1, s1, b2, s2, version), read when the kernels run: slot 0 takes (b1, s1), slot 1 (b2, s2).  Out of place:
 *   skip_out = skip with its four lowest spatial frequencies (bins {0, -1} x {0, -1}) scaled by s - the published
 *              fourier_filter(threshold = 1) - as a rank-7 update from seven moments per plane, no FFT;
 *   h_out    = h with channels [0, C_h / 2) times b (version 1) or times (b - 1) * mu_hat + 1 (version 2: mu = mean over all
 *              channels, mu_hat = (mu - min) / (max - min) over the sample's H x W map, 0 where the map is constant).
 * fp32 arithmetic, one rounding on output; s == 1 / b == 1 copy the bits.  Two launches, no atomics, fixed summation order.
 * stat_rows = st_freeu_stat_rows(H * W) > 0: the apply launch also writes the GroupNorm partials of both outputs,
 * (N * H * W / stat_rows, C, 2) floats each, in the form st_group_norm_from_stats[_cat] reads (rows = stat_rows);
 * 0 (a shape it does not tile, or statistics not wanted): stats_h = stats_skip = NULL.
 * workspace: st_freeu_workspace_bytes(N, C_skip, H * W) bytes, 16-byte aligned, not shared between concurrent launches. */
size_t st_freeu_workspace_bytes(int N, int C_skip, long HW);
int st_freeu_stat_rows(long HW);
int st_freeu(const void* h, const void* skip, void* h_out, void* skip_out, int N, int C_h, int C_skip, int H, int W,
             const float* params, int slot, int dtype, float* stats_h, float* stats_skip, int stat_rows,
             void* workspace, size_t workspace_bytes, void* stream);

/* ---- perturbed-attention guidance (PAG; Ahn et al. 2024; no reference counterpart: diffusers' PAGMixin and
 * PAGCFGIdentitySelfAttnProcessor2_0, ComfyUI's PerturbedAttentionGuidance node).
 *
 * st_attention_pag: st_attention whose LAST ident_count batch entries (0 <= ident_count <= B) are perturbed: their softmax matrix is
 * the identity, so out = v for them (csrc/pag.hip).  ident_count > 0 needs T == S (self-attention).  Two launches at most: the
 * unmodified attention kernels on the leading B - ident_count entries (the same pointers with a smaller B: those entries are
 * bit-identical to st_attention on that sub-batch; skipped when there are none) and a strided row copy of ident_count * T rows of
 * H * D values from row stride ldv to row stride ldo, 16-byte accesses, no atomics, nothing written outside those rows.  Every
 * dtype and head size st_attention takes; all four pointers 16-byte aligned and all four strides multiples of 16 bytes of elements.
 * An image armed by st_arm_split_output for the whole (B * T, H * D) fp32 output is completed by both launches: the attention launch
 * writes the rows of its sub-batch, the copy the rows of the tail, bit-equal to st_split_f32 of the copied values. */
int st_attention_pag(const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H, int D,
                     long ldq, long ldk, long ldv, long ldo, float scale, int dtype, int ident_count, void* stream);

/* ---- smoothed energy guidance (SEG; Hong 2024; no reference counterpart: the published SEG pipeline for SDXL, ComfyUI's SEG node):
 * the perturbed batch entries of a self-attention run with their projected queries Gaussian-blurred over the token grid
 * (csrc/seg.hip).  Added after ABI 18 without a bump: new entry points, no existing signature or contract changed.
 *
 * st_seg_blur: q holds n * h * w rows of C values at row stride ldq (3 * H * D behind the fused q|k|v projection), token
 * t = y * w + x of every batch entry; out the same rows at row stride ldo.  Every one of the C planes of h x w becomes the separable
 * convolution g (x) g of its reflect-padded self (pad k / 2, the edge sample not repeated), fp32 accumulation, the intermediate
 * between the two passes fp32, one rounding on output.  params is a DEVICE row of ST_SEG_PARAM_WORDS floats, read when the kernels
 * run: [mode, k, g_0 ... g_{k-1}], k odd with k / 2 < min(h, w) (the kernels clamp what they read to that range); mode != 0:
 * every token of a plane becomes the plane's mean (rows summed in x order, then the row means in y order: fixed order, no
 * atomics, bitwise repeatable).  h, w <= ST_SEG_MAX_SIDE, C and both strides multiples of 16 bytes of elements, q and out 16-byte
 * aligned and not overlapping.  Grids whose fp32 plane pair fits the LDS take one launch and no workspace; the others two launches
 * through `workspace`, st_seg_blur_workspace_bytes(...) bytes (0: none needed), 16-byte aligned, not shared between concurrent
 * launches.  Nothing is written outside the n * h * w output rows.
 *
 * st_attention_seg: st_attention whose LAST tail_count batch entries (0 <= tail_count <= B) take blurred queries; tail_count > 0
 * needs T == S == h * w.  st_attention, unmodified, on the leading B - tail_count entries (bit-identical to st_attention on that
 * sub-batch; skipped when there are none), st_seg_blur of the tail's queries into `scratch` (tail_count * T dense rows of H * D
 * elements, 16-byte aligned), st_attention on the tail with q = scratch and the tail's own k, v and out rows.  tail_count == 0 is
 * st_attention (scratch, params and workspace may be NULL).  workspace as st_seg_blur's for (tail_count, h, w, H * D).  An image
 * armed by st_arm_split_output for the whole (B * T, H * D) fp32 output is handed to the two attention launches for their rows. */
#define ST_SEG_MAX_SIDE 128
#define ST_SEG_PARAM_WORDS 132              /* 2 + the 129 taps of a 128 x 128 grid, rounded up to 16 bytes */
size_t st_seg_blur_workspace_bytes(int n, int h, int w, int C, int dtype);
int st_seg_blur(const void* q, void* out, const float* params, int n, int h, int w, int C, long ldq, long ldo, int dtype,
                void* workspace, size_t workspace_bytes, void* stream);
int st_attention_seg(const void* q, const void* k, const void* v, void* out, void* scratch, int B, int T, int S, int H, int D,
                     long ldq, long ldk, long ldv, long ldo, float scale, int dtype, int tail_count, int h, int w,
                     const float* params, void* workspace, size_t workspace_bytes, void* stream);

/* ---- regional prompts (no reference counterpart: ComfyUI's conditioning masks / "attention couple", the diffusers community
 * regional-prompting pipeline): cross-attention over R key/value segments, each with its own softmax, combined per query row.
 *
 * st_attention_regions: q (B, T, H*D); k, v (B, R*seg_len, H*D), segment r = keys [r*seg_len, (r+1)*seg_len); weights (B, R, T)
 * fp32, dense;
 *   out[b,t,h,:] = sum_r weights[b,r,t] * softmax_s(scale * q[b,t,h] . k[b, r*seg_len+s, h]) v[b, r*seg_len+s, h]   (s in segment r).
 * Every segment has its own running maximum and row sum; the weighted sum is formed in fp32 from the un-rounded normalised segment
 * results and rounded to the storage type once.  The weights are not normalised here: any finite values are legal, and a segment
 * whose weight is 0 for a row contributes exactly 0 (its k / v must be finite).  With weights 1 on one segment and 0 on the others
 * the result is bit-identical to st_attention on that segment's slice of k and v.
 * dtype ST_BF16 or ST_F16, D = 64, 1 <= R <= 8, 1 <= seg_len < 256 (the range in which st_attention takes its text-context kernel);
 * ld* are token strides in elements, batch strides T*ldq, R*seg_len*ldk, R*seg_len*ldv, T*ldo; alignment as st_attention (q, k, v,
 * out 16-byte aligned; ldq, ldk, ldv multiples of 8, ldo of 4).  One launch, the text-context launch's grid; no atomics, nothing
 * written outside out; never emits a split image (csrc/attention_regions.hip). */
int st_attention_regions(const void* q, const void* k, const void* v, const float* weights, void* out,
                         int B, int T, int R, int seg_len, int H, int D,
                         long ldq, long ldk, long ldv, long ldo, float scale, int dtype, void* stream);

/* ---- ragged segmented cross-attention (no reference counterpart: IP-Adapter's decoupled cross-attention, Ye et al. 2023;
 * diffusers' IPAdapterAttnProcessor2_0): S key/value segments of different lengths in different buffers, each with its own softmax,
 * combined per query row under a live per-segment scale.
 *
 * st_attention_segments: q (B, T, H*D); segment r: k, v of `len` keys, token strides ldk / ldv and batch strides bsk / bsv in
 * elements (bs* = 0: one K / V for every batch entry); weights (B, S, T) fp32, dense; seg_scale (S) fp32 or NULL = all 1;
 *   w_eff[b,r,t] = fl32(seg_scale[r] * weights[b,r,t])
 *   out[b,t,h,:] = sum_r w_eff[b,r,t] * softmax_s(scale * q[b,t,h] . k_r[b,s,h]) v_r[b,s,h]                 (s over the len_r keys).
 * Segments run in index order; the weighted sum is formed in fp32 from the un-rounded normalised segment results and rounded to
 * the storage type once, so weights 1 under a one-hot seg_scale give the bits of st_attention on that segment, and equal lengths
 * in one buffer with seg_scale NULL give the bits of st_attention_regions.
 * `segs` is a HOST array of S descriptors, read at the call and passed to the kernel by value (a captured launch keeps them);
 * `weights` and `seg_scale` are DEVICE memory read at every launch.  A segment whose seg_scale is exactly 0 is skipped by the whole
 * grid: its k / v are never read (they need not be finite) and it contributes nothing; with every segment skipped out = 0.  A
 * segment that runs with weight 0 on a row contributes exactly 0 there (its k / v must be finite).
 * dtype ST_BF16 or ST_F16, D = 64, 1 <= S <= 8, 1 <= len < 256; q batch stride T*ldq, out T*ldo; q, out and every k, v 16-byte
 * aligned; ldq, ldk, ldv, bsk, bsv multiples of 8, ldk, ldv >= H*D, ldo a multiple of 4.  One launch, the grid of
 * st_attention_regions; no atomics, nothing written outside out; never emits a split image (csrc/attention_segments.hip). */
typedef struct { const void* k; const void* v; long ldk, ldv; long bsk, bsv; int len; } st_kv_segment;
int st_attention_segments(const void* q, const st_kv_segment* segs, int S, const float* weights, const float* seg_scale,
                          void* out, int B, int T, int H, int D, long ldq, long ldo, float scale, int dtype, void* stream);

/* ---- two-source self-attention (no reference counterpart: reference-only control - A1111's ControlNet `reference_only`,
 * ComfyUI's ReferenceOnlySimple, diffusers' community stable_diffusion_xl_reference pipeline): every query row attends to its own
 * keys AND to the keys of a reference row, under ONE softmax.  ABI 18, added without a bump: a new entry point, no existing
 * signature or contract changed.
 *
 * st_attention_joint: q (B, T, H*D), k / v (B, S1, H*D) as st_attention takes them (batch strides T*ldq, S1*ldk, S1*ldv);
 * k2 / v2: B2 entries of S2 keys, token strides ldk2 / ldv2 and batch strides bsk2 / bsv2 in elements (as st_kv_segment);
 *   out[b,t,h,:] = softmax_s( scale * q[b,t,h] . Kcat[b,s,h] ) Vcat[b,s,h]
 *   Kcat[b] = [ k[b, 0:S1] ; k2[b % B2, 0:S2_eff(b)] ]      (V likewise)
 *   S2_eff(b) = S2 if b < lead and the gate is on, else 0.
 * The gate: on iff gate_table == NULL (then gate_step must be NULL too), or gate_table[clamp(*gate_step, 0, gate_n - 1)] != 0;
 * DEVICE memory read at every launch (one scalar load of a value no launch writes: uniform over the grid), so a captured launch
 * follows in-place writes of the table and of the step counter.
 * Bit contracts (tile partition and arithmetic are st_attention's; only the address a key row is read from differs):
 *   (a) gate on and b < lead: the bits of st_attention on the contiguous concatenation of the two sources;
 *   (b) gate off, or b >= lead: the bits of st_attention with S = S1; k2 and v2 are NEVER READ and need not be finite.
 * The kernel form (3, 4 or 7 compute waves with a loader wave, or 8 self-loading waves) is st_attention's choice for (T, H, B).
 * dtype ST_BF16 or ST_F16, D = 64, S1 >= 256 (so that both contracts compare with one kernel family), S2 >= 1, B2 >= 1,
 * 0 <= lead <= B; anything else is rejected (the Python host has a slow path).  All pointers 16-byte aligned; every stride a
 * multiple of 8, token strides under 2^31, ldk2 / ldv2 >= H*D, bsk2 / bsv2 >= 0 (0: one second source for every entry), ldo a
 * multiple of 4.  One launch, no atomics, nothing written but the B*T*H*64 values of out; never emits a split image
 * (csrc/attention_joint.hip).  Parity with A1111, ComfyUI and diffusers is unpinned; their `style_fidelity`, a continuous
 * strength and the AdaIN variant are out of scope. */
int st_attention_joint(const void* q, const void* k, const void* v, const void* k2, const void* v2, void* out,
                       int B, int T, int S1, int S2, int B2, int lead, int H, int D,
                       long ldq, long ldk, long ldv, long ldk2, long ldv2, long bsk2, long bsv2, long ldo, float scale,
                       const float* gate_table, const int* gate_step, int gate_n, int dtype, void* stream);

/* The three updates with a third noise prediction: st_cfg_euler_step, st_dpmpp2m_step and st_sde_step with one more device table
 * `pag` of n_steps floats (never NULL) and one more row block of eps / next_in, the prediction under perturbed self-attention.
 * With i = *step, s = pag[i]:
 *   guidance != NULL: eps and next_in have 3*batch rows [negative | positive | perturbed],
 *                     e = e_neg + guidance[i] * (e_pos - e_neg) + s * (e_pos - e_pert);
 *   guidance == NULL: they have 2*batch rows [positive | perturbed], e = e_pos + s * (e_pos - e_pert); rescale must be NULL.
 * Everything after e is the two-way entry point's arithmetic: the rescale of the total e against std(e_pos) through the same
 * workspace, the row update, history, noise keyed by the latent sample; every row block of next_in receives the same values.
 * The same kernels under a template flag: pag[i] == 0 gives the two-way entry point's latent and history bit for bit.  Alignment,
 * per_sample % 8 == 0, workspace and determinism as there. */
int st_pag_euler_step(float* latent, const void* eps, void* next_in, const float* dsigma, const float* in_scale,
                      const float* guidance, const float* rescale, const float* pag, const int* step, int batch, long per_sample,
                      int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int st_pag_dpmpp2m_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                        const float* guidance, const float* rescale, const float* pag, const int* step, const int* start, int batch,
                        long per_sample, int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int st_pag_sde_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                    const float* guidance, const float* rescale, const float* pag, const int* step, const int* start,
                    const unsigned long long* seeds, int batch, long per_sample, int n_steps, int dtype, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- T2I-Adapter residual sites (no reference counterpart: diffusers' `down_intrablock_additional_residuals`, ComfyUI's
 * `control["input"]` / `["middle"]` entries of a T2I adapter).  Added after ABI 18 without a bump: a new entry point, no existing
 * signature or contract changed.
 *
 * st_residual_add: x (rows, HW, C) dense NHWC of `dtype`, written IN PLACE; f (f_rows, HW, C) of the same type, f_rows a divisor of
 * rows (1: one feature map for every row; the batch: the row blocks [negative | positive | perturbed] of a guided call share one
 * copy; rows: one each).  With i = *step clamped to [0, n_steps) and s = scale_table[i], both read on the device when the kernel
 * runs (a captured graph sees new values):
 *   s == 0: beyond `*step` and that table entry nothing is read, and nothing is written - x and `stats` keep their bits ("off");
 *   else    x[n][p][c] = round(fma(s, f[n % f_rows][p][c], x[n][p][c])), fp32 arithmetic, one rounding to `dtype`,
 * and, with stats != NULL, the GroupNorm partials of x are REWRITTEN for the new values: stats is the `col_stats` buffer the
 * producer of x wrote (st_linear / st_conv2d), stat_tiles x C float2 = per tile of stat_rows consecutive pixel rows and per channel
 * (sum, sum of squares) of the values as stored (after the rounding), the producers' own convention; stat_rows is what the
 * producer returned through col_stats_rows (it divides HW) and stat_tiles = rows * HW / stat_rows.  Every (tile, channel) partial is
 * written by one workgroup from sums of a fixed shape: no atomics, two launches give the same bits.  stats == NULL (stat_rows =
 * stat_tiles = 0): add only.  C a multiple of one 16-byte vector, x and f 16-byte aligned and not overlapping.  One launch, its
 * grid split over pixel tiles and channel ranges (csrc/t2i_adapter.hip). */
int st_residual_add(void* x, const void* f, int rows, int f_rows, long HW, int C, const float* scale_table, int n_steps,
                    const int* step, int dtype, float* stats, int stat_rows, int stat_tiles, void* stream);

/* st_residual_add_grouped (ControlNet's skip and middle residuals; likewise added after ABI 18 without a bump): 1..16 sites of
 * st_residual_add in ONE launch whose grid is the concatenation of the sites' own grids.  `sites` is a HOST array of descriptors,
 * read at the call and passed to the kernel by value (a captured launch keeps them): per site x, r (the residual, r_rows a divisor
 * of rows, row n reads r[n % r_rows]), stats / stat_rows / stat_tiles as in st_residual_add (stats NULL, 0, 0: add only).
 * `site_weights` is DEVICE memory of n_sites fp32 values, or NULL = all 1; scale_table, n_steps and step as in st_residual_add.
 * Site k runs under s_k = fl32(scale_table[i] * site_weights[k]):
 *   s_k == 0: the site's workgroups leave after reading those two values; nothing of its x, r, stats is read or written;
 *   else      st_residual_add's arithmetic on that site with s = s_k: the same bits in x and in the partials as that entry point
 *             gives with a table entry s_k (one fp32 fma and one rounding per element; partials of the values as stored over the
 *             producer's own tiles; fixed reduction shape, no atomics, two launches give the same bits).
 * Per site the requirements of st_residual_add; over the whole call no two byte ranges among every x, r and stats may overlap.
 * All sites share `dtype` (csrc/t2i_adapter.hip). */
typedef struct { void* x; const void* r; float* stats; int rows, r_rows; long HW; int C; int stat_rows, stat_tiles; } st_residual_site;
int st_residual_add_grouped(const st_residual_site* sites, int n_sites, const float* site_weights, const float* scale_table,
                            int n_steps, const int* step, int dtype, void* stream);

/* ---- Tiled denoising (no reference counterpart: MultiDiffusion / Mixture of Diffusers, diffusers' StableDiffusionPanoramaPipeline,
 * ComfyUI's "Tiled Diffusion").  Added after ABI 18 without a bump: new entry points, no existing signature or contract changed.
 *
 * A canvas (rows, H, W, C) and its T = ny * nx windows (rows * T, h, w, C), both dense NHWC of `dtype` (ST_BF16, ST_F16, ST_F32), C a
 * multiple of 4; window t = iy * nx + ix starts at row ys[iy] and column xs[ix], and with wrap_w its columns are taken mod W.  ys and
 * xs are HOST arrays of 1 to 16 ints each: the entry points check them and pass them by value in the launch arguments.  Rejected
 * before any launch: a window outside the canvas (ys[i] + h > H, xs[i] + w > W; with wrap_w xs[i] outside [0, W)), a canvas row or
 * column no window covers, h > H or w > W, a pointer not aligned to one 4-element vector, canvas and windows whose byte ranges
 * overlap (st_tile_blend: also a weight map that overlaps the canvas).
 *
 * st_tile_gather: windows[r * T + t][py][px][:] = canvas[r][ys[iy] + py][(xs[ix] + px) mod W][:], a copy, bit exact.
 * st_tile_blend:  for every canvas pixel (Y, X) of row r, over the n windows that cover it in ascending t, with e_t the window's
 *   element there and w_t = weights[py * w + px] at the pixel's position inside window t (weights: fp32 (h, w) DEVICE map, read when
 *   the kernel runs - a captured graph sees new values):
 *     n == 1: canvas = e_t, the bits unchanged whatever the weight;
 *     else    num = fma(w_t, float(e_t), num) from 0, den += w_t, canvas = round(num / den) to `dtype`.
 *   One thread per canvas pixel vector, no atomics: two launches give the same bits.  Weights are expected finite and positive.
 * 64-bit index arithmetic throughout (csrc/tiles.hip). */
int st_tile_gather(const void* canvas, void* windows, int rows, int H, int W, int h, int w, int C, const int* ys, int ny,
                   const int* xs, int nx, int wrap_w, int dtype, void* stream);
int st_tile_blend(const void* windows, void* canvas, const float* weights, int rows, int H, int W, int h, int w, int C,
                  const int* ys, int ny, const int* xs, int nx, int wrap_w, int dtype, void* stream);

/* ---- Masked inpainting (no reference counterpart: the post-step blend of diffusers' StableDiffusionXLInpaintPipeline; with a
 * threshold table, Differential Diffusion).  Added after ABI 18 without a bump: a new entry point, no existing signature or contract
 * changed.
 *
 * st_inpaint_blend runs BEHIND a sampler step, on what the step wrote: latent (batch, HW, C) fp32 and next_in, `blocks` row blocks of
 * (batch, HW, C) in `dtype` (ST_BF16, ST_F16, ST_F32), row r * batch + b for sample b - the denoise loop's layout, every row block the
 * same latent.  init and noise: (batch, HW, C) fp32, the latent to keep and the trajectory's unit start noise.  All dense NHWC, C a
 * multiple of 4.  mask: (mask_rows, HW) fp32 with mask_rows 1 (one mask for every sample) or batch; 1 = repaint, 0 = keep.  thr (may be
 * NULL), sigma_next and in_scale are DEVICE tables of n_steps floats, step a DEVICE int; all are read when the kernel runs (a captured
 * graph sees new values).  With i = *step clamped to [0, n_steps), s = sigma_next[i], sc = in_scale[min(i + 1, n_steps - 1)], per
 * pixel with mask value m:
 *   w = m                      when thr == NULL, or when thr[i] is NaN (the table's own "no threshold at this step": one captured
 *                              launch serves both forms),
 *   w = (m > thr[i]) ? 1 : 0   otherwise;
 *   w = !(w < 1) ? 1 : max(w, 0): NaN and values of 1 or more repaint, negative values keep;
 *   w == 1: nothing of the pixel is written, neither latent nor any next_in row (mask all ones: the buffers keep the step's bits);
 *   else    per element known = fma(s, noise, init), v = (w == 0) ? known : fma(w, latent - known, known); latent = v, and every one
 *           of the `blocks` rows of next_in = (dtype)(v * sc).
 * One thread per pixel, no atomics: two launches give the same bits.  Rejected before any launch: null pointers (thr excepted), an
 * unsupported dtype, non-positive sizes, C % 4 != 0, mask_rows other than 1 or batch, blocks < 1, latent / init / noise / next_in not
 * 16-byte aligned, mask / tables / step not 4-byte aligned, latent overlapping init, noise, mask or next_in, sizes past the index
 * range.  64-bit index arithmetic throughout (csrc/inpaint.hip). */
int st_inpaint_blend(float* latent, void* next_in, const float* init, const float* noise, const float* mask,
                     const float* thr, const float* sigma_next, const float* in_scale, const int* step,
                     int batch, int blocks, long HW, int C, int mask_rows, int n_steps, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
