// Error plumbing, ABI version, and the small device-side pieces of the denoise
// loop (Euler update, step counter, sinusoidal timestep features).
#include "common.h"
#include "philox.h"

static thread_local char g_err[512] = "";

// ---- split image of the NEXT launch's output (strict mode; header: st_arm_split_output) -------------------------------
static thread_local struct { void* p; long rows; int cols; } g_split_arm = {nullptr, 0, 0};

extern "C" int st_arm_split_output(void* ys, long rows, int cols) {
    if (!ys) { g_split_arm = {nullptr, 0, 0}; return 0; }      // disarm (a caller whose armed launch was rejected before it looked at the arm)
    ST_REQUIRE(rows > 0 && cols > 0 && cols % 32 == 0 && (uintptr_t)ys % 16 == 0, "arm_split_output: (rows, cols) image with cols %% 32 == 0 expected");
    g_split_arm = {ys, rows, cols};
    return 0;
}

// Called by every entry point that can emit: returns the armed image for an output of (rows, cols) fp32 values and disarms
// it; a launch that is armed but cannot emit (other element type, other shape) fails, so an armed image is never left
// unwritten without the caller hearing of it.
int st_take_split_arm(const char* who, long rows, int cols, bool can_emit, void** out) {
    *out = nullptr;
    if (!g_split_arm.p) return 0;
    const auto arm = g_split_arm;
    g_split_arm = {nullptr, 0, 0};
    ST_REQUIRE(can_emit, "%s: a split output image was armed, but this launch cannot emit one (fp32 outputs only)", who);
    ST_REQUIRE(arm.rows == rows && arm.cols == cols, "%s: the armed split image is (%ld, %d), the output is (%ld, %d)", who, arm.rows, arm.cols, rows, cols);
    *out = arm.p;
    return 0;
}

int st_fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

int st_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return st_fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

extern "C" const char* st_last_error(void) { return g_err; }
extern "C" int st_abi_version(void) { return 18; }

// ---- Euler-discrete update ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void euler_kernel(float* __restrict__ latent, const T* __restrict__ eps, T* __restrict__ next_in,
                                                    const float* __restrict__ dsigma, const float* __restrict__ in_scale,
                                                    const int* __restrict__ step, long n, int n_steps) {
    const int i = *step;
    const float ds = dsigma[i];
    const float sc = in_scale[i + 1 < n_steps ? i + 1 : n_steps - 1];
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        float x = latent[j] + Elem<T>::to_f(eps[j]) * ds;
        latent[j] = x;
        next_in[j] = Elem<T>::from_f(x * sc);
    }
}

extern "C" int st_euler_step(float* latent, const void* eps, void* next_in, const float* dsigma, const float* in_scale,
                             const int* step, long n, int n_steps, int dtype, void* stream) {
    ST_REQUIRE(latent && eps && next_in && dsigma && in_scale && step, "euler_step: null pointer");
    ST_REQUIRE(n > 0 && n_steps > 0, "euler_step: bad sizes");
    int grid = (int)((n + 255) / 256);
    if (grid > 2048) grid = 2048;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16)
        hipLaunchKernelGGL(euler_kernel<bf16>, dim3(grid), dim3(256), 0, st, latent, (const bf16*)eps, (bf16*)next_in, dsigma, in_scale, step, n, n_steps);
    else if (dtype == ST_F16)
        hipLaunchKernelGGL(euler_kernel<f16>, dim3(grid), dim3(256), 0, st, latent, (const f16*)eps, (f16*)next_in, dsigma, in_scale, step, n, n_steps);
    else if (dtype == ST_F32)
        hipLaunchKernelGGL(euler_kernel<float>, dim3(grid), dim3(256), 0, st, latent, (const float*)eps, (float*)next_in, dsigma, in_scale, step, n, n_steps);
    else
        return st_fail("euler_step: unsupported dtype %d", dtype);
    return st_check_launch("euler_step");
}

// ---- classifier-free guidance + Euler update ----------------------------------------------------------------------------
// Restated third-party arithmetic (the reference leaves it to its Diffusers pipeline, diffusers 0.21.2
// StableDiffusionXLPipeline.__call__ and its `rescale_noise_cfg`), per sample b, i = *step, all in fp32:
//   e   = e_neg + g[i] * (e_pos - e_neg)                      e_neg = eps row b, e_pos = eps row B + b (cat([uncond, cond]))
//   e   = phi * (e * (std(e_pos) / std(e))) + (1 - phi) * e   only with a rescale table, phi = rescale[i]; std over the
//                                                             sample's C*H*W values with correction 1 (torch.std), no guard
//                                                             against std(e) == 0 (diffusers has none)
//   latent += e * dsigma[i];  next_in rows b and B + b = latent * in_scale[min(i + 1, n - 1)]
// Both kernels map one block to CFG_BLOCK_ELEMS consecutive values of one sample (blockIdx.y = sample), 8 per lane as 16-byte
// vectors.  The std needs the whole sample before any value can be written, and the rescale path must replay bit for bit: no
// atomics and no hand-off between blocks of one launch.  Launch 1 writes each block's fp64 (sum, sum of squares) of e_pos and e
// to its own workspace slot; launch 2 has every block of a sample re-reduce that sample's slots in one fixed order (so all of
// them compute the same ratio), then apply.  Without a rescale table launch 2 runs alone.
constexpr int CFG_THREADS = 256, CFG_VEC = 8, CFG_BLOCK_ELEMS = CFG_THREADS * CFG_VEC;

static inline long cfg_blocks_per_sample(long per_sample) { return (per_sample + CFG_BLOCK_ELEMS - 1) / CFG_BLOCK_ELEMS; }

template <typename T>
__device__ __forceinline__ void cfg_load8(const T* p, float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        const Vec16<T> a = load16(p), b = load16(p + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = a.get(k); v[4 + k] = b.get(k); }
    } else {
        const Vec16<T> a = load16(p);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = a.get(k);
    }
}

template <typename T>
__device__ __forceinline__ void cfg_store8(T* p, const float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        Vec16<T> a, b;
#pragma unroll
        for (int k = 0; k < 4; ++k) { a.set(k, v[k]); b.set(k, v[4 + k]); }
        store16(p, a);
        store16(p + 4, b);
    } else {
        Vec16<T> a;
#pragma unroll
        for (int k = 0; k < 8; ++k) a.set(k, v[k]);
        store16(p, a);
    }
}

// The PAG instantiations of the kernels below take one more argument, the `pag` table, as a parameter pack: the plain instantiations
// keep the parameter list (and with it the kernel-argument layout and the code) they always had.
__device__ __forceinline__ const float* pag_table() { return nullptr; }
__device__ __forceinline__ const float* pag_table(const float* p) { return p; }

// the guided eps of 8 values at offset j of sample b (also returns e_pos for the statistics).  PAG (perturbed-attention
// guidance, below): one more row block [.. | perturbed] and e += s * (e_pos - e_pert); GUIDED = false (PAG only): rows
// [positive | perturbed], e = e_pos + s * (e_pos - e_pert).  The plain instantiation <T> is the code it always was.
template <typename T, bool PAG = false, bool GUIDED = true>
__device__ __forceinline__ void cfg_guided8(const T* __restrict__ eps, int batch, int b, long per_sample, long j, float g, float s,
                                            float (&e)[8], float (&pos)[8]) {
    static_assert(PAG || GUIDED, "cfg_guided8: nothing to combine");
    if constexpr (GUIDED) {
        float neg[8];
        cfg_load8(eps + (long)b * per_sample + j, neg);
        cfg_load8(eps + (long)(batch + b) * per_sample + j, pos);
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = neg[k] + g * (pos[k] - neg[k]);
    } else {
        cfg_load8(eps + (long)b * per_sample + j, pos);
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = pos[k];
    }
    if constexpr (PAG) {
        float pert[8];
        cfg_load8(eps + (long)((GUIDED ? 2 : 1) * batch + b) * per_sample + j, pert);
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = e[k] + s * (pos[k] - pert[k]);      // s = 0: + 0 * finite, the two-way value
    }
}

// launch 1 (rescale only): ws[(b * nblk + blk) * 4 + {0..3}] = fp64 (sum e_pos, sum e_pos^2, sum e, sum e^2) over the block's values
template <typename T, bool PAG = false, typename... Extra>
__global__ __launch_bounds__(CFG_THREADS) void cfg_stats_kernel(const T* __restrict__ eps, const float* __restrict__ guidance,
                                                                const int* __restrict__ step, int batch, long per_sample,
                                                                double* __restrict__ ws, Extra... extra) {
    const float* __restrict__ pag = pag_table(extra...);
    const int b = blockIdx.y;
    const long j = (long)blockIdx.x * CFG_BLOCK_ELEMS + threadIdx.x * CFG_VEC;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (j < per_sample) {                        // per_sample % 8 == 0: a lane's 8 values are all inside or all outside
        float e[8], pos[8];
        float s = 0.f;
        if constexpr (PAG) s = pag[*step];
        cfg_guided8<T, PAG>(eps, batch, b, per_sample, j, guidance[*step], s, e, pos);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double p = pos[k], q = e[k];
            acc[0] += p; acc[1] = fma(p, p, acc[1]);
            acc[2] += q; acc[3] = fma(q, q, acc[3]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o, 64);
    __shared__ double part[CFG_THREADS / 64][4];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0)
        for (int k = 0; k < 4; ++k) part[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = part[0][threadIdx.x];
        for (int w = 1; w < CFG_THREADS / 64; ++w) s += part[w][threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = s;
    }
}

// launch 2's std(e_pos) / std(e) of sample b, the same value in every block of the sample: every block reduces the same slots
// in the same order (lane l takes slots l, l + 64, ..., then a fixed tree).  Called by every thread of the block (a barrier).
__device__ __forceinline__ float cfg_rescale_ratio(const double* __restrict__ ws, int b, long per_sample) {
    __shared__ float ratio_s;
    if (threadIdx.x < 64) {
        const double* p = ws + (long)b * gridDim.x * 4;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int s = threadIdx.x; s < (int)gridDim.x; s += 64)
            for (int k = 0; k < 4; ++k) acc[k] += p[(long)s * 4 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o, 64);
        if (threadIdx.x == 0) {
            const double n = (double)per_sample;
            const double var_pos = (acc[1] - acc[0] * (acc[0] / n)) / (n - 1.0);
            const double var_e = (acc[3] - acc[2] * (acc[2] / n)) / (n - 1.0);
            ratio_s = (float)(sqrt(var_pos) / sqrt(var_e));
        }
    }
    __syncthreads();
    return ratio_s;
}

// launch 2: guidance (+ rescale with the sample's ratio) + Euler update + both halves of the next UNet input
template <typename T, bool RESCALE, bool PAG = false, bool GUIDED = true, typename... Extra>
__global__ __launch_bounds__(CFG_THREADS) void cfg_euler_kernel(float* __restrict__ latent, const T* __restrict__ eps, T* __restrict__ next_in,
                                                                const float* __restrict__ dsigma, const float* __restrict__ in_scale,
                                                                const float* __restrict__ guidance, const float* __restrict__ rescale,
                                                                const int* __restrict__ step, int batch, long per_sample, int n_steps,
                                                                const double* __restrict__ ws, Extra... extra) {
    const float* __restrict__ pag = pag_table(extra...);
    static_assert(GUIDED || !RESCALE, "guidance rescale needs classifier-free guidance");
    const int b = blockIdx.y, i = *step;
    float ratio = 1.f, phi = 0.f;
    if constexpr (RESCALE) {
        ratio = cfg_rescale_ratio(ws, b, per_sample);
        phi = rescale[i];
    }
    const long j = (long)blockIdx.x * CFG_BLOCK_ELEMS + threadIdx.x * CFG_VEC;
    if (j >= per_sample) return;
    float g = 0.f, s = 0.f;
    if constexpr (GUIDED) g = guidance[i];
    if constexpr (PAG) s = pag[i];
    const float ds = dsigma[i];
    const float sc = in_scale[i + 1 < n_steps ? i + 1 : n_steps - 1];
    float e[8], pos[8], x[8];
    cfg_guided8<T, PAG, GUIDED>(eps, batch, b, per_sample, j, g, s, e, pos);
    if constexpr (RESCALE) {
        const float keep = 1.f - phi;
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = phi * (e[k] * ratio) + keep * e[k];      // phi = 0: 0 * r + 1 * e == e, the plain path's bits
    }
    float* lat = latent + (long)b * per_sample + j;
    {
        const f32x4 a = *reinterpret_cast<const f32x4*>(lat), c = *reinterpret_cast<const f32x4*>(lat + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { x[k] = a[k]; x[4 + k] = c[k]; }
    }
    float y[8];
    f32x4 a, c;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        x[k] = x[k] + e[k] * ds;
        y[k] = x[k] * sc;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = x[k]; c[k] = x[4 + k]; }
    *reinterpret_cast<f32x4*>(lat) = a;
    *reinterpret_cast<f32x4*>(lat + 4) = c;
    cfg_store8(next_in + (long)b * per_sample + j, y);
    if constexpr (GUIDED) cfg_store8(next_in + (long)(batch + b) * per_sample + j, y);
    if constexpr (PAG) cfg_store8(next_in + (long)((GUIDED ? 2 : 1) * batch + b) * per_sample + j, y);      // every row block: the same values
}

extern "C" size_t st_cfg_step_workspace_bytes(int batch, long per_sample) {
    if (batch <= 0 || per_sample <= 0) return 0;
    return (size_t)batch * (size_t)cfg_blocks_per_sample(per_sample) * 4 * sizeof(double);
}

template <typename T>
static int cfg_launch(float* latent, const void* eps, void* next_in, const float* dsigma, const float* in_scale, const float* guidance,
                       const float* rescale, const float* pag, const int* step, int batch, long per_sample, int n_steps, double* ws,
                       hipStream_t st) {
    const dim3 grid((unsigned)cfg_blocks_per_sample(per_sample), (unsigned)batch);
    if (pag) {                                   // the three-way instantiations (st_pag_euler_step)
        if (rescale) {
            hipLaunchKernelGGL((cfg_stats_kernel<T, true, const float*>), grid, dim3(CFG_THREADS), 0, st, (const T*)eps, guidance, step, batch, per_sample, ws, pag);
            if (st_check_launch("pag_euler_step (statistics)")) return 1;
            hipLaunchKernelGGL((cfg_euler_kernel<T, true, true, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, dsigma,
                               in_scale, guidance, rescale, step, batch, per_sample, n_steps, (const double*)ws, pag);
        } else if (guidance) {
            hipLaunchKernelGGL((cfg_euler_kernel<T, false, true, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, dsigma,
                               in_scale, guidance, rescale, step, batch, per_sample, n_steps, (const double*)nullptr, pag);
        } else {
            hipLaunchKernelGGL((cfg_euler_kernel<T, false, true, false, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, dsigma,
                               in_scale, guidance, rescale, step, batch, per_sample, n_steps, (const double*)nullptr, pag);
        }
        return st_check_launch("pag_euler_step");
    }
    if (rescale) {
        hipLaunchKernelGGL(cfg_stats_kernel<T>, grid, dim3(CFG_THREADS), 0, st, (const T*)eps, guidance, step, batch, per_sample, ws);
        if (st_check_launch("cfg_euler_step (statistics)")) return 1;
        hipLaunchKernelGGL((cfg_euler_kernel<T, true>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, dsigma,
                           in_scale, guidance, rescale, step, batch, per_sample, n_steps, (const double*)ws);
    } else {
        hipLaunchKernelGGL((cfg_euler_kernel<T, false>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, dsigma,
                           in_scale, guidance, rescale, step, batch, per_sample, n_steps, (const double*)nullptr);
    }
    return st_check_launch("cfg_euler_step");
}

// shared by st_cfg_euler_step (pag_entry false: `pag` is NULL, `guidance` required) and st_pag_euler_step
static int cfg_euler_entry(const char* who, bool pag_entry, float* latent, const void* eps, void* next_in, const float* dsigma,
                           const float* in_scale, const float* guidance, const float* rescale, const float* pag, const int* step,
                           int batch, long per_sample, int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    ST_REQUIRE(latent && eps && next_in && dsigma && in_scale && (pag_entry ? pag != nullptr : guidance != nullptr) && step, "%s: null pointer", who);
    ST_REQUIRE(!rescale || guidance, "%s: a rescale table needs a guidance table", who);
    ST_REQUIRE(batch > 0 && per_sample > 0 && n_steps > 0, "%s: bad sizes (batch %d, per_sample %ld, n_steps %d)", who,
               batch, per_sample, n_steps);
    ST_REQUIRE(per_sample % CFG_VEC == 0, "%s: per_sample %ld is not a multiple of %d (16-byte vectors)", who, per_sample, CFG_VEC);
    ST_REQUIRE(cfg_blocks_per_sample(per_sample) <= 0x7fffffffL && batch <= 65535, "%s: grid too large", who);
    ST_REQUIRE((uintptr_t)latent % 16 == 0 && (uintptr_t)eps % 16 == 0 && (uintptr_t)next_in % 16 == 0,
               "%s: latent, eps and next_in must be 16-byte aligned", who);
    if (rescale) {
        const size_t need = st_cfg_step_workspace_bytes(batch, per_sample);
        ST_REQUIRE(workspace && workspace_bytes >= need, "%s: the rescale path needs a workspace of %zu bytes, got %zu", who,
                   need, workspace ? workspace_bytes : (size_t)0);
        ST_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    }
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    if (dtype == ST_BF16)
        return cfg_launch<bf16>(latent, eps, next_in, dsigma, in_scale, guidance, rescale, pag, step, batch, per_sample, n_steps, ws, st);
    if (dtype == ST_F16)
        return cfg_launch<f16>(latent, eps, next_in, dsigma, in_scale, guidance, rescale, pag, step, batch, per_sample, n_steps, ws, st);
    if (dtype == ST_F32)
        return cfg_launch<float>(latent, eps, next_in, dsigma, in_scale, guidance, rescale, pag, step, batch, per_sample, n_steps, ws, st);
    return st_fail("%s: unsupported dtype %d", who, dtype);
}

extern "C" int st_cfg_euler_step(float* latent, const void* eps, void* next_in, const float* dsigma, const float* in_scale,
                                 const float* guidance, const float* rescale, const int* step, int batch, long per_sample,
                                 int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return cfg_euler_entry("cfg_euler_step", false, latent, eps, next_in, dsigma, in_scale, guidance, rescale, nullptr, step, batch,
                           per_sample, n_steps, dtype, workspace, workspace_bytes, stream);
}

// ---- perturbed-attention guidance (PAG; Ahn et al. 2024; restated diffusers PAGMixin) in the three updates ------------------
// One more row block of eps / next_in, the UNet's prediction with the perturbed self-attention (csrc/pag.hip), and one more device
// table `pag` of n_steps floats, s = pag[i]:
//   guidance != NULL   rows [negative | positive | perturbed], 3 * batch:   e = e_neg + g * (e_pos - e_neg) + s * (e_pos - e_pert)
//   guidance == NULL   rows [positive | perturbed], 2 * batch:              e = e_pos + s * (e_pos - e_pert)   (no rescale)
// Everything after e is the arithmetic above and below, unchanged: the rescale statistics of the total e against e_pos through the
// same workspace, the Euler / DPM++ / SDE row update, the history, the noise keyed by the latent sample; every row block of next_in
// receives the same values.  The kernels are the existing ones with a PAG template flag (cfg_guided8, cfg_stats_kernel and the
// three update kernels), so s = 0 gives the two-way kernels' latent and history bit for bit.
extern "C" int st_pag_euler_step(float* latent, const void* eps, void* next_in, const float* dsigma, const float* in_scale,
                                 const float* guidance, const float* rescale, const float* pag, const int* step, int batch,
                                 long per_sample, int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return cfg_euler_entry("pag_euler_step", true, latent, eps, next_in, dsigma, in_scale, guidance, rescale, pag, step, batch,
                           per_sample, n_steps, dtype, workspace, workspace_bytes, stream);
}

// ---- DPM-Solver++(2M) update (scheduler.py docstring; k-diffusion's sample_dpmpp_2m in sigma form) ----------------------
// Per sample b, i = *step, coef row i = [sigma, a, bb, k], all in fp32:
//   e = eps row b (unguided), or the guided (+ rescaled) eps of st_cfg_euler_step from rows b and B + b
//   d = x - sigma * e
//   x = a * x + bb * ((1 + k) * d - k * d_prev)   second order, d_prev = history; only when i != *start and k != 0
//   x = a * x + bb * d                            first order: history is not read (a branch, so stale or NaN values
//                                                 never reach the output)
//   history = d;  next_in row b (and B + b when guided) = x * in_scale[min(i + 1, n - 1)]
// The block mapping, the 16-byte vectors and the rescale statistics (cfg_stats_kernel, launch 1) are the CFG kernel's.
template <typename T, bool GUIDED, bool RESCALE, bool PAG = false, typename... Extra>
__global__ __launch_bounds__(CFG_THREADS) void dpmpp2m_kernel(float* __restrict__ latent, const T* __restrict__ eps, T* __restrict__ next_in,
                                                              float* __restrict__ history, const float* __restrict__ coef,
                                                              const float* __restrict__ in_scale, const float* __restrict__ guidance,
                                                              const float* __restrict__ rescale, const int* __restrict__ step,
                                                              const int* __restrict__ start, int batch, long per_sample, int n_steps,
                                                              const double* __restrict__ ws, Extra... extra) {
    const float* __restrict__ pag = pag_table(extra...);
    const int b = blockIdx.y, i = *step;
    float ratio = 1.f, phi = 0.f;
    if constexpr (RESCALE) {
        ratio = cfg_rescale_ratio(ws, b, per_sample);
        phi = rescale[i];
    }
    const long j = (long)blockIdx.x * CFG_BLOCK_ELEMS + threadIdx.x * CFG_VEC;
    if (j >= per_sample) return;
    const float sigma = coef[4 * i], a = coef[4 * i + 1], bb = coef[4 * i + 2], k = coef[4 * i + 3];
    const bool second = i != *start && k != 0.f;
    const float sc = in_scale[i + 1 < n_steps ? i + 1 : n_steps - 1];
    float e[8];
    if constexpr (GUIDED || PAG) {
        float pos[8], g = 0.f, s = 0.f;
        if constexpr (GUIDED) g = guidance[i];
        if constexpr (PAG) s = pag[i];
        cfg_guided8<T, PAG, GUIDED>(eps, batch, b, per_sample, j, g, s, e, pos);
        if constexpr (RESCALE) {
            const float keep = 1.f - phi;
#pragma unroll
            for (int q = 0; q < 8; ++q) e[q] = phi * (e[q] * ratio) + keep * e[q];   // phi = 0: the plain path's bits
        }
    } else {
        cfg_load8(eps + (long)b * per_sample + j, e);
    }
    float* lat = latent + (long)b * per_sample + j;
    float* hist = history + (long)b * per_sample + j;
    float x[8], d[8], y[8];
    cfg_load8(lat, x);
#pragma unroll
    for (int q = 0; q < 8; ++q) d[q] = x[q] - sigma * e[q];
    if (second) {
        float prev[8];
        cfg_load8(hist, prev);
        const float kp = 1.f + k;
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = a * x[q] + bb * (kp * d[q] - k * prev[q]);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = a * x[q] + bb * d[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = x[q] * sc;
    cfg_store8(hist, d);
    cfg_store8(lat, x);
    cfg_store8(next_in + (long)b * per_sample + j, y);
    if constexpr (GUIDED) cfg_store8(next_in + (long)(batch + b) * per_sample + j, y);
    if constexpr (PAG) cfg_store8(next_in + (long)((GUIDED ? 2 : 1) * batch + b) * per_sample + j, y);      // every row block: the same values
}

template <typename T>
static int dpm_launch(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                      const float* guidance, const float* rescale, const float* pag, const int* step, const int* start, int batch,
                      long per_sample, int n_steps, double* ws, hipStream_t st) {
    const dim3 grid((unsigned)cfg_blocks_per_sample(per_sample), (unsigned)batch);
    if (pag) {                                   // the three-way instantiations (st_pag_dpmpp2m_step)
        if (rescale) {
            hipLaunchKernelGGL((cfg_stats_kernel<T, true, const float*>), grid, dim3(CFG_THREADS), 0, st, (const T*)eps, guidance, step, batch, per_sample, ws, pag);
            if (st_check_launch("pag_dpmpp2m_step (statistics)")) return 1;
            hipLaunchKernelGGL((dpmpp2m_kernel<T, true, true, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                               coef, in_scale, guidance, rescale, step, start, batch, per_sample, n_steps, (const double*)ws, pag);
        } else if (guidance) {
            hipLaunchKernelGGL((dpmpp2m_kernel<T, true, false, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                               coef, in_scale, guidance, rescale, step, start, batch, per_sample, n_steps, (const double*)nullptr, pag);
        } else {
            hipLaunchKernelGGL((dpmpp2m_kernel<T, false, false, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                               coef, in_scale, guidance, rescale, step, start, batch, per_sample, n_steps, (const double*)nullptr, pag);
        }
        return st_check_launch("pag_dpmpp2m_step");
    }
    if (rescale) {
        hipLaunchKernelGGL(cfg_stats_kernel<T>, grid, dim3(CFG_THREADS), 0, st, (const T*)eps, guidance, step, batch, per_sample, ws);
        if (st_check_launch("dpmpp2m_step (statistics)")) return 1;
        hipLaunchKernelGGL((dpmpp2m_kernel<T, true, true>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                           coef, in_scale, guidance, rescale, step, start, batch, per_sample, n_steps, (const double*)ws);
    } else if (guidance) {
        hipLaunchKernelGGL((dpmpp2m_kernel<T, true, false>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                           coef, in_scale, guidance, rescale, step, start, batch, per_sample, n_steps, (const double*)nullptr);
    } else {
        hipLaunchKernelGGL((dpmpp2m_kernel<T, false, false>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                           coef, in_scale, guidance, rescale, step, start, batch, per_sample, n_steps, (const double*)nullptr);
    }
    return st_check_launch("dpmpp2m_step");
}

// shared by st_dpmpp2m_step (pag_entry false: `pag` is NULL) and st_pag_dpmpp2m_step
static int dpm_entry(const char* who, bool pag_entry, float* latent, const void* eps, void* next_in, float* history, const float* coef,
                     const float* in_scale, const float* guidance, const float* rescale, const float* pag, const int* step,
                     const int* start, int batch, long per_sample, int n_steps, int dtype, void* workspace, size_t workspace_bytes,
                     void* stream) {
    ST_REQUIRE(latent && eps && next_in && history && coef && in_scale && step && start && (!pag_entry || pag), "%s: null pointer", who);
    ST_REQUIRE(!rescale || guidance, "%s: a rescale table needs a guidance table", who);
    ST_REQUIRE(batch > 0 && per_sample > 0 && n_steps > 0, "%s: bad sizes (batch %d, per_sample %ld, n_steps %d)", who,
               batch, per_sample, n_steps);
    ST_REQUIRE(per_sample % CFG_VEC == 0, "%s: per_sample %ld is not a multiple of %d (16-byte vectors)", who, per_sample, CFG_VEC);
    ST_REQUIRE(cfg_blocks_per_sample(per_sample) <= 0x7fffffffL && batch <= 65535, "%s: grid too large", who);
    ST_REQUIRE((uintptr_t)latent % 16 == 0 && (uintptr_t)eps % 16 == 0 && (uintptr_t)next_in % 16 == 0 && (uintptr_t)history % 16 == 0,
               "%s: latent, eps, next_in and history must be 16-byte aligned", who);
    if (rescale) {
        const size_t need = st_cfg_step_workspace_bytes(batch, per_sample);
        ST_REQUIRE(workspace && workspace_bytes >= need, "%s: the rescale path needs a workspace of %zu bytes, got %zu", who,
                   need, workspace ? workspace_bytes : (size_t)0);
        ST_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    }
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    if (dtype == ST_BF16)
        return dpm_launch<bf16>(latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, batch, per_sample, n_steps, ws, st);
    if (dtype == ST_F16)
        return dpm_launch<f16>(latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, batch, per_sample, n_steps, ws, st);
    if (dtype == ST_F32)
        return dpm_launch<float>(latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, batch, per_sample, n_steps, ws, st);
    return st_fail("%s: unsupported dtype %d", who, dtype);
}

extern "C" int st_dpmpp2m_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                               const float* guidance, const float* rescale, const int* step, const int* start, int batch,
                               long per_sample, int n_steps, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
    return dpm_entry("dpmpp2m_step", false, latent, eps, next_in, history, coef, in_scale, guidance, rescale, nullptr, step, start, batch,
                     per_sample, n_steps, dtype, workspace, workspace_bytes, stream);
}

// st_dpmpp2m_step with the perturbed row block (st_pag_euler_step's comment states e)
extern "C" int st_pag_dpmpp2m_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                                   const float* guidance, const float* rescale, const float* pag, const int* step, const int* start,
                                   int batch, long per_sample, int n_steps, int dtype, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    return dpm_entry("pag_dpmpp2m_step", true, latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, batch,
                     per_sample, n_steps, dtype, workspace, workspace_bytes, stream);
}

// ---- stochastic samplers: Euler ancestral, DPM++ 2M SDE (scheduler.py docstring), with counter-based noise (philox.h) ------
// The DPM++(2M) update plus one noise column.  Per sample b, i = *step, coef row i = [sigma, a, bb, k, c], all in fp32:
//   e, d = x - sigma * e and x = a * x + bb * (...) exactly as dpmpp2m_kernel (same first-order branch on *start and k)
//   x += c * z    only when c != 0 (a branch: the last step and eta = 0 never run the generator, and then every bit is
//                 dpmpp2m_kernel's); z = the stream of seeds[b] at counter word i + 1, element j of the sample
//   history = d;  next_in row b (and B + b when guided) = x * in_scale[min(i + 1, n - 1)]
// With guidance the noise belongs to latent sample b (B seeds), not to the 2B UNet rows.  A lane's 8 values start at a
// multiple of 8: exactly the two Philox calls q = j / 4 and j / 4 + 1.
template <typename T, bool GUIDED, bool RESCALE, bool PAG = false, typename... Extra>
__global__ __launch_bounds__(CFG_THREADS) void sde_kernel(float* __restrict__ latent, const T* __restrict__ eps, T* __restrict__ next_in,
                                                          float* __restrict__ history, const float* __restrict__ coef,
                                                          const float* __restrict__ in_scale, const float* __restrict__ guidance,
                                                          const float* __restrict__ rescale, const int* __restrict__ step,
                                                          const int* __restrict__ start, const unsigned long long* __restrict__ seeds,
                                                          int batch, long per_sample, int n_steps, const double* __restrict__ ws,
                                                          Extra... extra) {
    const float* __restrict__ pag = pag_table(extra...);
    const int b = blockIdx.y, i = *step;
    float ratio = 1.f, phi = 0.f;
    if constexpr (RESCALE) {
        ratio = cfg_rescale_ratio(ws, b, per_sample);
        phi = rescale[i];
    }
    const long j = (long)blockIdx.x * CFG_BLOCK_ELEMS + threadIdx.x * CFG_VEC;
    if (j >= per_sample) return;
    const float sigma = coef[5 * i], a = coef[5 * i + 1], bb = coef[5 * i + 2], k = coef[5 * i + 3], c = coef[5 * i + 4];
    const bool second = i != *start && k != 0.f;
    const float sc = in_scale[i + 1 < n_steps ? i + 1 : n_steps - 1];
    float e[8];
    if constexpr (GUIDED || PAG) {
        float pos[8], g = 0.f, s = 0.f;
        if constexpr (GUIDED) g = guidance[i];
        if constexpr (PAG) s = pag[i];
        cfg_guided8<T, PAG, GUIDED>(eps, batch, b, per_sample, j, g, s, e, pos);
        if constexpr (RESCALE) {
            const float keep = 1.f - phi;
#pragma unroll
            for (int q = 0; q < 8; ++q) e[q] = phi * (e[q] * ratio) + keep * e[q];   // phi = 0: the plain path's bits
        }
    } else {
        cfg_load8(eps + (long)b * per_sample + j, e);
    }
    float* lat = latent + (long)b * per_sample + j;
    float* hist = history + (long)b * per_sample + j;
    float x[8], d[8], y[8], z[8];
    cfg_load8(lat, x);
    const bool noisy = c != 0.f;
    if (noisy) {                 // drawn before the loaded values are first used: the loads above are in flight meanwhile
        const PhiloxKey key = philox_key(seeds[b]);
        const unsigned q0 = (unsigned)(j >> 2), ctr = (unsigned)(i + 1);
        philox_normal4(key, q0, ctr, z);
        philox_normal4(key, q0 + 1u, ctr, z + 4);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) d[q] = x[q] - sigma * e[q];
    if (second) {
        float prev[8];
        cfg_load8(hist, prev);
        const float kp = 1.f + k;
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = a * x[q] + bb * (kp * d[q] - k * prev[q]);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = a * x[q] + bb * d[q];
    }
    if (noisy) {
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = x[q] + c * z[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = x[q] * sc;
    cfg_store8(hist, d);
    cfg_store8(lat, x);
    cfg_store8(next_in + (long)b * per_sample + j, y);
    if constexpr (GUIDED) cfg_store8(next_in + (long)(batch + b) * per_sample + j, y);
    if constexpr (PAG) cfg_store8(next_in + (long)((GUIDED ? 2 : 1) * batch + b) * per_sample + j, y);      // every row block: the same values
}

template <typename T>
static int sde_launch(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                      const float* guidance, const float* rescale, const float* pag, const int* step, const int* start,
                      const unsigned long long* seeds, int batch, long per_sample, int n_steps, double* ws, hipStream_t st) {
    const dim3 grid((unsigned)cfg_blocks_per_sample(per_sample), (unsigned)batch);
    if (pag) {                                   // the three-way instantiations (st_pag_sde_step)
        if (rescale) {
            hipLaunchKernelGGL((cfg_stats_kernel<T, true, const float*>), grid, dim3(CFG_THREADS), 0, st, (const T*)eps, guidance, step, batch, per_sample, ws, pag);
            if (st_check_launch("pag_sde_step (statistics)")) return 1;
            hipLaunchKernelGGL((sde_kernel<T, true, true, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                               coef, in_scale, guidance, rescale, step, start, seeds, batch, per_sample, n_steps, (const double*)ws, pag);
        } else if (guidance) {
            hipLaunchKernelGGL((sde_kernel<T, true, false, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                               coef, in_scale, guidance, rescale, step, start, seeds, batch, per_sample, n_steps, (const double*)nullptr, pag);
        } else {
            hipLaunchKernelGGL((sde_kernel<T, false, false, true, const float*>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                               coef, in_scale, guidance, rescale, step, start, seeds, batch, per_sample, n_steps, (const double*)nullptr, pag);
        }
        return st_check_launch("pag_sde_step");
    }
    if (rescale) {
        hipLaunchKernelGGL(cfg_stats_kernel<T>, grid, dim3(CFG_THREADS), 0, st, (const T*)eps, guidance, step, batch, per_sample, ws);
        if (st_check_launch("sde_step (statistics)")) return 1;
        hipLaunchKernelGGL((sde_kernel<T, true, true>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                           coef, in_scale, guidance, rescale, step, start, seeds, batch, per_sample, n_steps, (const double*)ws);
    } else if (guidance) {
        hipLaunchKernelGGL((sde_kernel<T, true, false>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                           coef, in_scale, guidance, rescale, step, start, seeds, batch, per_sample, n_steps, (const double*)nullptr);
    } else {
        hipLaunchKernelGGL((sde_kernel<T, false, false>), grid, dim3(CFG_THREADS), 0, st, latent, (const T*)eps, (T*)next_in, history,
                           coef, in_scale, guidance, rescale, step, start, seeds, batch, per_sample, n_steps, (const double*)nullptr);
    }
    return st_check_launch("sde_step");
}

// the generator's counter word is 32 bits: a sample holds at most 4 * 2^32 values
constexpr long PHILOX_MAX_PER_SAMPLE = 4L << 32;

// shared by st_sde_step (pag_entry false: `pag` is NULL) and st_pag_sde_step
static int sde_entry(const char* who, bool pag_entry, float* latent, const void* eps, void* next_in, float* history, const float* coef,
                     const float* in_scale, const float* guidance, const float* rescale, const float* pag, const int* step,
                     const int* start, const unsigned long long* seeds, int batch, long per_sample, int n_steps, int dtype,
                     void* workspace, size_t workspace_bytes, void* stream) {
    ST_REQUIRE(latent && eps && next_in && history && coef && in_scale && step && start && seeds && (!pag_entry || pag), "%s: null pointer", who);
    ST_REQUIRE(!rescale || guidance, "%s: a rescale table needs a guidance table", who);
    ST_REQUIRE(batch > 0 && per_sample > 0 && n_steps > 0, "%s: bad sizes (batch %d, per_sample %ld, n_steps %d)", who,
               batch, per_sample, n_steps);
    ST_REQUIRE(per_sample % CFG_VEC == 0, "%s: per_sample %ld is not a multiple of %d (16-byte vectors)", who, per_sample, CFG_VEC);
    ST_REQUIRE(per_sample <= PHILOX_MAX_PER_SAMPLE, "%s: per_sample %ld exceeds the generator's %ld values per sample", who,
               per_sample, PHILOX_MAX_PER_SAMPLE);
    ST_REQUIRE(cfg_blocks_per_sample(per_sample) <= 0x7fffffffL && batch <= 65535, "%s: grid too large", who);
    ST_REQUIRE((uintptr_t)latent % 16 == 0 && (uintptr_t)eps % 16 == 0 && (uintptr_t)next_in % 16 == 0 && (uintptr_t)history % 16 == 0,
               "%s: latent, eps, next_in and history must be 16-byte aligned", who);
    ST_REQUIRE((uintptr_t)seeds % 8 == 0, "%s: seeds must be 8-byte aligned", who);
    if (rescale) {
        const size_t need = st_cfg_step_workspace_bytes(batch, per_sample);
        ST_REQUIRE(workspace && workspace_bytes >= need, "%s: the rescale path needs a workspace of %zu bytes, got %zu", who,
                   need, workspace ? workspace_bytes : (size_t)0);
        ST_REQUIRE((uintptr_t)workspace % 16 == 0, "%s: workspace must be 16-byte aligned", who);
    }
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)workspace;
    if (dtype == ST_BF16)
        return sde_launch<bf16>(latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, seeds, batch, per_sample, n_steps, ws, st);
    if (dtype == ST_F16)
        return sde_launch<f16>(latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, seeds, batch, per_sample, n_steps, ws, st);
    if (dtype == ST_F32)
        return sde_launch<float>(latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, seeds, batch, per_sample, n_steps, ws, st);
    return st_fail("%s: unsupported dtype %d", who, dtype);
}

extern "C" int st_sde_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                           const float* guidance, const float* rescale, const int* step, const int* start,
                           const unsigned long long* seeds, int batch, long per_sample, int n_steps, int dtype, void* workspace,
                           size_t workspace_bytes, void* stream) {
    return sde_entry("sde_step", false, latent, eps, next_in, history, coef, in_scale, guidance, rescale, nullptr, step, start, seeds, batch,
                     per_sample, n_steps, dtype, workspace, workspace_bytes, stream);
}

// st_sde_step with the perturbed row block (st_pag_euler_step's comment states e); the noise stays keyed by the latent sample
extern "C" int st_pag_sde_step(float* latent, const void* eps, void* next_in, float* history, const float* coef, const float* in_scale,
                               const float* guidance, const float* rescale, const float* pag, const int* step, const int* start,
                               const unsigned long long* seeds, int batch, long per_sample, int n_steps, int dtype, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return sde_entry("pag_sde_step", true, latent, eps, next_in, history, coef, in_scale, guidance, rescale, pag, step, start, seeds, batch,
                     per_sample, n_steps, dtype, workspace, workspace_bytes, stream);
}

// out[b][4q .. 4q + 3] = the stream of seeds[b] at counter word ctr, one Philox call (16-byte store) per lane
__global__ __launch_bounds__(256) void philox_normal_kernel(float* __restrict__ out, const unsigned long long* __restrict__ seeds,
                                                            long per_sample, unsigned ctr) {
    const int b = blockIdx.y;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (4 * q >= per_sample) return;
    float z[4];
    philox_normal4(philox_key(seeds[b]), (unsigned)q, ctr, z);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = z[k];
    *reinterpret_cast<f32x4*>(out + (long)b * per_sample + 4 * q) = v;
}

extern "C" int st_philox_normal(float* out, const unsigned long long* seeds, int batch, long per_sample, unsigned counter, void* stream) {
    ST_REQUIRE(out && seeds, "philox_normal: null pointer");
    ST_REQUIRE(batch > 0 && per_sample > 0, "philox_normal: bad sizes (batch %d, per_sample %ld)", batch, per_sample);
    ST_REQUIRE(per_sample % 4 == 0, "philox_normal: per_sample %ld is not a multiple of 4 (one Philox call per 4 values)", per_sample);
    ST_REQUIRE(per_sample <= PHILOX_MAX_PER_SAMPLE, "philox_normal: per_sample %ld exceeds the generator's %ld values per sample",
               per_sample, PHILOX_MAX_PER_SAMPLE);
    ST_REQUIRE(batch <= 65535 && (per_sample / 4 + 255) / 256 <= 0x7fffffffL, "philox_normal: grid too large");
    ST_REQUIRE((uintptr_t)out % 16 == 0, "philox_normal: out must be 16-byte aligned");
    ST_REQUIRE((uintptr_t)seeds % 8 == 0, "philox_normal: seeds must be 8-byte aligned");
    const dim3 grid((unsigned)((per_sample / 4 + 255) / 256), (unsigned)batch);
    hipLaunchKernelGGL(philox_normal_kernel, grid, dim3(256), 0, (hipStream_t)stream, out, seeds, per_sample, counter);
    return st_check_launch("philox_normal");
}

__global__ void step_advance_kernel(int* step, int n_steps) {
    int s = *step + 1;
    *step = s >= n_steps ? 0 : s;
}

extern "C" int st_step_advance(int* step, int n_steps, void* stream) {
    ST_REQUIRE(step && n_steps > 0, "step_advance: bad arguments");
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, n_steps);
    return st_check_launch("step_advance");
}

// ---- sinusoidal features (reference unet_pt.py:17-36; its fuse_timesteps pass,
// optimizers/replace_timesteps.py:43-58, targets the same sub-graph) -----------
template <typename T>
__global__ void timestep_kernel(const float* __restrict__ t, long t_stride, const int* __restrict__ step,
                                T* __restrict__ out, int batch, int dim, const float* __restrict__ table, int table_rows) {
    const int half = dim / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * half) return;
    const int b = idx / half, j = idx - b * half;
    const int base = step ? *step : 0;
    const float tv = t[base + b * t_stride];
    // an integer timestep inside the host's table: the reference's own bits (the header says why)
    if (table && tv >= 0.f && tv < (float)table_rows && tv == floorf(tv)) {
        const float* row = table + (size_t)(int)tv * dim;
        out[(size_t)b * dim + j] = Elem<T>::from_f(row[j]);
        out[(size_t)b * dim + half + j] = Elem<T>::from_f(row[half + j]);
        return;
    }
    // same fp32 op order as the eager module: (-ln(1e4) * j) / half, exp, * t
    const float e = (-9.210340371976184f * (float)j) / (float)half;
    const float a = tv * expf(e);
    out[(size_t)b * dim + j] = Elem<T>::from_f(cosf(a));
    out[(size_t)b * dim + half + j] = Elem<T>::from_f(sinf(a));
}

extern "C" int st_timestep_features(const float* t, long t_stride, const int* step, void* out, int batch, int dim,
                                    int dtype, const float* table, int table_rows, void* stream) {
    ST_REQUIRE(t && out && batch > 0 && dim > 0 && dim % 2 == 0, "timestep_features: bad arguments");
    ST_REQUIRE(!table || table_rows > 0, "timestep_features: a table of %d rows", table_rows);
    if (!table) table_rows = 0;
    const int n = batch * (dim / 2);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16)
        hipLaunchKernelGGL(timestep_kernel<bf16>, dim3(cdiv(n, 256)), dim3(256), 0, st, t, t_stride, step, (bf16*)out, batch, dim, table, table_rows);
    else if (dtype == ST_F16)
        hipLaunchKernelGGL(timestep_kernel<f16>, dim3(cdiv(n, 256)), dim3(256), 0, st, t, t_stride, step, (f16*)out, batch, dim, table, table_rows);
    else if (dtype == ST_F32)
        hipLaunchKernelGGL(timestep_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, t, t_stride, step, (float*)out, batch, dim, table, table_rows);
    else
        return st_fail("timestep_features: unsupported dtype %d", dtype);
    return st_check_launch("timestep_features");
}

// ---- the reference's own timestep operator (optimizers/replace_timesteps.py:33-40 -> kernels/timestep.py:13-45):
// elementwise over an already broadcast tensor x of shape (..., half):
//   sin_out[i] = sin(x[i] * f_j), cos_out[i] = cos(x[i] * f_j),  j = i % half,  f_j = exp(-ln(1e4) * j / half)
__global__ void timestep_sincos_kernel(const float* __restrict__ x, float* __restrict__ s, float* __restrict__ c, long n, int half) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = (int)(i % half);
    const float e = (-9.210340371976184f * (float)j) / (float)half;
    const float a = x[i] * expf(e);
    s[i] = sinf(a);
    c[i] = cosf(a);
}

extern "C" int st_timestep_sincos(const float* x, float* sin_out, float* cos_out, long n, int half, void* stream) {
    ST_REQUIRE(x && sin_out && cos_out && n > 0 && half > 0, "timestep_sincos: bad arguments");
    hipLaunchKernelGGL(timestep_sincos_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, sin_out, cos_out, n, half);
    return st_check_launch("timestep_sincos");
}
