// Self-attention guidance (SAG; Hong et al., "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance", 2023;
// ComfyUI's nodes_sag.py restated for an eps-predicting loop): the input of the step's SECOND UNet call (header: st_sag_degrade).
// Per pixel of the fp32 latent x, with e the negative block's prediction, i = clamp(*step), sigma = sigmas[i]:
//   x0    = x - sigma e                                       the predicted clean latent
//   mask  = A[b, floor(y th / lh), floor(x tw / lw)] > thr    A: the site's column sums (attention_colsum.hip) on its (th, tw) grid,
//                                                             nearest-upsampled to the latent
//   blur  = g (x) g of x0 per channel, nine taps g_d = exp(-(d / s_b)^2 / 2) / sum, d = -4..4, reflect padding (edge not repeated)
//   out   = ((mask ? blur : x0) + sigma e) * in_scale[i]      rounded once to the model dtype
// thr and s_b are a DEVICE row of two floats, read when the kernel runs: changing them never needs a new capture.
//
// One launch.  A block of 256 threads owns a 16 x 16 pixel tile of one image: it stages x0 of the tile and a 4-pixel halo (24 x 24
// pixels x 4 channels, one float4 each, the halo reflect-indexed at the image border) in LDS, runs the horizontal pass into a second
// LDS plane (24 rows x 16 columns), then every thread finishes its own pixel: vertical pass, select, re-noise, scale, store, and the
// mask it used.  NHWC with C = 4: a pixel is one 16-byte load of the latent and one 8-byte (16-bit types) load of eps.
#include "common.h"

namespace {

constexpr int SAG_TILE = 16, SAG_HALO = 4, SAG_SPAN = SAG_TILE + 2 * SAG_HALO, SAG_TAPS = 2 * SAG_HALO + 1, SAG_THREADS = SAG_TILE * SAG_TILE;

template <typename T>
__device__ __forceinline__ f32x4 sag_load4(const T* p) {
    if constexpr (sizeof(T) == 4) {
        return *reinterpret_cast<const f32x4*>(p);
    } else {
        const typename V16<T>::x4 v = *reinterpret_cast<const typename V16<T>::x4*>(p);
        return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
}
template <typename T>
__device__ __forceinline__ void sag_store4(T* p, const f32x4& v) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<f32x4*>(p) = v;
    } else {
        typename V16<T>::x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = (T)v[c];
        *reinterpret_cast<typename V16<T>::x4*>(p) = o;
    }
}
// reflect without repeating the edge; one reflection covers the halo of every pixel inside the image (n > SAG_HALO), the clamp only
// keeps the addresses of a partial tile's unused cells inside the image
__device__ __forceinline__ int sag_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}
__device__ __forceinline__ f32x4 sag_fma(float a, const f32x4& b, const f32x4& c) {
    return f32x4{fmaf(a, b[0], c[0]), fmaf(a, b[1], c[1]), fmaf(a, b[2], c[2]), fmaf(a, b[3], c[3])};
}

template <typename T>
__global__ __launch_bounds__(SAG_THREADS) void sag_degrade_kernel(const float* __restrict__ latent, const T* __restrict__ eps,
                                                                  const float* __restrict__ amap, const float* __restrict__ sigmas,
                                                                  const float* __restrict__ in_scale, const int* __restrict__ step,
                                                                  const float* __restrict__ params, T* __restrict__ out,
                                                                  float* __restrict__ mask, int lh, int lw, int th, int tw, int n_steps) {
    __shared__ f32x4 x0s[SAG_SPAN][SAG_SPAN];
    __shared__ f32x4 hs[SAG_SPAN][SAG_TILE];
    __shared__ float taps[SAG_TAPS];
    const int tid = threadIdx.x, b = blockIdx.z, ty0 = blockIdx.y * SAG_TILE, tx0 = blockIdx.x * SAG_TILE;
    const int i = min(max(*step, 0), n_steps - 1);
    const float sigma = sigmas[i], sc = in_scale[i], thr = params[0], sb = params[1];
    const size_t image = (size_t)b * lh * lw;
    if (tid < SAG_TAPS) {                        // every one of the nine threads forms the same sum, d ascending
        float w[SAG_TAPS], total = 0.f;
#pragma unroll
        for (int d = 0; d < SAG_TAPS; ++d) {
            const float z = (float)(d - SAG_HALO) / sb;
            w[d] = expf(-0.5f * z * z);
            total += w[d];
        }
        taps[tid] = w[tid] / total;
    }
    for (int p = tid; p < SAG_SPAN * SAG_SPAN; p += SAG_THREADS) {
        const int yy = p / SAG_SPAN, xx = p - yy * SAG_SPAN;
        const size_t px = image + (size_t)sag_reflect(ty0 - SAG_HALO + yy, lh) * lw + sag_reflect(tx0 - SAG_HALO + xx, lw);
        const f32x4 x = *reinterpret_cast<const f32x4*>(latent + 4 * px);
        x0s[yy][xx] = sag_fma(-sigma, sag_load4(eps + 4 * px), x);
    }
    __syncthreads();
    for (int p = tid; p < SAG_SPAN * SAG_TILE; p += SAG_THREADS) {
        const int yy = p / SAG_TILE, xx = p - yy * SAG_TILE;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < SAG_TAPS; ++d) a = sag_fma(taps[d], x0s[yy][xx + d], a);
        hs[yy][xx] = a;
    }
    __syncthreads();
    const int ly = tid / SAG_TILE, lx = tid - ly * SAG_TILE, gy = ty0 + ly, gx = tx0 + lx;
    if (gy >= lh || gx >= lw) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < SAG_TAPS; ++d) v = sag_fma(taps[d], hs[ly + d][lx], v);
    const int cy = (int)(((long)gy * th) / lh), cx = (int)(((long)gx * tw) / lw);
    const bool on = amap[(size_t)b * th * tw + (size_t)cy * tw + cx] > thr;
    if (!on) v = x0s[ly + SAG_HALO][lx + SAG_HALO];
    const size_t px = image + (size_t)gy * lw + gx;
    v = sag_fma(sigma, sag_load4(eps + 4 * px), v);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] *= sc;
    sag_store4(out + 4 * px, v);
    mask[px] = on ? 1.f : 0.f;
}

template <typename T>
int sag_launch(const float* latent, const void* eps, const float* amap, const float* sigmas, const float* in_scale, const int* step,
               const float* params, void* out, float* mask, int B, int lh, int lw, int th, int tw, int n_steps, hipStream_t st) {
    const dim3 grid((unsigned)((lw + SAG_TILE - 1) / SAG_TILE), (unsigned)((lh + SAG_TILE - 1) / SAG_TILE), (unsigned)B);
    hipLaunchKernelGGL(sag_degrade_kernel<T>, grid, dim3(SAG_THREADS), 0, st, latent, (const T*)eps, amap, sigmas, in_scale, step, params,
                       (T*)out, mask, lh, lw, th, tw, n_steps);
    return st_check_launch("sag_degrade");
}

}  // namespace

extern "C" int st_sag_degrade(const float* latent, const void* eps_neg, const float* amap, const float* sigmas, const float* in_scale,
                              const int* step, const float* params, void* out, float* mask, int B, int lh, int lw, int th, int tw,
                              int n_steps, int dtype, void* stream) {
    ST_REQUIRE(latent && eps_neg && amap && sigmas && in_scale && step && params && out && mask, "sag_degrade: null pointer");
    ST_REQUIRE(B > 0 && B <= 65535 && n_steps > 0, "sag_degrade: bad sizes (B %d, n_steps %d)", B, n_steps);
    ST_REQUIRE(lh > SAG_HALO && lw > SAG_HALO && lh <= (1 << 20) && lw <= (1 << 20), "sag_degrade: a latent of %d x %d (each side more than %d, the blur's reach)",
               lh, lw, SAG_HALO);
    ST_REQUIRE(th > 0 && tw > 0 && th <= lh && tw <= lw, "sag_degrade: a map grid of %d x %d for a latent of %d x %d", th, tw, lh, lw);
    ST_REQUIRE(st_dtype_ok(dtype), "sag_degrade: unsupported dtype %d", dtype);
    ST_REQUIRE((uintptr_t)latent % 16 == 0 && (uintptr_t)eps_neg % 16 == 0 && (uintptr_t)out % 16 == 0,
               "sag_degrade: latent, eps_neg and out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return sag_launch<bf16>(latent, eps_neg, amap, sigmas, in_scale, step, params, out, mask, B, lh, lw, th, tw, n_steps, st);
    if (dtype == ST_F16) return sag_launch<f16>(latent, eps_neg, amap, sigmas, in_scale, step, params, out, mask, B, lh, lw, th, tw, n_steps, st);
    return sag_launch<float>(latent, eps_neg, amap, sigmas, in_scale, step, params, out, mask, B, lh, lw, th, tw, n_steps, st);
}
