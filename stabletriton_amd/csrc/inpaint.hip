// Masked inpainting (include/stabletriton_amd.h, st_inpaint_blend): the blend behind the sampler step.  latent, init, noise are
// (batch, HW, C) fp32 dense NHWC; next_in holds `blocks` row blocks of (batch, HW, C) in the UNet's type, row r * batch + b for sample
// b (the loop's x_step: every row block sees the same latent); mask is (mask_rows, HW) fp32, 1 = repaint, 0 = keep.
//
// With i = *step, s = sigma_next[i], sc = in_scale[min(i + 1, n_steps - 1)] and t = thr[i] (thr == NULL, or a NaN entry: no threshold),
// per pixel:  w = m without a threshold, else (m > t ? 1 : 0);  w = !(w < 1) ? 1 : max(w, 0)  (NaN and >= 1 repaint);
//   w == 1: nothing of the pixel is written, neither latent nor any next_in row;
//   else    known = fma(s, noise, init);  v = (w == 0) ? known : fma(w, latent - known, known);  latent = v;  every row block of
//           next_in = (T)(v * sc).
//
// One thread per pixel, 16-byte accesses of the fp32 tensors per four channels; step and the three table entries are
// workgroup-uniform (scalar reads, once per wave).  Memory-bound: no LDS, no atomics, every element written by one thread from
// values no other thread writes - two launches give the same bits.  All index arithmetic is 64-bit.
#include "common.h"

namespace {

constexpr int IP_THREADS = 256;

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef f32x4 type; };
template <> struct Vec4<bf16> { typedef bf16x4 type; };
template <> struct Vec4<f16> { typedef f16x4 type; };

template <typename T>
__global__ __launch_bounds__(IP_THREADS) void inpaint_blend_kernel(float* __restrict__ latent, T* __restrict__ next_in,
                                                                   const float* __restrict__ init, const float* __restrict__ noise,
                                                                   const float* __restrict__ mask, const float* __restrict__ thr,
                                                                   const float* __restrict__ sigma_next, const float* __restrict__ in_scale,
                                                                   const int* __restrict__ step, long pixels, long HW, int cv, int blocks,
                                                                   int per_sample_mask, int n_steps) {
    typedef typename Vec4<T>::type V;
    int i = *step;                                               // (uniform) clamped: no table is read outside its n_steps entries
    i = i < 0 ? 0 : (i >= n_steps ? n_steps - 1 : i);
    const float s = sigma_next[i];
    const float sc = in_scale[i + 1 < n_steps ? i + 1 : n_steps - 1];
    const float t = thr != nullptr ? thr[i] : __builtin_nanf("");
    const long p = (long)blockIdx.x * IP_THREADS + threadIdx.x;
    if (p >= pixels) return;
    const long q = per_sample_mask ? p : p % HW;
    const float m = mask[q];
    float w = (t != t) ? m : (m > t ? 1.0f : 0.0f);
    w = !(w < 1.0f) ? 1.0f : fmaxf(w, 0.0f);
    if (w == 1.0f) return;                                       // repaint: the sampler's values stay, nothing is written
    const long block_stride = pixels * cv * 4;                   // elements of one row block of next_in
    for (int c = 0; c < cv; ++c) {
        const long at = (p * cv + c) * 4;
        const f32x4 a = *reinterpret_cast<const f32x4*>(init + at);
        const f32x4 z = *reinterpret_cast<const f32x4*>(noise + at);
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaf(s, z[k], a[k]);
        if (w != 0.0f) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(latent + at);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaf(w, x[k] - v[k], v[k]);
        }
        *reinterpret_cast<f32x4*>(latent + at) = v;
        V o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (T)(v[k] * sc);
        for (int r = 0; r < blocks; ++r) *reinterpret_cast<V*>(next_in + r * block_stride + at) = o;
    }
}

bool ranges_overlap(uintptr_t a0, uintptr_t a_bytes, uintptr_t b0, uintptr_t b_bytes) { return a0 < b0 + b_bytes && b0 < a0 + a_bytes; }

}  // namespace

extern "C" int st_inpaint_blend(float* latent, void* next_in, const float* init, const float* noise, const float* mask,
                                const float* thr, const float* sigma_next, const float* in_scale, const int* step, int batch,
                                int blocks, long HW, int C, int mask_rows, int n_steps, int dtype, void* stream) {
    ST_REQUIRE(latent && next_in && init && noise && mask && sigma_next && in_scale && step, "inpaint_blend: null pointer");
    ST_REQUIRE(st_dtype_ok(dtype), "inpaint_blend: unsupported dtype %d", dtype);
    ST_REQUIRE(batch > 0 && HW > 0 && C > 0 && n_steps > 0, "inpaint_blend: bad shape batch=%d HW=%ld C=%d n_steps=%d", batch, HW, C, n_steps);
    ST_REQUIRE(C % 4 == 0, "inpaint_blend: channel count %d must be a multiple of 4 (one 4-element vector per access)", C);
    ST_REQUIRE(mask_rows == 1 || mask_rows == batch, "inpaint_blend: mask_rows=%d must be 1 or the batch %d", mask_rows, batch);
    ST_REQUIRE(blocks >= 1, "inpaint_blend: blocks=%d row blocks of next_in; at least 1", blocks);
    const long esz = dtype == ST_F32 ? 4 : 2;
    const long limit = 0x7fffffffffffL / (4L * C);               // bytes stay far inside 63 bits
    ST_REQUIRE(HW <= limit / batch / blocks, "inpaint_blend: tensor too large");
    const long pixels = (long)batch * HW;
    const long groups = (pixels + IP_THREADS - 1) / IP_THREADS;
    ST_REQUIRE(groups <= 0x7fffffffL, "inpaint_blend: tensor too large (too many workgroups)");
    const uintptr_t l0 = (uintptr_t)latent, i0 = (uintptr_t)init, z0 = (uintptr_t)noise, x0 = (uintptr_t)next_in, m0 = (uintptr_t)mask;
    ST_REQUIRE(((l0 | i0 | z0 | x0) & 15) == 0, "inpaint_blend: misaligned pointer (latent, init, noise and next_in: 16 bytes)");
    ST_REQUIRE(((m0 | (uintptr_t)thr | (uintptr_t)sigma_next | (uintptr_t)in_scale | (uintptr_t)step) & 3) == 0,
               "inpaint_blend: misaligned pointer (mask, tables and step: 4 bytes)");
    const uintptr_t lat_bytes = (uintptr_t)pixels * C * 4;
    ST_REQUIRE(!ranges_overlap(l0, lat_bytes, i0, lat_bytes), "inpaint_blend: latent must not overlap init");
    ST_REQUIRE(!ranges_overlap(l0, lat_bytes, z0, lat_bytes), "inpaint_blend: latent must not overlap noise");
    ST_REQUIRE(!ranges_overlap(l0, lat_bytes, m0, (uintptr_t)mask_rows * HW * 4), "inpaint_blend: latent must not overlap mask");
    ST_REQUIRE(!ranges_overlap(l0, lat_bytes, x0, (uintptr_t)blocks * pixels * C * esz), "inpaint_blend: latent must not overlap next_in");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)groups), block(IP_THREADS);
    const int cv = C / 4, psm = mask_rows != 1;
    if (dtype == ST_BF16)
        hipLaunchKernelGGL(inpaint_blend_kernel<bf16>, grid, block, 0, st, latent, (bf16*)next_in, init, noise, mask, thr, sigma_next, in_scale,
                           step, pixels, HW, cv, blocks, psm, n_steps);
    else if (dtype == ST_F16)
        hipLaunchKernelGGL(inpaint_blend_kernel<f16>, grid, block, 0, st, latent, (f16*)next_in, init, noise, mask, thr, sigma_next, in_scale,
                           step, pixels, HW, cv, blocks, psm, n_steps);
    else
        hipLaunchKernelGGL(inpaint_blend_kernel<float>, grid, block, 0, st, latent, (float*)next_in, init, noise, mask, thr, sigma_next, in_scale,
                           step, pixels, HW, cv, blocks, psm, n_steps);
    return st_check_launch("inpaint_blend");
}
