// Smoothed energy guidance (SEG; Hong 2024): the attention core whose tail batch entries run with Gaussian-blurred queries.
//
// In a perturbed self-attention site the projected queries of the perturbed batch entries (the LAST tail_count of the batch, as in
// pag.hip) are blurred over the token grid: q (n, T = h * w, C = H * D) is read as C planes of h x w, token t = y * w + x, and every
// plane becomes the separable convolution g (x) g of its reflect-padded self; keys and values stay as they are.  Channels are
// innermost, so this is an NHWC depthwise stencil: a lane owns one 16-byte vector of channels of one token and walks the taps.
//
// The blur parameters are a DEVICE row of ST_SEG_PARAM_WORDS floats, [mode, k, g_0 ... g_{k-1}], read when the kernels run: the
// same captured launches serve every sigma, and mode 1 (sigma = infinity) replaces every token of a plane by the plane's mean.  In
// mean mode the two passes are the same two loops with every tap 1 and a division at the end: the row pass sums the w values of a
// token's row in x order and divides by w, the column pass sums the h row means in y order and divides by h - a fixed order, no
// atomics, every token of a plane receives the same bits, and two runs repeat them.  What the row holds is not trusted: k is
// clamped to [1, min(h, w) + 1 - (min(h, w) mod 2)] and made odd on the device, so the reflected index stays inside the plane.
//
// Two forms:
//   plane (2 * T * VEC floats fit 160 KiB of LDS): one workgroup per (batch entry, 16-byte channel vector).  The plane is staged as
//     fp32 in LDS, the row pass goes LDS -> LDS, the column pass LDS -> out; q is read once and out written once.
//   general (any grid up to 128 x 128): two launches, the row pass q -> an fp32 workspace of n * T * C floats, the column pass
//     workspace -> out, one lane per (token, channel vector), taps read through the caches.
// Either way the intermediate between the two passes is fp32 and the only rounding to the element type is the output's.
//
// st_attention_seg is st_attention_pag's composition: st_attention, unmodified, on the leading B - tail_count entries, the blur
// of the tail's queries into a dense scratch, st_attention on the tail with q = scratch.  An armed split image (strict mode) is
// handed to the two attention launches for the rows of their sub-batches.
#include "common.h"

constexpr int SEG_THREADS = 256;
constexpr int SEG_MAX_SIDE = ST_SEG_MAX_SIDE;
constexpr size_t SEG_LDS_BUDGET = 160 * 1024;

struct SegRow {
    int mean;      // 1: every token becomes its plane's mean
    int k;         // odd tap count, k / 2 < min(h, w)
};

__device__ __forceinline__ SegRow seg_row(const float* __restrict__ params, int h, int w) {
    const int m = h < w ? h : w;
    const int kmax = m + 1 - (m & 1);
    int k = (int)params[1];
    k = k < 1 ? 1 : (k > kmax ? kmax : k);
    k -= 1 - (k & 1);
    SegRow r;
    r.mean = params[0] != 0.0f;
    r.k = k;
    return r;
}

// index of tap i (offset i - r) around position p on an axis of `len` samples, reflected without repeating the edge; r < len
__device__ __forceinline__ int seg_reflect(int p, int i, int r, int len) {
    int j = p + i - r;
    j = j < 0 ? -j : j;
    return j >= len ? 2 * (len - 1) - j : j;
}

// One axis of the blur at one position: VEC channels from `src` (fp32), whose sample s of this line is at src + s * stride; channels
// [4 j, 4 j + 4) of a sample are `group` floats after channels [4 (j - 1), 4 j) (4: one contiguous vector; the LDS planes keep the
// groups apart so that neighbouring lanes read neighbouring 16-byte slots).
template <int VEC>
__device__ __forceinline__ void seg_line_f32(const float* __restrict__ src, long stride, long group, int p, int len, SegRow row,
                                             const float* __restrict__ taps, float (&acc)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
    if (row.mean) {
        for (int s = 0; s < len; ++s) {
#pragma unroll
            for (int e = 0; e < VEC; e += 4) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(src + (long)s * stride + (e >> 2) * group);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[e + c] += x[c];
            }
        }
        const float inv = (float)len;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = acc[e] / inv;
        return;
    }
    const int r = row.k >> 1;
    for (int i = 0; i < row.k; ++i) {
        const float g = taps[i];
        const int s = seg_reflect(p, i, r, len);
#pragma unroll
        for (int e = 0; e < VEC; e += 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(src + (long)s * stride + (e >> 2) * group);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[e + c] = fmaf(g, x[c], acc[e + c]);
        }
    }
}

// The same from a line of T elements (the row pass of the general form reads q itself).
template <typename T>
__device__ __forceinline__ void seg_line_elem(const T* __restrict__ src, long stride, int p, int len, SegRow row,
                                              const float* __restrict__ taps, float (&acc)[Elem<T>::VEC]) {
    constexpr int VEC = Elem<T>::VEC;
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
    if (row.mean) {
        for (int s = 0; s < len; ++s) {
            const Vec16<T> x = load16(src + (long)s * stride);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] += x.get(e);
        }
        const float inv = (float)len;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = acc[e] / inv;
        return;
    }
    const int r = row.k >> 1;
    for (int i = 0; i < row.k; ++i) {
        const float g = taps[i];
        const Vec16<T> x = load16(src + (long)seg_reflect(p, i, r, len) * stride);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = fmaf(g, x.get(e), acc[e]);
    }
}

template <int VEC>
__device__ __forceinline__ void seg_store_f32(float* __restrict__ dst, long group, const float (&acc)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; e += 4) {
        f32x4 x;
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = acc[e + c];
        *reinterpret_cast<f32x4*>(dst + (e >> 2) * group) = x;
    }
}

// ---- plane form: block = (batch entry, channel vector); LDS = two fp32 planes of h * w * VEC floats --------------------------
template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void seg_blur_plane_kernel(const T* __restrict__ q, T* __restrict__ out,
                                                                      const float* __restrict__ params, int h, int w,
                                                                      int vecs_per_row, long ldq, long ldo) {
    constexpr int VEC = Elem<T>::VEC;
    extern __shared__ __attribute__((aligned(16))) float seg_lds[];
    const int tokens = h * w;
    float* a = seg_lds;                                    // [channel group of 4][token][4]
    float* b = seg_lds + (size_t)tokens * VEC;
    const long group = (long)tokens * 4;
    // blocks that share an XCD (ids congruent mod 8) take neighbouring channel vectors: they read the same cache lines of q
    int id = blockIdx.x;
    if ((gridDim.x & 7) == 0) id = (id & 7) * (gridDim.x >> 3) + (id >> 3);
    const int n = id / vecs_per_row, cv = id - n * vecs_per_row;
    const T* src = q + (long)n * tokens * ldq + cv * VEC;
    T* dst = out + (long)n * tokens * ldo + cv * VEC;
    const SegRow row = seg_row(params, h, w);
    const float* taps = params + 2;
    for (int t = threadIdx.x; t < tokens; t += SEG_THREADS) {
        const Vec16<T> x = load16(src + (long)t * ldq);
        float f[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] = x.get(e);
        seg_store_f32<VEC>(a + (size_t)t * 4, group, f);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tokens; t += SEG_THREADS) {      // rows: a -> b
        const int y = t / w, x = t - y * w;
        float acc[VEC];
        seg_line_f32<VEC>(a + (size_t)y * w * 4, 4, group, x, w, row, taps, acc);
        seg_store_f32<VEC>(b + (size_t)t * 4, group, acc);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < tokens; t += SEG_THREADS) {      // columns: b -> out
        const int y = t / w, x = t - y * w;
        float acc[VEC];
        seg_line_f32<VEC>(b + (size_t)x * 4, (long)w * 4, group, y, h, row, taps, acc);
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) o.set(e, acc[e]);
        store16(dst + (long)t * ldo, o);
    }
}

// ---- general form: lane = (token row of the n * T, channel vector) -----------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void seg_blur_rows_kernel(const T* __restrict__ q, float* __restrict__ mid,
                                                                     const float* __restrict__ params, long n_vec, int h, int w,
                                                                     int vecs_per_row, long ldq) {
    constexpr int VEC = Elem<T>::VEC;
    const long g = (long)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (g >= n_vec) return;
    const long r = g / vecs_per_row;                       // token row of the whole (n * T)
    const int col = (int)(g - r * vecs_per_row) * VEC;
    const int x = (int)(r % w);
    const SegRow row = seg_row(params, h, w);
    float acc[VEC];
    seg_line_elem<T>(q + (r - x) * ldq + col, ldq, x, w, row, params + 2, acc);
    seg_store_f32<VEC>(mid + r * ((long)vecs_per_row * VEC) + col, 4, acc);
}

template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void seg_blur_cols_kernel(const float* __restrict__ mid, T* __restrict__ out,
                                                                     const float* __restrict__ params, long n_vec, int h, int w,
                                                                     int vecs_per_row, long ldo) {
    constexpr int VEC = Elem<T>::VEC;
    const long g = (long)blockIdx.x * SEG_THREADS + threadIdx.x;
    if (g >= n_vec) return;
    const long r = g / vecs_per_row;
    const int col = (int)(g - r * vecs_per_row) * VEC;
    const long cols = (long)vecs_per_row * VEC;
    const int x = (int)(r % w);
    const int y = (int)((r / w) % h);
    const SegRow row = seg_row(params, h, w);
    float acc[VEC];
    seg_line_f32<VEC>(mid + (r - (long)y * w) * cols + col, (long)w * cols, 4, y, h, row, params + 2, acc);
    Vec16<T> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o.set(e, acc[e]);
    store16(out + r * ldo + col, o);
}

static inline size_t seg_plane_lds(int h, int w, int dtype) {
    return (size_t)2 * h * w * (st_dtype_is16(dtype) ? 8 : 4) * sizeof(float);
}

template <typename T>
static int seg_blur_launch(const void* q, void* out, const float* params, int n, int h, int w, int C, long ldq, long ldo, int dtype,
                           void* workspace, hipStream_t st) {
    const int vecs_per_row = C / Elem<T>::VEC;
    const size_t lds = seg_plane_lds(h, w, dtype);
    if (lds <= SEG_LDS_BUDGET) {
        static unsigned long long raised = 0;
        ensure_dynamic_lds(seg_blur_plane_kernel<T>, lds, &raised);
        const long blocks = (long)n * vecs_per_row;
        ST_REQUIRE(blocks < (1L << 31), "seg_blur: too many blocks");
        hipLaunchKernelGGL((seg_blur_plane_kernel<T>), dim3((unsigned)blocks), dim3(SEG_THREADS), lds, st, (const T*)q, (T*)out, params,
                           h, w, vecs_per_row, ldq, ldo);
        return st_check_launch("seg_blur (plane)");
    }
    const long n_vec = (long)n * h * w * vecs_per_row;
    const long blocks = (n_vec + SEG_THREADS - 1) / SEG_THREADS;
    ST_REQUIRE(blocks < (1L << 31), "seg_blur: too many blocks");
    hipLaunchKernelGGL((seg_blur_rows_kernel<T>), dim3((unsigned)blocks), dim3(SEG_THREADS), 0, st, (const T*)q, (float*)workspace, params,
                       n_vec, h, w, vecs_per_row, ldq);
    if (int e = st_check_launch("seg_blur (rows)")) return e;
    hipLaunchKernelGGL((seg_blur_cols_kernel<T>), dim3((unsigned)blocks), dim3(SEG_THREADS), 0, st, (const float*)workspace, (T*)out, params,
                       n_vec, h, w, vecs_per_row, ldo);
    return st_check_launch("seg_blur (columns)");
}

extern "C" size_t st_seg_blur_workspace_bytes(int n, int h, int w, int C, int dtype) {
    if (n <= 0 || h <= 0 || w <= 0 || C <= 0 || !st_dtype_ok(dtype)) return 0;
    if (seg_plane_lds(h, w, dtype) <= SEG_LDS_BUDGET) return 0;
    return (size_t)n * h * w * C * sizeof(float);
}

extern "C" int st_seg_blur(const void* q, void* out, const float* params, int n, int h, int w, int C, long ldq, long ldo, int dtype,
                           void* workspace, size_t workspace_bytes, void* stream) {
    ST_REQUIRE(q && out && params, "seg_blur: null pointer");
    ST_REQUIRE(st_dtype_ok(dtype), "seg_blur: unsupported dtype %d", dtype);
    ST_REQUIRE(n > 0 && h > 0 && w > 0 && C > 0, "seg_blur: bad shape n=%d h=%d w=%d C=%d", n, h, w, C);
    ST_REQUIRE(h <= SEG_MAX_SIDE && w <= SEG_MAX_SIDE, "seg_blur: token grid %d x %d is larger than %d x %d", h, w, SEG_MAX_SIDE, SEG_MAX_SIDE);
    const int vec = st_dtype_is16(dtype) ? 8 : 4;
    ST_REQUIRE(C % vec == 0 && ldq % vec == 0 && ldo % vec == 0, "seg_blur: row length and strides must be 16-byte multiples");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)out) % 16 == 0 && (uintptr_t)params % 4 == 0, "seg_blur: pointers must be 16-byte aligned");
    ST_REQUIRE(ldq >= C && ldo >= C, "seg_blur: row strides shorter than a row of C = %d values", C);
    const size_t need = st_seg_blur_workspace_bytes(n, h, w, C, dtype);
    ST_REQUIRE(need == 0 || (workspace && (uintptr_t)workspace % 16 == 0 && workspace_bytes >= need),
               "seg_blur: a %d x %d grid needs a 16-byte aligned fp32 workspace of %zu bytes (st_seg_blur_workspace_bytes)", h, w, need);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return seg_blur_launch<bf16>(q, out, params, n, h, w, C, ldq, ldo, dtype, workspace, st);
    if (dtype == ST_F16) return seg_blur_launch<f16>(q, out, params, n, h, w, C, ldq, ldo, dtype, workspace, st);
    return seg_blur_launch<float>(q, out, params, n, h, w, C, ldq, ldo, dtype, workspace, st);
}

extern "C" int st_attention_seg(const void* q, const void* k, const void* v, void* out, void* scratch, int B, int T, int S, int H, int D,
                                long ldq, long ldk, long ldv, long ldo, float scale, int dtype, int tail_count, int h, int w,
                                const float* params, void* workspace, size_t workspace_bytes, void* stream) {
    ST_REQUIRE(q && k && v && out, "attention_seg: null pointer");
    ST_REQUIRE(B > 0 && T > 0 && S > 0 && H > 0, "attention_seg: bad shape B=%d T=%d S=%d H=%d", B, T, S, H);
    ST_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, "attention_seg: head_dim %d not supported (16, 32, 64, 128)", D);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_seg: too many heads/batches for one launch");
    ST_REQUIRE(st_dtype_ok(dtype), "attention_seg: unsupported dtype %d", dtype);
    ST_REQUIRE(tail_count >= 0 && tail_count <= B, "attention_seg: tail_count %d outside [0, B = %d]", tail_count, B);
    ST_REQUIRE(tail_count == 0 || T == S, "attention_seg: the blurred tail needs self-attention shapes (T == S), got T=%d S=%d", T, S);
    ST_REQUIRE(tail_count == 0 || (h > 0 && w > 0 && (long)h * w == T), "attention_seg: the token grid %d x %d does not hold T = %d tokens", h, w, T);
    ST_REQUIRE(tail_count == 0 || (h <= SEG_MAX_SIDE && w <= SEG_MAX_SIDE), "attention_seg: token grid %d x %d is larger than %d x %d", h, w,
               SEG_MAX_SIDE, SEG_MAX_SIDE);
    ST_REQUIRE(tail_count == 0 || (scratch && params), "attention_seg: the blurred tail needs scratch and the parameter row");
    const int vec = st_dtype_is16(dtype) ? 8 : 4;
    const size_t esz = st_dtype_is16(dtype) ? 2 : 4;
    ST_REQUIRE(ldq % vec == 0 && ldk % vec == 0 && ldv % vec == 0 && ldo % vec == 0, "attention_seg: strides must be 16-byte multiples");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)scratch) % 16 == 0,
               "attention_seg: pointers must be 16-byte aligned");
    const int cols = H * D;
    ST_REQUIRE(ldq >= cols && ldo >= cols, "attention_seg: row strides shorter than a row of H * D = %d values", cols);
    void* image = nullptr;
    if (int e = st_take_split_arm("attention_seg", (long)B * T, cols, dtype == ST_F32, &image)) return e;
    const int lead = B - tail_count;
    if (lead > 0) {
        if (image)
            if (int e = st_arm_split_output(image, (long)lead * T, cols)) return e;
        if (int e = st_attention(q, k, v, out, lead, T, S, H, D, ldq, ldk, ldv, ldo, scale, dtype, stream)) return e;
    }
    if (tail_count == 0) return 0;
    const size_t first = (size_t)lead * T;                 // (T == S: one row offset for q, k, v and out)
    const char* qt = (const char*)q + first * (size_t)ldq * esz;
    const char* kt = (const char*)k + first * (size_t)ldk * esz;
    const char* vt = (const char*)v + first * (size_t)ldv * esz;
    char* ot = (char*)out + first * (size_t)ldo * esz;
    if (int e = st_seg_blur(qt, scratch, params, tail_count, h, w, cols, ldq, cols, dtype, workspace, workspace_bytes, stream)) return e;
    if (image)
        if (int e = st_arm_split_output((char*)image + first * (size_t)cols * 4, (long)tail_count * T, cols)) return e;
    return st_attention(scratch, kt, vt, ot, tail_count, T, S, H, D, cols, ldk, ldv, ldo, scale, dtype, stream);
}
