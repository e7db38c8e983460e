// Residual site of a T2I-Adapter (include/stabletriton_amd.h, st_residual_add): x[n, p, c] += s * f[n % f_rows, p, c], in place on a
// dense NHWC tensor, with s = scale_table[*step] read on the device, and - when the producer of x left GroupNorm partials beside
// it - those partials rewritten for the new values, so that the GroupNorm behind the site still needs no statistics pass.
//
// One launch.  The M = rows * HW pixel rows are cut into tiles of `trows` rows (the producer's own tile height when statistics are
// kept, RA_ROWS otherwise) and the channels into chunks of RA_CL 16-byte vectors: workgroup (tile, chunk) owns that rectangle of x
// and the (tile, channel) partials of its channels, so a 1280-channel site with eight tiles is 160 (bf16) or 320 (fp32)
// workgroups, not eight.  Thread (pl, cl) visits pixels pl, pl + 32, ... of its tile in order; the partial of a channel is that
// per-thread sum, a three-step butterfly over the pixel lanes of a wave, then the four waves in order: a fixed shape, no atomics, two
// launches give the same bits.  What is summed is the value as STORED (after the rounding to the element type), the convention
// of the GEMM / conv epilogues (epilogue.h: "what is stored").
//
// s == 0 is the "off" state: every workgroup reads s and leaves at once (uniform), nothing else is read and nothing is written, x and the partials
// keep the producer's bits.  The arithmetic is one fp32 fma per element and one rounding on output.
#include "common.h"

namespace {

constexpr int RA_THREADS = 256;
constexpr int RA_CL = 8;           // channel lanes: 8 x 16 bytes = one 128-byte line per pixel and chunk
constexpr int RA_PL = 32;          // pixel lanes
constexpr int RA_ROWS = 64;        // rows per tile when no statistics are kept

template <typename T>
__global__ __launch_bounds__(RA_THREADS) void residual_add_kernel(T* __restrict__ x, const T* __restrict__ f, const float* __restrict__ table,
                                                                  const int* __restrict__ step, int n_steps, long M, int HW, int C, int f_rows,
                                                                  int trows, int chunks, float* __restrict__ stats) {
    constexpr int VEC = Elem<T>::VEC, CW = RA_CL * VEC;
    __shared__ float red[4 * 2 * VEC * RA_CL];
    const int i = *step;
    const float s = table[i < 0 ? 0 : (i >= n_steps ? n_steps - 1 : i)];
    if (s == 0.0f) return;                                       // (uniform) off: the producer's bits stay
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = tid & (RA_CL - 1), pl = tid >> 3;
    const int chunk = blockIdx.x % chunks;
    const long t = blockIdx.x / chunks;
    const int c = chunk * CW + cl * VEC;
    const long m0 = t * trows;
    float acc[2 * VEC];
#pragma unroll
    for (int j = 0; j < 2 * VEC; ++j) acc[j] = 0.f;
    if (c < C) {                                                 // C % VEC == 0: the whole vector is inside
        const long n0 = m0 / HW;
        int p = (int)(m0 - n0 * HW) + pl;                        // pixel inside its image; fr: the feature row of that image
        int fr = (int)(n0 % f_rows);
        for (int q = pl; q < trows && m0 + q < M; q += RA_PL, p += RA_PL) {
            while (p >= HW) { p -= HW; fr = fr + 1 == f_rows ? 0 : fr + 1; }
            T* dst = x + (m0 + q) * C + c;
            const T* src = f + ((long)fr * HW + p) * C + c;
            Vec16<T> v = load16(dst);
            const Vec16<T> r = load16(src);
#pragma unroll
            for (int e = 0; e < VEC; ++e) v.set(e, fmaf(s, r.get(e), v.get(e)));
            store16(dst, v);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float w = v.get(e);                        // as stored
                acc[e] += w;
                acc[VEC + e] = fmaf(w, w, acc[VEC + e]);
            }
        }
    }
    if (stats == nullptr) return;                                // (uniform)
#pragma unroll
    for (int j = 0; j < 2 * VEC; ++j) {
        float v = acc[j];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < RA_CL) red[(wave * 2 * VEC + j) * RA_CL + cl] = v;
    }
    __syncthreads();
    if (tid < CW && chunk * CW + tid < C) {
        const int e = tid % VEC, l = tid / VEC;
        float a[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = k * VEC + e;
            a[k] = (red[(0 * 2 * VEC + j) * RA_CL + l] + red[(1 * 2 * VEC + j) * RA_CL + l]) +
                   (red[(2 * 2 * VEC + j) * RA_CL + l] + red[(3 * 2 * VEC + j) * RA_CL + l]);
        }
        reinterpret_cast<float2*>(stats)[t * C + chunk * CW + tid] = make_float2(a[0], a[1]);
    }
}

template <typename T>
int residual_add_launch(void* x, const void* f, long M, int HW, int C, int f_rows, const float* table, int n_steps, const int* step,
                        float* stats, int stat_rows, hipStream_t st) {
    constexpr int CW = RA_CL * Elem<T>::VEC;
    const int trows = stat_rows > 0 ? stat_rows : RA_ROWS;
    const int chunks = cdiv(C, CW);
    const long blocks = ((M + trows - 1) / trows) * chunks;
    ST_REQUIRE(blocks <= 0x7fffffffL, "residual_add: too many workgroups");
    hipLaunchKernelGGL(residual_add_kernel<T>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, (T*)x, (const T*)f, table, step, n_steps, M, HW, C,
                       f_rows, trows, chunks, stats);
    return st_check_launch("residual_add");
}

}  // namespace

extern "C" int st_residual_add(void* x, const void* f, int rows, int f_rows, long HW, int C, const float* scale_table, int n_steps,
                               const int* step, int dtype, float* stats, int stat_rows, int stat_tiles, void* stream) {
    ST_REQUIRE(x && f && scale_table && step, "residual_add: null pointer");
    ST_REQUIRE(rows > 0 && C > 0 && HW > 0 && HW <= 0x3fffffffL, "residual_add: bad shape rows=%d HW=%ld C=%d", rows, HW, C);
    ST_REQUIRE(f_rows > 0 && rows % f_rows == 0, "residual_add: f_rows=%d must divide rows=%d (1, the batch, or every row)", f_rows, rows);
    ST_REQUIRE(n_steps > 0, "residual_add: scale table of %d entries", n_steps);
    ST_REQUIRE(st_dtype_ok(dtype), "residual_add: unsupported dtype %d", dtype);
    const int vec = dtype == ST_F32 ? 4 : 8;
    {
        // the byte ranges [x, x + rows HW C) and [f, f + f_rows HW C) must be disjoint: a workgroup reads f where another writes x
        const uintptr_t esz = dtype == ST_F32 ? 4 : 2, per_row = (uintptr_t)HW * (uintptr_t)C * esz;
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)rows * per_row, f0 = (uintptr_t)f, f1 = f0 + (uintptr_t)f_rows * per_row;
        ST_REQUIRE(x1 <= f0 || f1 <= x0, "residual_add: x and f must not alias or overlap");
    }
    ST_REQUIRE(C % vec == 0, "residual_add: channel count %d must be a multiple of %d (16-byte vectors)", C, vec);
    ST_REQUIRE((((uintptr_t)x | (uintptr_t)f) & 15) == 0 && (((uintptr_t)scale_table | (uintptr_t)step) & 3) == 0,
               "residual_add: misaligned pointer");
    const long M = (long)rows * HW;
    ST_REQUIRE((stats != nullptr) == (stat_rows > 0) && stat_rows >= 0, "residual_add: statistics buffer and stat_rows=%d do not agree", stat_rows);
    if (stats != nullptr) {
        ST_REQUIRE(((uintptr_t)stats & 7) == 0, "residual_add: misaligned statistics buffer");
        ST_REQUIRE(HW % stat_rows == 0, "residual_add: %d rows per statistics partial do not divide the %ld pixels of an image", stat_rows, HW);
        ST_REQUIRE((long)stat_tiles == M / stat_rows, "residual_add: %d statistics tiles, %ld rows in tiles of %d make %ld", stat_tiles, M,
                   stat_rows, M / stat_rows);
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return residual_add_launch<bf16>(x, f, M, (int)HW, C, f_rows, scale_table, n_steps, step, stats, stat_rows, st);
    if (dtype == ST_F16) return residual_add_launch<f16>(x, f, M, (int)HW, C, f_rows, scale_table, n_steps, step, stats, stat_rows, st);
    return residual_add_launch<float>(x, f, M, (int)HW, C, f_rows, scale_table, n_steps, step, stats, stat_rows, st);
}
