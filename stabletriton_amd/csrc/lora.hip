// LoRA merge: ONE grouped launch rebuilds every adapted weight from its base snapshot (include/stabletriton_amd.h, st_lora_merge).
//
//   W_t[n][k] = round_to_dtype( fp32(Base_t[n][k]) + sum_j scale[slot_j] * sum_r Up_tj[n][r] * DownT_tj[k][r] )
//
// The work list is flat: workgroup b reads tiles[b] = (target, tile index inside the target), the target's row of the
// descriptor table, and owns one 64 (n) x 128 (k) tile of that weight.  Every output element is produced by exactly one lane
// from a fixed sequence of operations (no atomics, no split over the rank), so two launches give the same bits.  A weight
// is rebuilt from its base, never updated: with every scale that touches it zero the base's bits are copied through.
//
// 16-bit models run on the matrix pipe (v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation), as the product D = DownT . Up^T:
// the MFMA's row index is k and its column index is n, so a lane ends up with values that are consecutive in k, the
// contiguous direction of W.  The rows of a PAIR of MFMA tiles are interleaved - row i of tile t is k = 8 (i >> 2) + 4 t +
// (i & 3) of the pair's 32 columns - so that lane group g = lane >> 4 holds k = 8 g .. 8 g + 7 in the two accumulators: one
// 16-byte base read and one 16-byte store per lane and pair.  A workgroup stages the factor rows of its tile in LDS first: they
// are contiguous in memory, so the copy is coalesced, where operand reads straight from memory take one cache line per lane
// (measured on SDXL-base at rank 128: 5.4 ms against this form's figure in DESIGN.md).  The ranks are zero-padded to the
// MFMA's k = 32 by the host, which is exact and leaves no remainder path.  fp32 models use plain fp32 FMAs, ranks padded to 4.
#include "common.h"

namespace {

constexpr int LORA_THREADS = 256;
constexpr int LORA_TN = ST_LORA_TILE_N;      // 64: four waves of 16 rows
constexpr int LORA_TK = ST_LORA_TILE_K;      // 128: four pairs of MFMA tiles
constexpr int TGT_WORDS = 6, SEG_WORDS = 4;

struct Target {
    char* w;
    const char* base;
    int N, K, seg0, nseg;
};

__device__ __forceinline__ Target load_target(const long long* __restrict__ targets, int t) {
    const long long* d = targets + (long)t * TGT_WORDS;
    Target r;
    r.w = (char*)d[0];
    r.base = (const char*)d[1];
    r.N = (int)d[2];
    r.K = (int)d[3];
    r.seg0 = (int)d[4];
    r.nseg = (int)d[5];
    return r;
}

// base + delta for VEC consecutive k of row n, rounded once; 16-byte accesses when the target allows them (K a multiple of
// VEC and both images 16-byte aligned), elementwise with a bound check per value otherwise.  `merged` false: the base's bits.
template <typename T>
__device__ __forceinline__ void finish_row(const Target& tg, int n, int k, const float* delta, bool merged, bool vec) {
    constexpr int VEC = Elem<T>::VEC;
    if (n >= tg.N || k >= tg.K) return;
    const long at = (long)n * tg.K + k;
    const T* b = reinterpret_cast<const T*>(tg.base) + at;
    T* w = reinterpret_cast<T*>(tg.w) + at;
    if (vec) {                                   // k + VEC <= K: k and K are multiples of VEC
        Vec16<T> v = load16(b);
        if (merged) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) v.set(i, v.get(i) + delta[i]);
        }
        store16(w, v);
    } else {
        for (int i = 0; i < VEC && k + i < tg.K; ++i)
            w[i] = merged ? Elem<T>::from_f(Elem<T>::to_f(b[i]) + delta[i]) : b[i];
    }
}

template <typename T> struct Mfma16;
template <> struct Mfma16<bf16> {
    static __device__ __forceinline__ f32x4 run(const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma16<f16> {
    static __device__ __forceinline__ f32x4 run(const f16x8& a, const f16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// LDS images of one segment's factor tiles.  Rows are padded by 16 bytes: (rp + 8) * 2 bytes = 4 (rp / 8 + 1) banks, an odd
// multiple of 4 for every rp that is a multiple of 32, so 16 consecutive rows read as 16-byte chunks cover all 64 banks
// once.  The images are sized by the launch's largest padded rank (15 KiB at rank <= 32, 51 KiB at 128), which sets how many
// workgroups share a CU.  The DownT rows are stored in MFMA order - tile row k = 32 p + 8 a + 4 h + b lives in
// image row 32 p + 16 h + 4 a + b - so the 16 lanes of an operand read take 16 consecutive image rows.
static inline int lora_lds_row(int max_rank) { return (max_rank + 8) * 2; }      // bytes

template <typename T>
__global__ __launch_bounds__(LORA_THREADS) void lora_merge16_kernel(const long long* __restrict__ targets, const long long* __restrict__ segments,
                                                                   const int* __restrict__ tiles, const float* __restrict__ scales, int lds_row) {
    typedef typename V16<T>::x8 frag;
    extern __shared__ __attribute__((aligned(16))) char lds_down[];
    char* lds_up = lds_down + LORA_TK * lds_row;
    const int t = tiles[2 * blockIdx.x], tile = tiles[2 * blockIdx.x + 1];
    const Target tg = load_target(targets, t);
    const int tiles_k = (tg.K + LORA_TK - 1) / LORA_TK;
    const int nt = (tile / tiles_k) * LORA_TN, k0 = (tile % tiles_k) * LORA_TK;
    const int wave = threadIdx.x >> 6, n0 = nt + wave * 16;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const bool vec = tg.K % 8 == 0 && (((uintptr_t)tg.w | (uintptr_t)tg.base) & 15) == 0;
    const int rows_k = min(LORA_TK, tg.K - k0), rows_n = min(LORA_TN, tg.N - nt);      // rows of the factors this tile may read
    // the base's 16-byte vectors are requested first: they come from HBM while the factors are staged and multiplied
    Vec16<T> basev[4];
    if (vec && n0 + c < tg.N) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (k0 + 32 * p + 8 * g < tg.K)
                basev[p] = load16(reinterpret_cast<const T*>(tg.base) + (long)(n0 + c) * tg.K + k0 + 32 * p + 8 * g);
    }
    f32x4 sum[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sum[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool merged = false;
    for (int j = 0; j < tg.nseg; ++j) {
        const long long* sg = segments + (long)(tg.seg0 + j) * SEG_WORDS;
        const float s = scales[(int)sg[3]];
        if (s == 0.f) continue;                                 // (uniform) an adapter at scale 0 contributes nothing, whatever it holds
        const T* up = (const T*)sg[0] + (long)nt * (int)sg[2];
        const T* down_t = (const T*)sg[1] + (long)k0 * (int)sg[2];
        const int rp = (int)sg[2], chunks = rp >> 3;             // 16-byte chunks per factor row
        if ((rp + 8) * 2 > lds_row) continue;                   // (uniform; a table that breaks the max_rank contract: no image overrun)
        if (merged) __syncthreads();                            // the previous segment's images have been read
        merged = true;
        // both tiles are contiguous in memory (whole rows of row-major factors): coalesced 16-byte copies.  Rows past the
        // weight's edge are not read; what the image holds there only reaches outputs that are never stored.
        for (int q = threadIdx.x; q < rows_k * chunks; q += LORA_THREADS) {
            const int row = q / chunks, col = q - row * chunks;
            const int img = (row & ~31) + 16 * ((row >> 2) & 1) + 4 * ((row >> 3) & 3) + (row & 3);
            *reinterpret_cast<frag*>(lds_down + img * lds_row + col * 16) = *reinterpret_cast<const frag*>(down_t + (long)q * 8);
        }
        for (int q = threadIdx.x; q < rows_n * chunks; q += LORA_THREADS) {
            const int row = q / chunks, col = q - row * chunks;
            *reinterpret_cast<frag*>(lds_up + row * lds_row + col * 16) = *reinterpret_cast<const frag*>(up + (long)q * 8);
        }
        __syncthreads();
        f32x4 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < rp; r0 += 32) {
            const int col = (r0 + 8 * g) * 2;
            const frag b = *reinterpret_cast<const frag*>(lds_up + (wave * 16 + c) * lds_row + col);
#pragma unroll
            for (int i = 0; i < 8; ++i) {                       // i = 2 p + h: image rows 16 i .. 16 i + 15
                const frag a = *reinterpret_cast<const frag*>(lds_down + (16 * i + c) * lds_row + col);
                acc[i] = Mfma16<T>::run(a, b, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[i][e] = fmaf(s, acc[i][e], sum[i][e]);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float delta[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            delta[e] = sum[2 * p][e];
            delta[4 + e] = sum[2 * p + 1][e];
        }
        const int n = n0 + c, k = k0 + 32 * p + 8 * g;
        if (!vec) {
            finish_row<T>(tg, n, k, delta, merged, false);
        } else if (n < tg.N && k < tg.K) {                      // k + 8 <= K: k and K are multiples of 8
            if (merged) {
#pragma unroll
                for (int e = 0; e < 8; ++e) basev[p].set(e, basev[p].get(e) + delta[e]);
            }
            store16(reinterpret_cast<T*>(tg.w) + (long)n * tg.K + k, basev[p]);
        }
    }
}

// fp32: thread (rg, cg) owns rows 8 rg .. 8 rg + 7 and columns 4 cg .. 4 cg + 3 of the tile; factors are read four ranks at a time
__global__ __launch_bounds__(LORA_THREADS) void lora_merge32_kernel(const long long* __restrict__ targets, const long long* __restrict__ segments,
                                                                   const int* __restrict__ tiles, const float* __restrict__ scales) {
    const int t = tiles[2 * blockIdx.x], tile = tiles[2 * blockIdx.x + 1];
    const Target tg = load_target(targets, t);
    const int tiles_k = (tg.K + LORA_TK - 1) / LORA_TK;
    const int n0 = (tile / tiles_k) * LORA_TN + (threadIdx.x >> 5) * 8, k0 = (tile % tiles_k) * LORA_TK + (threadIdx.x & 31) * 4;
    const bool vec = tg.K % 4 == 0 && (((uintptr_t)tg.w | (uintptr_t)tg.base) & 15) == 0;
    float sum[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[i][e] = 0.f;
    bool merged = false;
    for (int j = 0; j < tg.nseg; ++j) {
        const long long* sg = segments + (long)(tg.seg0 + j) * SEG_WORDS;
        const float s = scales[(int)sg[3]];
        if (s == 0.f) continue;
        merged = true;
        const float* up = (const float*)sg[0];
        const float* down_t = (const float*)sg[1];
        const int rp = (int)sg[2];
        float acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
        for (int r0 = 0; r0 < rp; r0 += 4) {
            f32x4 d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                d[e] = *reinterpret_cast<const f32x4*>(down_t + (long)min(k0 + e, tg.K - 1) * rp + r0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(up + (long)min(n0 + i, tg.N - 1) * rp + r0);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][e] = fmaf(u[q], d[e][q], acc[i][e]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[i][e] = fmaf(s, acc[i][e], sum[i][e]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) finish_row<float>(tg, n0 + i, k0, sum[i], merged, vec);
}

}  // namespace

extern "C" int st_lora_merge(const long long* targets, int n_targets, const long long* segments, int n_segments, int max_rank,
                             const int* tiles, long n_tiles, const float* scales, int n_scales, int dtype, void* stream) {
    ST_REQUIRE(targets && tiles && scales && (segments || n_segments == 0), "lora_merge: null pointer");
    ST_REQUIRE(n_targets > 0 && n_segments >= 0 && n_scales > 0, "lora_merge: bad sizes (targets %d, segments %d, scales %d)",
               n_targets, n_segments, n_scales);      // (a target without segments is restored to its base)
    ST_REQUIRE(n_tiles > 0 && n_tiles <= 0x7fffffffL, "lora_merge: %ld tiles (a launch takes 1 .. 2^31 - 1)", n_tiles);
    ST_REQUIRE((uintptr_t)targets % 8 == 0 && (uintptr_t)segments % 8 == 0 && (uintptr_t)tiles % 4 == 0 && (uintptr_t)scales % 4 == 0,
               "lora_merge: misaligned table");
    ST_REQUIRE(max_rank >= 0 && max_rank <= ST_LORA_MAX_RANK && (n_segments == 0 || max_rank > 0),
               "lora_merge: max_rank %d (the largest padded rank of the segments, 1 .. %d)", max_rank, (int)ST_LORA_MAX_RANK);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_tiles), block(LORA_THREADS);
    const int lds_row = lora_lds_row((max_rank + 31) / 32 * 32);
    const size_t lds = (size_t)(LORA_TK + LORA_TN) * lds_row;
    if (dtype == ST_BF16)
        hipLaunchKernelGGL(lora_merge16_kernel<bf16>, grid, block, lds, st, targets, segments, tiles, scales, lds_row);
    else if (dtype == ST_F16)
        hipLaunchKernelGGL(lora_merge16_kernel<f16>, grid, block, lds, st, targets, segments, tiles, scales, lds_row);
    else if (dtype == ST_F32)
        hipLaunchKernelGGL(lora_merge32_kernel, grid, block, 0, st, targets, segments, tiles, scales);
    else
        return st_fail("lora_merge: unsupported dtype %d", dtype);
    return st_check_launch("lora_merge");
}
