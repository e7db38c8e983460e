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
//
// st_residual_add_grouped (ControlNet's skip and middle residuals) runs up to 16 such sites in one grid, the concatenation of the
// sites' own grids, each under s_k = scale * weight_k; the workgroup body is one device function, so a site gets the same bits
// from either entry point.
#include "common.h"

namespace {

constexpr int RA_THREADS = 256;
constexpr int RA_CL = 8;           // channel lanes: 8 x 16 bytes = one 128-byte line per pixel and chunk
constexpr int RA_PL = 32;          // pixel lanes
constexpr int RA_ROWS = 64;        // rows per tile when no statistics are kept

// The rectangle of one workgroup: `block` = tile * chunks + chunk inside its site.  Shared by the single-site kernel and the grouped
// one, so both store the same bits.  `red` is the workgroup's 4 * 2 * VEC * RA_CL floats of LDS.
template <typename T>
__device__ __forceinline__ void residual_add_body(T* __restrict__ x, const T* __restrict__ f, float s, long M, int HW, int C, int f_rows,
                                                  int trows, int chunks, float* __restrict__ stats, unsigned block, float* red) {
    constexpr int VEC = Elem<T>::VEC, CW = RA_CL * VEC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = tid & (RA_CL - 1), pl = tid >> 3;
    const int chunk = block % chunks;
    const long t = block / chunks;
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
__global__ __launch_bounds__(RA_THREADS) void residual_add_kernel(T* __restrict__ x, const T* __restrict__ f, const float* __restrict__ table,
                                                                  const int* __restrict__ step, int n_steps, long M, int HW, int C, int f_rows,
                                                                  int trows, int chunks, float* __restrict__ stats) {
    __shared__ float red[4 * 2 * Elem<T>::VEC * RA_CL];
    const int i = *step;
    const float s = table[i < 0 ? 0 : (i >= n_steps ? n_steps - 1 : i)];
    if (s == 0.0f) return;                                       // (uniform) off: the producer's bits stay
    residual_add_body<T>(x, f, s, M, HW, C, f_rows, trows, chunks, stats, blockIdx.x, red);
}

// ---- the grouped launch (st_residual_add_grouped): up to RA_MAX_SITES sites in ONE grid, the concatenation of their own grids.
// The descriptors travel by value in the kernel arguments (a captured launch keeps them).  A workgroup finds its site with a
// uniform scan over the sites' first workgroups: every index below is a compile-time constant after unrolling, every compare is
// on blockIdx.x, so the chosen descriptor sits in scalar registers and nothing of the array goes to scratch.
constexpr int RA_MAX_SITES = 16;

struct RaSite {
    void* x;
    const void* f;
    float* stats;
    long M;
    int HW, C, f_rows, trows, chunks;
    unsigned first;                                              // the site's first workgroup in the grid; unused entries: 0xffffffff
};
struct RaGroup { RaSite site[RA_MAX_SITES]; };

template <typename T>
__global__ __launch_bounds__(RA_THREADS) void residual_add_grouped_kernel(const RaGroup g, const float* __restrict__ weights,
                                                                          const float* __restrict__ table, const int* __restrict__ step,
                                                                          int n_steps) {
    __shared__ float red[4 * 2 * Elem<T>::VEC * RA_CL];
    const unsigned b = blockIdx.x;
    RaSite d = g.site[0];
    int k = 0;
#pragma unroll
    for (int j = 1; j < RA_MAX_SITES; ++j)
        if (b >= g.site[j].first) { d = g.site[j]; k = j; }       // (uniform; `first` ascends over the used entries)
    const int i = *step;
    float s = table[i < 0 ? 0 : (i >= n_steps ? n_steps - 1 : i)];
    if (weights != nullptr) s = s * weights[k];                  // one fp32 product: s_k = fl32(scale * weight_k)
    if (s == 0.0f) return;                                       // (uniform) this site is off: its producer's bits stay
    residual_add_body<T>((T*)d.x, (const T*)d.f, s, d.M, d.HW, d.C, d.f_rows, d.trows, d.chunks, d.stats, b - d.first, red);
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

template <typename T>
int residual_add_grouped_launch(const st_residual_site* sites, int n_sites, const float* weights, const float* table, int n_steps,
                                const int* step, hipStream_t st) {
    constexpr int CW = RA_CL * Elem<T>::VEC;
    RaGroup g;
    long blocks = 0;
    for (int k = 0; k < RA_MAX_SITES; ++k) {
        RaSite& d = g.site[k];
        if (k >= n_sites) {
            d = RaSite{nullptr, nullptr, nullptr, 0, 1, 0, 1, 1, 1, 0xffffffffu};
            continue;
        }
        const st_residual_site& h = sites[k];
        d.x = h.x; d.f = h.r; d.stats = h.stats;
        d.M = (long)h.rows * h.HW;
        d.HW = (int)h.HW; d.C = h.C; d.f_rows = h.r_rows;
        d.trows = h.stat_rows > 0 ? h.stat_rows : RA_ROWS;          // the per-site grid of residual_add_launch
        d.chunks = cdiv(h.C, CW);
        d.first = (unsigned)blocks;
        blocks += ((d.M + d.trows - 1) / d.trows) * d.chunks;
        ST_REQUIRE(blocks <= 0x7fffffffL, "residual_add_grouped: too many workgroups");
    }
    hipLaunchKernelGGL(residual_add_grouped_kernel<T>, dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, g, weights, table, step, n_steps);
    return st_check_launch("residual_add_grouped");
}

// What both entry points ask of one site, before any launch.  `who` names the entry point (and, grouped, the site).
int residual_site_check(const char* who, const void* x, const void* f, int rows, int f_rows, long HW, int C, int dtype, const float* stats,
                        int stat_rows, int stat_tiles) {
    ST_REQUIRE(x && f, "%s: null pointer", who);
    ST_REQUIRE(rows > 0 && C > 0 && HW > 0 && HW <= 0x3fffffffL, "%s: bad shape rows=%d HW=%ld C=%d", who, rows, HW, C);
    ST_REQUIRE(f_rows > 0 && rows % f_rows == 0, "%s: f_rows=%d must divide rows=%d (1, the batch, or every row)", who, f_rows, rows);
    const int vec = dtype == ST_F32 ? 4 : 8;
    {
        // the byte ranges [x, x + rows HW C) and [f, f + f_rows HW C) must be disjoint: a workgroup reads f where another writes x
        const uintptr_t esz = dtype == ST_F32 ? 4 : 2, per_row = (uintptr_t)HW * (uintptr_t)C * esz;
        const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)rows * per_row, f0 = (uintptr_t)f, f1 = f0 + (uintptr_t)f_rows * per_row;
        ST_REQUIRE(x1 <= f0 || f1 <= x0, "%s: x and f must not alias or overlap", who);
    }
    ST_REQUIRE(C % vec == 0, "%s: channel count %d must be a multiple of %d (16-byte vectors)", who, C, vec);
    ST_REQUIRE((((uintptr_t)x | (uintptr_t)f) & 15) == 0, "%s: misaligned pointer", who);
    const long M = (long)rows * HW;
    ST_REQUIRE((stats != nullptr) == (stat_rows > 0) && stat_rows >= 0, "%s: statistics buffer and stat_rows=%d do not agree", who, stat_rows);
    if (stats != nullptr) {
        ST_REQUIRE(((uintptr_t)stats & 7) == 0, "%s: misaligned statistics buffer", who);
        ST_REQUIRE(HW % stat_rows == 0, "%s: %d rows per statistics partial do not divide the %ld pixels of an image", who, stat_rows, HW);
        ST_REQUIRE((long)stat_tiles == M / stat_rows, "%s: %d statistics tiles, %ld rows in tiles of %d make %ld", who, stat_tiles, M,
                   stat_rows, M / stat_rows);
    }
    return 0;
}

}  // namespace

extern "C" int st_residual_add(void* x, const void* f, int rows, int f_rows, long HW, int C, const float* scale_table, int n_steps,
                               const int* step, int dtype, float* stats, int stat_rows, int stat_tiles, void* stream) {
    ST_REQUIRE(scale_table && step, "residual_add: null pointer");
    ST_REQUIRE(n_steps > 0, "residual_add: scale table of %d entries", n_steps);
    ST_REQUIRE(st_dtype_ok(dtype), "residual_add: unsupported dtype %d", dtype);
    ST_REQUIRE((((uintptr_t)scale_table | (uintptr_t)step) & 3) == 0, "residual_add: misaligned pointer");
    if (int rc = residual_site_check("residual_add", x, f, rows, f_rows, HW, C, dtype, stats, stat_rows, stat_tiles)) return rc;
    const long M = (long)rows * HW;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return residual_add_launch<bf16>(x, f, M, (int)HW, C, f_rows, scale_table, n_steps, step, stats, stat_rows, st);
    if (dtype == ST_F16) return residual_add_launch<f16>(x, f, M, (int)HW, C, f_rows, scale_table, n_steps, step, stats, stat_rows, st);
    return residual_add_launch<float>(x, f, M, (int)HW, C, f_rows, scale_table, n_steps, step, stats, stat_rows, st);
}

extern "C" int st_residual_add_grouped(const st_residual_site* sites, int n_sites, const float* site_weights, const float* scale_table,
                                       int n_steps, const int* step, int dtype, void* stream) {
    ST_REQUIRE(n_sites >= 1 && n_sites <= RA_MAX_SITES, "residual_add_grouped: %d sites; one launch takes 1..%d", n_sites, RA_MAX_SITES);
    ST_REQUIRE(sites && scale_table && step, "residual_add_grouped: null pointer");
    ST_REQUIRE(n_steps > 0, "residual_add_grouped: scale table of %d entries", n_steps);
    ST_REQUIRE(st_dtype_ok(dtype), "residual_add_grouped: unsupported dtype %d", dtype);
    ST_REQUIRE((((uintptr_t)scale_table | (uintptr_t)step | (uintptr_t)site_weights) & 3) == 0, "residual_add_grouped: misaligned pointer");
    // every byte range of the call: x written, r read, stats rewritten, by workgroups of one grid in no order
    struct Range { uintptr_t lo, hi; int site; const char* what; } ranges[3 * RA_MAX_SITES];
    int n_ranges = 0;
    const uintptr_t esz = dtype == ST_F32 ? 4 : 2;
    for (int k = 0; k < n_sites; ++k) {
        const st_residual_site& h = sites[k];
        char who[48];
        snprintf(who, sizeof who, "residual_add_grouped: site %d", k);
        if (int rc = residual_site_check(who, h.x, h.r, h.rows, h.r_rows, h.HW, h.C, dtype, h.stats, h.stat_rows, h.stat_tiles)) return rc;
        const uintptr_t per_row = (uintptr_t)h.HW * (uintptr_t)h.C * esz;
        ranges[n_ranges++] = Range{(uintptr_t)h.x, (uintptr_t)h.x + (uintptr_t)h.rows * per_row, k, "x"};
        ranges[n_ranges++] = Range{(uintptr_t)h.r, (uintptr_t)h.r + (uintptr_t)h.r_rows * per_row, k, "r"};
        if (h.stats != nullptr)
            ranges[n_ranges++] = Range{(uintptr_t)h.stats, (uintptr_t)h.stats + (uintptr_t)h.stat_tiles * (uintptr_t)h.C * 8, k, "stats"};
    }
    for (int a = 0; a < n_ranges; ++a)
        for (int b = a + 1; b < n_ranges; ++b)
            ST_REQUIRE(ranges[a].hi <= ranges[b].lo || ranges[b].hi <= ranges[a].lo,
                       "residual_add_grouped: %s of site %d and %s of site %d overlap; every x, r and stats of one call must be disjoint",
                       ranges[a].what, ranges[a].site, ranges[b].what, ranges[b].site);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return residual_add_grouped_launch<bf16>(sites, n_sites, site_weights, scale_table, n_steps, step, st);
    if (dtype == ST_F16) return residual_add_grouped_launch<f16>(sites, n_sites, site_weights, scale_table, n_steps, step, st);
    return residual_add_grouped_launch<float>(sites, n_sites, site_weights, scale_table, n_steps, step, st);
}

