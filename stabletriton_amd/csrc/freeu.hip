// FreeU at a decoder skip connection (include/stabletriton_amd.h, st_freeu): the running activation h (N, H, W, C_h) gets half of
// its channels rescaled, the skip tensor r (N, H, W, C_s) gets its four lowest spatial frequencies scaled by s.  NHWC, two launches.
//
// The published filter - fftshift(fftn(x)), the box [H/2-1 : H/2+1, W/2-1 : W/2+1] times s, the inverse transform's real part -
// touches the bins (u, v) in {0, -1} x {0, -1} only, so per (n, c) plane it is a rank-7 update, with t = 2 pi y / H, p = 2 pi x / W:
//
//   x'[y,x] = x[y,x] + (s - 1) / (H W) * (m0 + m1 cos t + m2 sin t + m3 cos p + m4 sin p + m5 cos(t + p) + m6 sin(t + p))
//   m_k     = sum_{y,x} x[y,x] * basis_k[y,x],      basis = (1, cos t, sin t, cos p, sin p, cos(t + p), sin(t + p))
//
// Launch 1 (freeu_reduce): blocks [0, nb_s) each own 256 pixels x one chunk of 8 16-byte channel vectors of r and write the seven
// moments of their channels over their pixels as one partial row; the remaining blocks write the channel mean of every pixel of h
// (read by version 2 only; they leave at once otherwise).  Launch 2 (freeu_apply): every block first adds the partial rows of its
// channels in tile order (and, for version 2, takes min / max of its sample's mean map), then writes h' or r' and the
// GroupNorm partials (sum, sum of squares per tile and channel, of the values as stored) of what it wrote.
//
// Every sum has a fixed shape - 8 pixels per thread in order, a three-step butterfly over the pixel lanes of a wave, the four
// waves, the tiles in order - and nothing is accumulated with atomics: two launches give the same bits.  The trigonometry is
// evaluated once per pixel and workgroup (sincospif on 2 y / H and 2 x / W, the sum angle by the addition formulas) into LDS.
// b, s and the version are read from the device row `params` = (b1, s1, b2, s2, version): a captured graph sees new values.
// s == 1 adds nothing and b == 1 multiplies by nothing (not "+ 0" / "* 1"): neutral parameters copy the bits through.
#include "common.h"

namespace {

constexpr int FU_THREADS = 256;
constexpr int FU_TILE = 256;      // pixels per moment tile (and the largest apply tile)
constexpr int FU_CL = 8;          // channel lanes: 8 x 16 bytes = one 128-byte line per pixel and chunk
constexpr int FU_PL = 32;         // pixel lanes: thread (pl, cl) visits pixels pl, pl + 32, ... of its tile
constexpr int FU_K = 7;           // moments per plane

struct FuShape { int N, Ch, Cs, H, W, HW, tiles_m, chunks_h, chunks_s; };

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// cos / sin of t = 2 pi y / H, p = 2 pi x / W and t + p for the `count` pixels from p0 on (one pixel per thread) -> bas[6][FU_TILE]
__device__ __forceinline__ void stage_basis(float (*bas)[FU_TILE], int p0, int count, const FuShape& g) {
    const int i = threadIdx.x;
    if (i >= FU_TILE) return;
    float ct = 0.f, st = 0.f, cp = 0.f, sp = 0.f;
    const int p = p0 + i;
    if (i < count && p < g.HW) {
        const int y = p / g.W, x = p - y * g.W;
        sincospif(2.0f * (float)y / (float)g.H, &st, &ct);
        sincospif(2.0f * (float)x / (float)g.W, &sp, &cp);
    }
    bas[0][i] = ct; bas[1][i] = st; bas[2][i] = cp; bas[3][i] = sp;
    bas[4][i] = ct * cp - st * sp;
    bas[5][i] = st * cp + ct * sp;
}

// sum over the 32 pixel lanes of acc[0 .. n) (each thread's values for its channel lane): butterfly inside the wave, then the
// four waves through red[4][n][FU_CL]; afterwards thread (wave 0 .. 3 irrelevant) reads red and every (j, cl) total is
// (red[0] + red[1]) + (red[2] + red[3]).
template <int NV>
__device__ __forceinline__ void reduce_pixel_lanes(float* acc, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = threadIdx.x & (FU_CL - 1);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        float v = acc[j];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < FU_CL) red[(wave * NV + j) * FU_CL + cl] = v;
    }
    __syncthreads();
}
template <int NV>
__device__ __forceinline__ float reduced(const float* red, int j, int cl) {
    return (red[(0 * NV + j) * FU_CL + cl] + red[(1 * NV + j) * FU_CL + cl]) + (red[(2 * NV + j) * FU_CL + cl] + red[(3 * NV + j) * FU_CL + cl]);
}

template <typename T>
__global__ __launch_bounds__(FU_THREADS) void freeu_reduce(const T* __restrict__ h, const T* __restrict__ r, float* __restrict__ part,
                                                           float* __restrict__ mu, const float* __restrict__ params, int slot,
                                                           FuShape g, int nb_s) {
    constexpr int VEC = Elem<T>::VEC, CW = FU_CL * VEC;
    __shared__ float bas[6][FU_TILE];
    __shared__ float red[4 * FU_K * VEC * FU_CL];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= nb_s) {
        // ---- channel mean of every pixel of h (version 2): one wave per pixel, lanes over 16-byte vectors, butterfly sum
        if (params[4] != 2.0f || params[2 * slot] == 1.0f) return;
        const int wave = tid >> 6, lane = tid & 63, nvec = g.Ch / VEC;
        const long rows = (long)g.N * g.HW, stride = (long)(gridDim.x - nb_s) * 4;
        for (long row = (long)(blockIdx.x - nb_s) * 4 + wave; row < rows; row += stride) {
            const T* src = h + row * g.Ch;
            float s = 0.f;
            for (int v = lane; v < nvec; v += 64) {
                const Vec16<T> x = load16(src + v * VEC);
#pragma unroll
                for (int e = 0; e < VEC; ++e) s += x.get(e);
            }
            s = wave_sum(s);
            if (lane == 0) mu[row] = s / (float)g.Ch;
        }
        return;
    }
    // ---- seven moments of one chunk of skip channels over one tile of pixels
    if (params[2 * slot + 1] == 1.0f) return;                    // (uniform) the filter is off: nobody reads the partials
    const int chunk = blockIdx.x % g.chunks_s, t = (blockIdx.x / g.chunks_s) % g.tiles_m, n = blockIdx.x / (g.chunks_s * g.tiles_m);
    const int p0 = t * FU_TILE;
    stage_basis(bas, p0, FU_TILE, g);
    __syncthreads();
    const int cl = tid & (FU_CL - 1), pl = tid >> 3;
    const int c = chunk * CW + cl * VEC;
    float acc[FU_K * VEC];
#pragma unroll
    for (int j = 0; j < FU_K * VEC; ++j) acc[j] = 0.f;
    if (c < g.Cs) {                                              // Cs % VEC == 0: the whole vector is inside
        const T* src = r + ((long)n * g.HW + p0) * g.Cs + c;
#pragma unroll
        for (int i = 0; i < FU_TILE / FU_PL; ++i) {
            const int q = pl + FU_PL * i;
            if (p0 + q < g.HW) {
                const Vec16<T> x = load16(src + (long)q * g.Cs);
                float b[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) b[k] = bas[k][q];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float v = x.get(e);
                    acc[e] += v;
#pragma unroll
                    for (int k = 0; k < 6; ++k) acc[(k + 1) * VEC + e] = fmaf(v, b[k], acc[(k + 1) * VEC + e]);
                }
            }
        }
    }
    reduce_pixel_lanes<FU_K * VEC>(acc, red);
    float* dst = part + ((long)n * g.tiles_m + t) * FU_K * g.Cs;
    for (int q = tid; q < FU_K * CW; q += FU_THREADS) {
        const int k = q / CW, cc = q - k * CW;
        if (chunk * CW + cc < g.Cs) dst[(long)k * g.Cs + chunk * CW + cc] = reduced<FU_K * VEC>(red, k * VEC + (cc % VEC), cc / VEC);
    }
}

template <typename T>
__global__ __launch_bounds__(FU_THREADS) void freeu_apply(const T* __restrict__ h, const T* __restrict__ r, T* __restrict__ h_out,
                                                          T* __restrict__ r_out, const float* __restrict__ part, const float* __restrict__ mu,
                                                          const float* __restrict__ params, int slot, FuShape g, int trows, int tiles_a,
                                                          int nb_s, float* __restrict__ stats_h, float* __restrict__ stats_s) {
    constexpr int VEC = Elem<T>::VEC, CW = FU_CL * VEC;
    __shared__ float bas[6][FU_TILE];            // skip blocks: the basis; h blocks: bas[0] = the per-pixel factor
    __shared__ float fin[FU_K][CW];              // finished moments of this block's channels, times (s - 1) / (H W)
    __shared__ float red[4 * 2 * VEC * FU_CL];
    __shared__ float mm[2][4];
    const int tid = threadIdx.x, cl = tid & (FU_CL - 1), pl = tid >> 3;
    const bool is_skip = (int)blockIdx.x < nb_s;
    const int bid = is_skip ? blockIdx.x : blockIdx.x - nb_s;
    const int chunks = is_skip ? g.chunks_s : g.chunks_h, C = is_skip ? g.Cs : g.Ch;
    const int chunk = bid % chunks, t = (bid / chunks) % tiles_a, n = bid / (chunks * tiles_a);
    const int p0 = t * trows;
    const int c = chunk * CW + cl * VEC;
    const float bq = params[2 * slot], sq = params[2 * slot + 1];
    const bool v2 = params[4] == 2.0f;
    const bool active = is_skip ? sq != 1.0f : bq != 1.0f;      // (uniform)
    float m[FU_K * VEC];
    if (is_skip) {
        if (active) {
            const float gain = (sq - 1.0f) / ((float)g.H * (float)g.W);
            const float* src = part + (long)n * g.tiles_m * FU_K * g.Cs;
            for (int q = tid; q < FU_K * CW; q += FU_THREADS) {
                const int k = q / CW, cc = q - k * CW;
                float s = 0.f;
                if (chunk * CW + cc < g.Cs)
                    for (int tm = 0; tm < g.tiles_m; ++tm) s += src[((long)tm * FU_K + k) * g.Cs + chunk * CW + cc];
                fin[k][cc] = s * gain;
            }
            stage_basis(bas, p0, trows, g);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < FU_K; ++k)
#pragma unroll
                for (int e = 0; e < VEC; ++e) m[k * VEC + e] = fin[k][cl * VEC + e];
        }
    } else if (active && v2) {
        // version 2: factor (b - 1) * (mu - min) / (max - min) + 1 per pixel, min / max over this sample's map (0 where it is flat)
        const float* map = mu + (long)n * g.HW;
        float lo = INFINITY, hi = -INFINITY;
        for (int p = tid; p < g.HW; p += FU_THREADS) {
            const float v = map[p];
            lo = fminf(lo, v); hi = fmaxf(hi, v);
        }
        lo = wave_min(lo); hi = wave_max(hi);
        if ((tid & 63) == 0) { mm[0][tid >> 6] = lo; mm[1][tid >> 6] = hi; }
        __syncthreads();
        lo = fminf(fminf(mm[0][0], mm[0][1]), fminf(mm[0][2], mm[0][3]));
        hi = fmaxf(fmaxf(mm[1][0], mm[1][1]), fmaxf(mm[1][2], mm[1][3]));
        if (tid < trows && p0 + tid < g.HW) {
            const float hat = hi > lo ? (map[p0 + tid] - lo) / (hi - lo) : 0.f;
            bas[0][tid] = (bq - 1.0f) * hat + 1.0f;
        }
        __syncthreads();
    }
    float acc[2 * VEC];
#pragma unroll
    for (int j = 0; j < 2 * VEC; ++j) acc[j] = 0.f;
    if (c < C) {
        const long at = ((long)n * g.HW + p0) * C + c;
        const T* src = (is_skip ? r : h) + at;
        T* dst = (is_skip ? r_out : h_out) + at;
        const int half = g.Ch / 2;
#pragma unroll
        for (int i = 0; i < FU_TILE / FU_PL; ++i) {
            const int q = pl + FU_PL * i;
            if (q < trows && p0 + q < g.HW) {
                Vec16<T> x = load16(src + (long)q * C);
                if (active) {
                    if (is_skip) {
                        float b[6];
#pragma unroll
                        for (int k = 0; k < 6; ++k) b[k] = bas[k][q];
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            float d = m[e];
#pragma unroll
                            for (int k = 0; k < 6; ++k) d = fmaf(m[(k + 1) * VEC + e], b[k], d);
                            x.set(e, x.get(e) + d);
                        }
                    } else {
                        const float f = v2 ? bas[0][q] : bq;
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
                            if (c + e < half) x.set(e, x.get(e) * f);
                    }
                }
                store16(dst + (long)q * C, x);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float v = x.get(e);                 // as stored
                    acc[e] += v;
                    acc[VEC + e] = fmaf(v, v, acc[VEC + e]);
                }
            }
        }
    }
    float* stats = is_skip ? stats_s : stats_h;
    if (stats == nullptr) return;                              // (uniform)
    reduce_pixel_lanes<2 * VEC>(acc, red);
    if (tid < CW && chunk * CW + tid < C) {
        const int e = tid % VEC, l = tid / VEC;
        float2* dst = reinterpret_cast<float2*>(stats) + ((long)n * tiles_a + t) * C + chunk * CW + tid;
        *dst = make_float2(reduced<2 * VEC>(red, e, l), reduced<2 * VEC>(red, VEC + e, l));
    }
}

int stat_rows_for(long HW) {
    long a = HW, b = FU_TILE;
    while (b) { const long c = a % b; a = b; b = c; }
    return a >= 64 ? (int)a : 0;
}

size_t mu_bytes(int N, long HW) { return ((size_t)N * HW * sizeof(float) + 15) & ~(size_t)15; }

template <typename T>
int freeu_launch(const void* h, const void* skip, void* h_out, void* skip_out, FuShape g, const float* params, int slot, float* stats_h,
                 float* stats_skip, int stat_rows, void* workspace, hipStream_t st) {
    constexpr int CW = FU_CL * Elem<T>::VEC;
    g.chunks_h = cdiv(g.Ch, CW);
    g.chunks_s = cdiv(g.Cs, CW);
    float* mu = (float*)workspace;
    float* part = (float*)((char*)workspace + mu_bytes(g.N, g.HW));
    const long nb_s = (long)g.N * g.tiles_m * g.chunks_s;
    const long nb_mean = cdiv((long)g.N * g.HW, 16);                  // four pixels per wave
    const int trows = stat_rows > 0 ? stat_rows : FU_TILE, tiles_a = cdiv(g.HW, trows);
    const long nb_sa = (long)g.N * tiles_a * g.chunks_s, nb_ha = (long)g.N * tiles_a * g.chunks_h;
    ST_REQUIRE(nb_s + nb_mean <= 0x7fffffffL && nb_sa + nb_ha <= 0x7fffffffL, "freeu: too many workgroups");
    hipLaunchKernelGGL(freeu_reduce<T>, dim3((unsigned)(nb_s + nb_mean)), dim3(FU_THREADS), 0, st, (const T*)h, (const T*)skip, part, mu,
                       params, slot, g, (int)nb_s);
    hipLaunchKernelGGL(freeu_apply<T>, dim3((unsigned)(nb_sa + nb_ha)), dim3(FU_THREADS), 0, st, (const T*)h, (const T*)skip, (T*)h_out,
                       (T*)skip_out, part, mu, params, slot, g, trows, tiles_a, (int)nb_sa, stats_h, stats_skip);
    return st_check_launch("freeu");
}

}  // namespace

extern "C" int st_freeu_stat_rows(long HW) { return HW > 0 ? stat_rows_for(HW) : 0; }

extern "C" size_t st_freeu_workspace_bytes(int N, int C_skip, long HW) {
    if (N <= 0 || C_skip <= 0 || HW <= 0) return 0;
    return mu_bytes(N, HW) + (size_t)N * cdiv(HW, FU_TILE) * FU_K * C_skip * sizeof(float);
}

extern "C" int st_freeu(const void* h, const void* skip, void* h_out, void* skip_out, int N, int C_h, int C_skip, int H, int W,
                        const float* params, int slot, int dtype, float* stats_h, float* stats_skip, int stat_rows,
                        void* workspace, size_t workspace_bytes, void* stream) {
    ST_REQUIRE(h && skip && h_out && skip_out && params && workspace, "freeu: null pointer");
    ST_REQUIRE(h != h_out && skip != skip_out, "freeu: the outputs are written out of place");
    ST_REQUIRE(N > 0 && C_h > 0 && C_skip > 0, "freeu: bad shape N=%d C_h=%d C_skip=%d", N, C_h, C_skip);
    ST_REQUIRE(H >= 2 && W >= 2, "freeu: H=%d W=%d (the published filter's box is empty for a side of 1)", H, W);
    ST_REQUIRE((long)H * W <= 0x7fffffffL / 4 && (long)N * H * W <= 0x7fffffffL, "freeu: image too large");
    ST_REQUIRE(slot == 0 || slot == 1, "freeu: slot %d (0: b1, s1; 1: b2, s2)", slot);
    ST_REQUIRE(st_dtype_ok(dtype), "freeu: unsupported dtype %d", dtype);
    const int vec = dtype == ST_F32 ? 4 : 8;
    ST_REQUIRE(C_h % vec == 0 && C_skip % vec == 0, "freeu: channel counts (%d, %d) must be multiples of %d", C_h, C_skip, vec);
    ST_REQUIRE((((uintptr_t)h | (uintptr_t)skip | (uintptr_t)h_out | (uintptr_t)skip_out | (uintptr_t)workspace) & 15) == 0 &&
               ((uintptr_t)params & 3) == 0, "freeu: misaligned pointer");
    const long HW = (long)H * W;
    ST_REQUIRE(workspace_bytes >= st_freeu_workspace_bytes(N, C_skip, HW), "freeu: workspace of %zu bytes, %zu needed", workspace_bytes,
               st_freeu_workspace_bytes(N, C_skip, HW));
    ST_REQUIRE(stat_rows == 0 || stat_rows == stat_rows_for(HW), "freeu: %d rows per statistics partial, this shape emits %d", stat_rows,
               stat_rows_for(HW));
    ST_REQUIRE((stat_rows > 0) == (stats_h != nullptr) && (stat_rows > 0) == (stats_skip != nullptr) &&
               (((uintptr_t)stats_h | (uintptr_t)stats_skip) & 7) == 0, "freeu: statistics buffers and stat_rows do not agree");
    FuShape g = {N, C_h, C_skip, H, W, (int)HW, cdiv(HW, FU_TILE), 0, 0};
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return freeu_launch<bf16>(h, skip, h_out, skip_out, g, params, slot, stats_h, stats_skip, stat_rows, workspace, st);
    if (dtype == ST_F16) return freeu_launch<f16>(h, skip, h_out, skip_out, g, params, slot, stats_h, stats_skip, stat_rows, workspace, st);
    return freeu_launch<float>(h, skip, h_out, skip_out, g, params, slot, stats_h, stats_skip, stat_rows, workspace, st);
}
