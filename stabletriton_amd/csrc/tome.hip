// Token merging (ToMe for Stable Diffusion; include/stabletriton_amd.h, st_tome_*): the four launches that shrink the token count of a
// self-attention site from N to N - r and bring it back.
//
// Geometry.  The N = h * w tokens of a site are D = (h / 2)(w / 2) cells of 2 x 2 tokens.  off[c] in 0..3 (one uint8 row of D per step,
// the row picked by the device step counter) names the cell's dst token, slot (off >> 1, off & 1); its three other tokens are the src
// tokens s = 3 c + k, k = 0..2, at slot k + (k >= off[c]).  Nothing is ever copied into a src / dst order: every kernel computes
// the token of a row from (c, slot) and reads x where it lies.  Table bytes are masked to two bits, so no value can leave the cell.
//
//   match       node_max[s] = max_j cos(src s, dst j), node_idx[s] = the smallest such j.  A block of four waves owns 64 src rows of one
//               batch row and streams the dst rows past them in tiles of 64.  Per (dst tile, 64-wide K slab) the block stages the src
//               and the dst slab in LDS (rows padded to 72 values: the 16-byte fragment reads of 16 rows then fall on distinct banks),
//               the next slab's 16-byte loads in flight under the MFMAs.  Wave v multiplies src rows 16 v .. 16 v + 15 by the four
//               16-column groups of the tile on v_mfma_f32_16x16x32: a lane ends a tile with 4 rows x 4 columns of dot products.
//               The thread that stages a vector also squares it: eight neighbouring lanes hold a row's sum of squares in fp32 when the
//               last slab has passed (dst: every tile; src: the first tile), three shuffles and one v_rsq make 1 / |row| in LDS.
//               The src slab is staged again for every dst tile (a 64 x C tile does not fit LDS beside the dst slab at C = 1280): the
//               kernel reads the block's src rows D / 64 times, from L2 after the first.
//               Epilogue: dot * (1 / |dst j|) against the lane's running (max, arg) - columns only ever ascend within a lane, so a
//               strict > keeps the smallest j -, after the last tile four shuffle rounds across the 16 lanes of a row group (ties to the
//               smaller j), one multiply by 1 / |src s|, one store.  The score matrix exists only as accumulators.
//   select      rank[s] = #{t: max[t] > max[s]} + #{t < s: max[t] == max[s]} by counting: every block keeps all S maxima of its batch
//               row in LDS, a thread ranks one src (LDS broadcast reads), writes where[token] for its src - and for its cell's dst when
//               k == 0 -, assign[s] (node_idx or -1) and, for a kept src, kept[rank - r] = s.  A NaN maximum ranks as -inf, so ranks are a
//               permutation for any input and every word has one writer.
//   merge_norm  one wave per output row, sixteen rows per block.  A row's members - the dst token, then the merged src in ascending s -
//               are LayerNormed one after the other (two passes over the registers: mean, then the squared deviations) and summed in
//               fp32 with gamma and beta applied; blocks that hold rows below D keep assign[] in LDS and find the members of row m by
//               ballot over 64 entries at a time.  Rows from D on are the LayerNorm of kept[m - D].
//   unmerge_add out[token] = x[token] + y[where[token]], one rounding, and the (sum, sum of squares) of the rounded row as the one
//               chunk of LayerNorm partials the next folded projection reads.
// No atomics anywhere: two launches give the same bits.  LDS holds S words in select and merge_norm: S <= ST_TOME_MAX_SRC.
#include "common.h"

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_M = 64, TM_N = 64, TM_K = 64;      // src rows per block, dst rows per tile, K slab
constexpr int TM_LD = 72;                           // LDS row stride in values
constexpr int TM_RPB = 16;                          // rows per block of merge_norm and unmerge_add: four per wave
constexpr int TM_VEC = 4;                           // 16-byte vectors of a row per lane: C <= 64 * 8 * TM_VEC

template <typename E> struct TomeMma;
template <> struct TomeMma<bf16> {
    static __device__ __forceinline__ f32x4 run(const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct TomeMma<f16> {
    static __device__ __forceinline__ f32x4 run(const f16x8& a, const f16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

__device__ __forceinline__ int tome_cell_token(int c, int slot, int wc, int w) {
    const int cy = c / wc, cx = c - cy * wc;
    return (2 * cy + (slot >> 1)) * w + 2 * cx + (slot & 1);
}
__device__ __forceinline__ int tome_dst_token(const unsigned char* off, int c, int wc, int w) { return tome_cell_token(c, off[c] & 3, wc, w); }
__device__ __forceinline__ int tome_src_token(const unsigned char* off, int s, int wc, int w) {
    const int c = s / 3, k = s - 3 * c, o = off[c] & 3;
    return tome_cell_token(c, k + (k >= o ? 1 : 0), wc, w);
}
__device__ __forceinline__ const unsigned char* tome_off_row(const unsigned char* off, const int* step, int n_steps, int D) {
    int i = step ? *step : 0;
    i = i < 0 ? 0 : (i >= n_steps ? n_steps - 1 : i);
    return off + (long)i * D;
}
__device__ __forceinline__ int tome_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- match ----------------------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(TM_THREADS) void tome_match_kernel(const E* x, long ldx, const unsigned char* off, const int* step, int n_steps,
                                                                int N, int C, int w, int D, float* node_max, int* node_idx) {
    typedef typename V16<E>::x8 X8;
    __shared__ __attribute__((aligned(16))) E As[TM_M * TM_LD];
    __shared__ __attribute__((aligned(16))) E Bs[TM_N * TM_LD];
    __shared__ float rnA[TM_M], rnB[TM_N];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, s0 = blockIdx.x * TM_M, S = 3 * D, wc = w >> 1;
    const unsigned char* o = tome_off_row(off, step, n_steps, D);
    const E* xb = x + (long)b * N * ldx;
    // staging: this thread moves values lc .. lc + 7 of rows lr and lr + 32 of both slabs; rows past the end repeat the last one
    const int lr = tid >> 3, lc = (tid & 7) * 8;
    const E* pa[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) pa[i] = xb + (long)tome_src_token(o, min(s0 + lr + 32 * i, S - 1), wc, w) * ldx + lc;
    float ssa[2] = {0.f, 0.f};
    float best[4];
    int bidx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        best[j] = -INFINITY;
        bidx[j] = 0;
    }
    const int nK = C / TM_K, nT = (D + TM_N - 1) / TM_N;
    for (int t = 0; t < nT; ++t) {
        const E* pb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) pb[i] = xb + (long)tome_dst_token(o, min(t * TM_N + lr + 32 * i, D - 1), wc, w) * ldx + lc;
        f32x4 acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        float ssb[2] = {0.f, 0.f};
        X8 ra[2], rb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ra[i] = *reinterpret_cast<const X8*>(pa[i]);
            rb[i] = *reinterpret_cast<const X8*>(pb[i]);
        }
        for (int ks = 0; ks < nK; ++ks) {
            __syncthreads();                                      // the previous slab's fragments are read
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                *reinterpret_cast<X8*>(&As[(lr + 32 * i) * TM_LD + lc]) = ra[i];
                *reinterpret_cast<X8*>(&Bs[(lr + 32 * i) * TM_LD + lc]) = rb[i];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float fb = (float)rb[i][e];
                    ssb[i] = fmaf(fb, fb, ssb[i]);
                }
                if (t == 0) {                                     // (uniform) the src rows are the same on every tile
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float fa = (float)ra[i][e];
                        ssa[i] = fmaf(fa, fa, ssa[i]);
                    }
                }
            }
            __syncthreads();
            if (ks + 1 < nK) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ra[i] = *reinterpret_cast<const X8*>(pa[i] + (ks + 1) * TM_K);
                    rb[i] = *reinterpret_cast<const X8*>(pb[i] + (ks + 1) * TM_K);
                }
            }
#pragma unroll
            for (int kk = 0; kk < TM_K / 32; ++kk) {
                const X8 a = *reinterpret_cast<const X8*>(&As[(wave * 16 + r) * TM_LD + kk * 32 + g * 8]);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const X8 bb = *reinterpret_cast<const X8*>(&Bs[(nt * 16 + r) * TM_LD + kk * 32 + g * 8]);
                    acc[nt] = TomeMma<E>::run(a, bb, acc[nt]);
                }
            }
        }
        // 1 / |row|: the eight lanes of a row meet in a fixed order
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float vb = ssb[i], va = ssa[i];
#pragma unroll
            for (int sh = 1; sh <= 4; sh <<= 1) {
                vb += __shfl_xor(vb, sh, 64);
                va += __shfl_xor(va, sh, 64);
            }
            if ((tid & 7) == 0) {
                rnB[lr + 32 * i] = rsqrtf(fmaxf(vb, 1e-24f));
                if (t == 0) rnA[lr + 32 * i] = rsqrtf(fmaxf(va, 1e-24f));
            }
        }
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int n = nt * 16 + r, j = t * TM_N + n;
            const float rn = rnB[n];
            if (j < D) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float v = acc[nt][q] * rn;
                    if (v > best[q]) {
                        best[q] = v;
                        bidx[q] = j;
                    }
                }
            }
        }
    }
    // the 16 lanes of a row group (same g) hold the candidates of rows 4 g .. 4 g + 3 of the wave
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int sh = 1; sh <= 8; sh <<= 1) {
            const float ov = __shfl_xor(best[q], sh, 64);
            const int oi = __shfl_xor(bidx[q], sh, 64);
            if (ov > best[q] || (ov == best[q] && oi < bidx[q])) {
                best[q] = ov;
                bidx[q] = oi;
            }
        }
    }
    if (r == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = wave * 16 + g * 4 + q, s = s0 + row;
            if (s < S) {
                node_max[(long)b * S + s] = best[q] * rnA[row];
                node_idx[(long)b * S + s] = bidx[q];
            }
        }
    }
}

// ---- select ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TM_THREADS) void tome_select_kernel(const float* node_max, const int* node_idx, const unsigned char* off,
                                                                 const int* step, int n_steps, int N, int w, int D, int r, int* where,
                                                                 int* assign, int* kept) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, b = blockIdx.y, S = 3 * D, wc = w >> 1;
    for (int i = tid; i < S; i += TM_THREADS) {
        const float m = node_max[(long)b * S + i];
        sm[i] = m == m ? m : -INFINITY;                           // NaN ranks as -inf: the order stays total, every word keeps one writer
    }
    __syncthreads();
    const int s = blockIdx.x * TM_THREADS + tid;
    if (s >= S) return;
    const float v = sm[s];
    int rank = 0;
    for (int t = 0; t < S; ++t) {
        const float u = sm[t];
        rank += (u > v || (u == v && t < s)) ? 1 : 0;
    }
    const unsigned char* o = tome_off_row(off, step, n_steps, D);
    const bool merged = rank < r;
    const int j = tome_clamp(node_idx[(long)b * S + s], D - 1);
    where[(long)b * N + tome_src_token(o, s, wc, w)] = merged ? j : D + rank - r;
    assign[(long)b * S + s] = merged ? j : -1;
    if (!merged) kept[(long)b * S + rank - r] = s;
    if (s % 3 == 0) where[(long)b * N + tome_dst_token(o, s / 3, wc, w)] = s / 3;
}

// ---- merge + LayerNorm ----------------------------------------------------------------------------------------------------------
// acc += LayerNorm(row) * gamma + beta, the row spread over the wave in 16-byte vectors lane, lane + 64, ...
template <typename E>
__device__ __forceinline__ void tome_add_normed(const E* row, const E* gamma, const E* beta, int nv, int C, float eps, int lane,
                                                float (&acc)[TM_VEC][8]) {
    float xv[TM_VEC][8];
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < TM_VEC; ++q) {
        const int v = lane + 64 * q;
        if (v < nv) {
            const Vec16<E> t = load16(row + v * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                xv[q][e] = t.get(e);
                sum += xv[q][e];
            }
        }
    }
    const float mean = wave_sum(sum) / (float)C;
    float dev = 0.f;
#pragma unroll
    for (int q = 0; q < TM_VEC; ++q)
        if (lane + 64 * q < nv) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                xv[q][e] -= mean;
                dev = fmaf(xv[q][e], xv[q][e], dev);
            }
        }
    const float rstd = rsqrtf(wave_sum(dev) / (float)C + eps);
#pragma unroll
    for (int q = 0; q < TM_VEC; ++q) {
        const int v = lane + 64 * q;
        if (v < nv) {
            const Vec16<E> gv = load16(gamma + v * 8), bv = load16(beta + v * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[q][e] += fmaf(xv[q][e] * rstd, gv.get(e), bv.get(e));
        }
    }
}

template <typename E>
__global__ __launch_bounds__(TM_THREADS) void tome_merge_norm_kernel(const E* x, long ldx, const E* gamma, const E* beta, float eps,
                                                                     const unsigned char* off, const int* step, int n_steps,
                                                                     const int* assign, const int* kept, int N, int C, int w, int D, int r,
                                                                     E* y) {
    extern __shared__ int sa[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, m0 = blockIdx.x * TM_RPB, S = 3 * D, R = N - r, wc = w >> 1, nv = C >> 3;
    if (m0 < D) {                                                 // (uniform) the block holds merged rows: their members come from assign[]
        for (int i = tid; i < S; i += TM_THREADS) sa[i] = assign[(long)b * S + i];
        __syncthreads();
    }
    const unsigned char* o = tome_off_row(off, step, n_steps, D);
    const E* xb = x + (long)b * N * ldx;
    for (int i = 0; i < TM_RPB / 4; ++i) {
        const int m = m0 + wave * (TM_RPB / 4) + i;
        if (m >= R) break;                                        // (uniform per wave)
        float acc[TM_VEC][8];
#pragma unroll
        for (int q = 0; q < TM_VEC; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[q][e] = 0.f;
        int count = 0;
        if (m < D) {
            tome_add_normed(xb + (long)tome_dst_token(o, m, wc, w) * ldx, gamma, beta, nv, C, eps, lane, acc);
            for (int base = 0; base < S; base += 64) {
                const int idx = base + lane;
                unsigned long long hits = __ballot(idx < S && sa[idx] == m);
                while (hits) {                                    // ascending s
                    const int k = __ffsll((long long)hits) - 1;
                    hits &= hits - 1;
                    tome_add_normed(xb + (long)tome_src_token(o, base + k, wc, w) * ldx, gamma, beta, nv, C, eps, lane, acc);
                    ++count;
                }
            }
        } else {
            const int s = tome_clamp(kept[(long)b * S + m - D], S - 1);
            tome_add_normed(xb + (long)tome_src_token(o, s, wc, w) * ldx, gamma, beta, nv, C, eps, lane, acc);
        }
        const float inv = 1.0f / (float)(1 + count);
        E* yr = y + ((long)b * R + m) * C;
#pragma unroll
        for (int q = 0; q < TM_VEC; ++q) {
            const int v = lane + 64 * q;
            if (v < nv) {
                Vec16<E> t;
#pragma unroll
                for (int e = 0; e < 8; ++e) t.set(e, acc[q][e] * inv);
                store16(yr + v * 8, t);
            }
        }
    }
}

// ---- unmerge + residual ---------------------------------------------------------------------------------------------------------
template <typename E>
__global__ __launch_bounds__(TM_THREADS) void tome_unmerge_add_kernel(const E* x, long ldx, const E* y, const int* where, int N, int R, int C,
                                                                      E* out, float2* stats) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, nv = C >> 3;
    for (int i = 0; i < TM_RPB / 4; ++i) {
        const int t = blockIdx.x * TM_RPB + wave * (TM_RPB / 4) + i;
        if (t >= N) break;                                        // (uniform per wave)
        const long row = (long)b * N + t;
        const E* xr = x + row * ldx;
        const E* yr = y + ((long)b * R + tome_clamp(where[row], R - 1)) * C;
        E* orow = out + row * C;
        float s1 = 0.f, s2 = 0.f;
        for (int v = lane; v < nv; v += 64) {
            const Vec16<E> a = load16(xr + v * 8), c = load16(yr + v * 8);
            Vec16<E> d;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                d.set(e, a.get(e) + c.get(e));
                const float f = d.get(e);                         // the stored value
                s1 += f;
                s2 = fmaf(f, f, s2);
            }
            store16(orow + v * 8, d);
        }
        if (stats) {
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            if (lane == 0) stats[row] = make_float2(s1, s2);
        }
    }
}

// what the four entry points check alike: the grid, the table and the batch
int tome_check_site(const char* who, const unsigned char* off, const int* step, int n_steps, int B, int h, int w) {
    ST_REQUIRE(B > 0 && B <= 65535, "%s: batch of %d rows (1 to 65535)", who, B);
    ST_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "%s: the token grid %d x %d must have even sides: odd grids are not merged", who, h, w);
    ST_REQUIRE((long)h * w / 4 * 3 <= ST_TOME_MAX_SRC, "%s: %ld src tokens, at most %d (the rank and member tables live in LDS)", who,
               (long)h * w / 4 * 3, ST_TOME_MAX_SRC);
    ST_REQUIRE(off, "%s: null pointer (off)", who);
    ST_REQUIRE(n_steps >= 1, "%s: offset table of %d rows", who, n_steps);
    ST_REQUIRE(((uintptr_t)step & 3) == 0, "%s: misaligned step counter", who);
    return 0;
}

int tome_check_rows(const char* who, const void* p, long ld, int C, int dtype) {
    ST_REQUIRE(st_dtype_is16(dtype), "%s: 16-bit types only (dtype %d); other types take the host's plain form", who, dtype);
    ST_REQUIRE(C >= 64 && C % 64 == 0 && C <= 64 * 8 * TM_VEC, "%s: C = %d must be a multiple of 64, at most %d", who, C, 64 * 8 * TM_VEC);
    ST_REQUIRE(p, "%s: null pointer (x)", who);
    ST_REQUIRE((uintptr_t)p % 16 == 0 && ld % 8 == 0 && ld >= C && ld < (1L << 31), "%s: rows must keep 16-byte alignment, stride %ld >= C = %d", who, ld, C);
    return 0;
}

}  // namespace

extern "C" int st_tome_match(const void* x, long ldx, const unsigned char* off, const int* step, int n_steps, int B, int h, int w, int C,
                             float* node_max, int* node_idx, int dtype, void* stream) {
    if (int e = tome_check_site("tome_match", off, step, n_steps, B, h, w)) return e;
    if (int e = tome_check_rows("tome_match", x, ldx, C, dtype)) return e;
    ST_REQUIRE(node_max && node_idx, "tome_match: null pointer (node_max / node_idx)");
    ST_REQUIRE((((uintptr_t)node_max | (uintptr_t)node_idx) & 3) == 0, "tome_match: misaligned output");
    const int N = h * w, D = N / 4;
    const dim3 grid((3 * D + TM_M - 1) / TM_M, B);
    if (dtype == ST_BF16)
        hipLaunchKernelGGL(tome_match_kernel<bf16>, grid, dim3(TM_THREADS), 0, (hipStream_t)stream, (const bf16*)x, ldx, off, step, n_steps, N, C, w, D, node_max, node_idx);
    else
        hipLaunchKernelGGL(tome_match_kernel<f16>, grid, dim3(TM_THREADS), 0, (hipStream_t)stream, (const f16*)x, ldx, off, step, n_steps, N, C, w, D, node_max, node_idx);
    return st_check_launch("tome_match");
}

extern "C" int st_tome_select(const float* node_max, const int* node_idx, const unsigned char* off, const int* step, int n_steps, int B, int h,
                              int w, int r, int* where, int* assign, int* kept, void* stream) {
    if (int e = tome_check_site("tome_select", off, step, n_steps, B, h, w)) return e;
    ST_REQUIRE(node_max && node_idx && where && assign && kept, "tome_select: null pointer");
    ST_REQUIRE((((uintptr_t)node_max | (uintptr_t)node_idx | (uintptr_t)where | (uintptr_t)assign | (uintptr_t)kept) & 3) == 0, "tome_select: misaligned pointer");
    const int N = h * w, D = N / 4, S = 3 * D;
    ST_REQUIRE(r >= 0 && r <= S, "tome_select: r = %d out of range (0 to %d src tokens)", r, S);
    hipLaunchKernelGGL(tome_select_kernel, dim3((S + TM_THREADS - 1) / TM_THREADS, B), dim3(TM_THREADS), (size_t)S * sizeof(float), (hipStream_t)stream,
                       node_max, node_idx, off, step, n_steps, N, w, D, r, where, assign, kept);
    return st_check_launch("tome_select");
}

extern "C" int st_tome_merge_norm(const void* x, long ldx, const void* gamma, const void* beta, float eps, const unsigned char* off,
                                  const int* step, int n_steps, const int* assign, const int* kept, int B, int h, int w, int C, int r, void* y,
                                  int dtype, void* stream) {
    if (int e = tome_check_site("tome_merge_norm", off, step, n_steps, B, h, w)) return e;
    if (int e = tome_check_rows("tome_merge_norm", x, ldx, C, dtype)) return e;
    ST_REQUIRE(gamma && beta && assign && kept && y, "tome_merge_norm: null pointer");
    ST_REQUIRE((((uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) == 0 && (((uintptr_t)assign | (uintptr_t)kept) & 3) == 0, "tome_merge_norm: misaligned pointer");
    ST_REQUIRE(eps > 0.f, "tome_merge_norm: eps must be positive");
    const int N = h * w, D = N / 4, S = 3 * D;
    ST_REQUIRE(r >= 0 && r <= S, "tome_merge_norm: r = %d out of range (0 to %d src tokens)", r, S);
    const dim3 grid((N - r + TM_RPB - 1) / TM_RPB, B);
    const size_t lds = (size_t)S * sizeof(int);
    if (dtype == ST_BF16)
        hipLaunchKernelGGL(tome_merge_norm_kernel<bf16>, grid, dim3(TM_THREADS), lds, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)gamma,
                           (const bf16*)beta, eps, off, step, n_steps, assign, kept, N, C, w, D, r, (bf16*)y);
    else
        hipLaunchKernelGGL(tome_merge_norm_kernel<f16>, grid, dim3(TM_THREADS), lds, (hipStream_t)stream, (const f16*)x, ldx, (const f16*)gamma,
                           (const f16*)beta, eps, off, step, n_steps, assign, kept, N, C, w, D, r, (f16*)y);
    return st_check_launch("tome_merge_norm");
}

extern "C" int st_tome_unmerge_add(const void* x, long ldx, const void* y, const int* where, int B, int N, int R, int C, void* out, float* stats,
                                   int dtype, void* stream) {
    if (int e = tome_check_rows("tome_unmerge_add", x, ldx, C, dtype)) return e;
    ST_REQUIRE(B > 0 && B <= 65535 && N > 0 && (long)B * N < (1L << 31), "tome_unmerge_add: bad shape B=%d N=%d", B, N);
    ST_REQUIRE(R >= 1 && R <= N, "tome_unmerge_add: %d merged rows out of range (1 to N = %d)", R, N);
    ST_REQUIRE(y && where && out, "tome_unmerge_add: null pointer");
    ST_REQUIRE((((uintptr_t)y | (uintptr_t)out) & 15) == 0 && ((uintptr_t)where & 3) == 0 && ((uintptr_t)stats & 7) == 0, "tome_unmerge_add: misaligned pointer");
    const dim3 grid((N + TM_RPB - 1) / TM_RPB, B);
    if (dtype == ST_BF16)
        hipLaunchKernelGGL(tome_unmerge_add_kernel<bf16>, grid, dim3(TM_THREADS), 0, (hipStream_t)stream, (const bf16*)x, ldx, (const bf16*)y, where, N, R, C, (bf16*)out, (float2*)stats);
    else
        hipLaunchKernelGGL(tome_unmerge_add_kernel<f16>, grid, dim3(TM_THREADS), 0, (hipStream_t)stream, (const f16*)x, ldx, (const f16*)y, where, N, R, C, (f16*)out, (float2*)stats);
    return st_check_launch("tome_unmerge_add");
}
