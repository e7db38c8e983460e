// Column sums of a self-attention's softmax matrix (self-attention guidance, sag.py; header: st_attention_colsum):
//   A[b, j] = (1 / H) sum_h sum_i P[b, h, i, j],   P = softmax_j(q_i . k_j * scale)
// one fp32 value per key token, from q and k where the fused q|k|v projection left them.  The (B H, T, T) matrix is never stored:
// the attention kernels do not form it either, so it is computed here a second time, in two passes over QK^T on the matrix pipe
// (v_mfma_f32_16x16x32, S^T[key][query] = K Q^T as in attention_core.h's 16-row kernel: a lane holds query l & 15, keys 4 (l >> 4) + r
// of every 16-key block) and one small pass over the heads.
//
//   rows pass   one block = 64 query rows of one (b, h), 16 per wave, their Q fragments in registers.  The 64-key tiles of K come
//               through LDS (global -> registers -> LDS, the next tile's loads in flight under this tile's MFMAs).  Every lane
//               keeps an online (maximum, sum) over the keys IT holds; the four lanes of a query are merged once, at the end, in
//               lane order.  Writes lse[b, h, i] = m_i + log2(l_i), base-2 units, fp32.  No PV product.
//   cols pass   one block = a 64-key tile of one (b, h), its K fragments in registers of every wave; the 64-query tiles of Q come
//               through LDS the same way, wave w takes queries 16 w .. 16 w + 15 of each.  p = exp2(s - lse_i) is added to 16
//               per-lane accumulators (the lane's keys x its query column); at the end the 16 lanes that share a key are summed by
//               a butterfly, the four waves through LDS in wave order.  Writes part[b, h, j].
//   heads pass  A[b, j] = (sum_h part[b, h, j], h ascending) * (1 / H).
//
// Both matrix passes form a score with the same operand roles and the same two-MFMA chain, then one fp32 multiply by
// scale * log2(e): the bits of s are the same in both, so p <= 1 up to the rounding of lse.  No atomics and no tickets: every sum's
// tree is fixed by the shape (style_adain.hip's rule), the bits do not depend on the order the blocks run in.  Query rows past T are
// loaded as zeros and given lse = +inf (p = 0); keys past T score -inf in the rows pass and are not written by the cols pass.
#include "attention_core.h"

namespace {

constexpr int CS_TILE = 64;          // query rows of a rows-pass block, keys of a cols-pass block, rows of an LDS tile
constexpr int CS_THREADS = 256;
constexpr int CS_ROW_B = 144;        // bytes of an LDS row: 128 of data + 16 of padding (the 16 rows of a fragment read start in distinct banks)
constexpr float CS_LOG2E = 1.4426950408889634f;

// 64 rows x 64 values of one head: 512 16-byte pieces, two per thread; rows at or past `limit` are zeros
template <typename E>
__device__ __forceinline__ void cs_fetch(const E* base, long ld, int row0, int limit, int tid, u32x4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = tid + CS_THREADS * i, row = row0 + (p >> 3), c = p & 7;
        r[i] = row < limit ? *reinterpret_cast<const u32x4*>(base + (size_t)row * ld + c * 8) : u32x4{0u, 0u, 0u, 0u};
    }
}
__device__ __forceinline__ void cs_stash(char* lds, int tid, const u32x4 (&r)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = tid + CS_THREADS * i;
        *reinterpret_cast<u32x4*>(lds + (p >> 3) * CS_ROW_B + (p & 7) * 16) = r[i];
    }
}
// MFMA operand of rows 16 blk + (lane & 15), values 32 ks + 8 (lane >> 4) .. + 7: from an LDS tile, or from global (rows clamped)
template <typename E>
__device__ __forceinline__ typename V16<E>::x8 cs_frag_lds(const char* lds, int blk, int ks, int c16, int g) {
    return *reinterpret_cast<const typename V16<E>::x8*>(lds + (16 * blk + c16) * CS_ROW_B + (4 * ks + g) * 16);
}
template <typename E>
__device__ __forceinline__ typename V16<E>::x8 cs_frag_global(const E* base, long ld, int row, int limit, int ks, int g) {
    return *reinterpret_cast<const typename V16<E>::x8*>(base + (size_t)min(row, limit - 1) * ld + 32 * ks + 8 * g);
}
// the score block S^T[16 keys][16 queries] in base-2 exponent units
template <typename E>
__device__ __forceinline__ f32x4 cs_scores(const typename V16<E>::x8 (&kf)[2], const typename V16<E>::x8 (&qf)[2], float scale_log2e) {
    f32x4 s = AttMma<E>::m16(kf[0], qf[0], f32x4{0.f, 0.f, 0.f, 0.f});
    s = AttMma<E>::m16(kf[1], qf[1], s);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = __fmul_rn(s[r], scale_log2e);
    return s;
}

__device__ __forceinline__ void cs_decode(int T, int H, int& bh, int& tile, int& b, int& h) {
    const int nt = (T + CS_TILE - 1) / CS_TILE;
    bh = blockIdx.x / nt;
    tile = blockIdx.x - bh * nt;
    b = bh / H;
    h = bh - b * H;
}

template <typename E>
__global__ __launch_bounds__(CS_THREADS) void colsum_rows_kernel(const E* __restrict__ q, const E* __restrict__ k, float* __restrict__ lse,
                                                                 int T, int H, long ldq, long ldk, float scale_log2e) {
    typedef typename V16<E>::x8 E8;
    __shared__ __attribute__((aligned(16))) char lds[CS_TILE * CS_ROW_B];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
    int bh, qt, b, h;
    cs_decode(T, H, bh, qt, b, h);
    const E* Q = q + (size_t)b * T * ldq + h * ATT_D;
    const E* K = k + (size_t)b * T * ldk + h * ATT_D;
    const int row = qt * CS_TILE + wave * 16 + c16;
    E8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = cs_frag_global(Q, ldq, row, T, ks, g);

    float m = -INFINITY, l = 0.f;                 // over the keys this lane holds
    const int nkt = (T + CS_TILE - 1) / CS_TILE;
    u32x4 stage[2];
    cs_fetch(K, ldk, 0, T, tid, stage);
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();                          // the previous tile has been read by every wave
        cs_stash(lds, tid, stage);
        __syncthreads();
        if (kt + 1 < nkt) cs_fetch(K, ldk, (kt + 1) * CS_TILE, T, tid, stage);
        f32x4 s[4];
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const E8 kf[2] = {cs_frag_lds<E>(lds, kb, 0, c16, g), cs_frag_lds<E>(lds, kb, 1, c16, g)};
            s[kb] = cs_scores<E>(kf, qf, scale_log2e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (kt * CS_TILE + 16 * kb + 4 * g + r >= T) s[kb][r] = -INFINITY;
                mx = fmaxf(mx, s[kb][r]);
            }
        }
        const float m_new = fmaxf(m, mx);
        if (m_new > -INFINITY) {                  // (a lane whose keys so far all lie past T keeps (-inf, 0))
            float add = 0.f;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) add += fast_exp2(s[kb][r] - m_new);
            l = l * fast_exp2(m - m_new) + add;
            m = m_new;
        }
    }
    // the four lanes of a query (g = 0..3), merged in that order by every one of them
    float mg[4], lg[4], M = -INFINITY, L = 0.f;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
        mg[gg] = __shfl(m, c16 + 16 * gg, 64);
        lg[gg] = __shfl(l, c16 + 16 * gg, 64);
        M = fmaxf(M, mg[gg]);
    }
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) L += lg[gg] * fast_exp2(mg[gg] - M);
    if (g == 0 && row < T) lse[(size_t)bh * T + row] = M + log2f(L);
}

template <typename E>
__global__ __launch_bounds__(CS_THREADS) void colsum_cols_kernel(const E* __restrict__ q, const E* __restrict__ k, const float* __restrict__ lse,
                                                                 float* __restrict__ part, int T, int H, long ldq, long ldk,
                                                                 float scale_log2e) {
    typedef typename V16<E>::x8 E8;
    __shared__ __attribute__((aligned(16))) char lds[CS_TILE * CS_ROW_B];
    __shared__ float red[CS_THREADS / 64][CS_TILE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c16 = lane & 15, g = lane >> 4;
    int bh, kt, b, h;
    cs_decode(T, H, bh, kt, b, h);
    const E* Q = q + (size_t)b * T * ldq + h * ATT_D;
    const E* K = k + (size_t)b * T * ldk + h * ATT_D;
    E8 kf[4][2];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) kf[kb][ks] = cs_frag_global(K, ldk, kt * CS_TILE + 16 * kb + c16, T, ks, g);

    float acc[4][4];                              // [key block][r]: this lane's keys, summed over its query column of every tile
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[kb][r] = 0.f;
    const int nqt = (T + CS_TILE - 1) / CS_TILE;
    u32x4 stage[2];
    cs_fetch(Q, ldq, 0, T, tid, stage);
    for (int qt = 0; qt < nqt; ++qt) {
        __syncthreads();
        cs_stash(lds, tid, stage);
        __syncthreads();
        if (qt + 1 < nqt) cs_fetch(Q, ldq, (qt + 1) * CS_TILE, T, tid, stage);
        const int row = qt * CS_TILE + wave * 16 + c16;
        const float ls = row < T ? lse[(size_t)bh * T + row] : INFINITY;      // a row past T: exp2(s - inf) = 0
        const E8 qf[2] = {cs_frag_lds<E>(lds, wave, 0, c16, g), cs_frag_lds<E>(lds, wave, 1, c16, g)};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const f32x4 s = cs_scores<E>(kf[kb], qf, scale_log2e);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[kb][r] += fast_exp2(s[r] - ls);
        }
    }
    // the 16 query columns of a wave (lanes that differ in l & 15): a butterfly, the same sum in every lane
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[kb][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
            if (c16 == 0) red[wave][16 * kb + 4 * g + r] = v;
        }
    __syncthreads();
    if (tid < CS_TILE) {                          // the four waves, in wave order
        const int key = kt * CS_TILE + tid;
        const float v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        if (key < T) part[(size_t)bh * T + key] = v;
    }
}

__global__ __launch_bounds__(CS_THREADS) void colsum_heads_kernel(const float* __restrict__ part, float* __restrict__ out, int B, int T, int H) {
    const long idx = (long)blockIdx.x * CS_THREADS + threadIdx.x;
    if (idx >= (long)B * T) return;
    const int b = (int)(idx / T), j = (int)(idx - (long)b * T);
    float v = 0.f;
    for (int h = 0; h < H; ++h) v += part[((size_t)b * H + h) * T + j];
    out[idx] = v * (1.0f / (float)H);
}

template <typename E>
int colsum_launch(const void* q, const void* k, float* out, int B, int T, int H, long ldq, long ldk, float scale, float* ws, hipStream_t st) {
    const int nt = (T + CS_TILE - 1) / CS_TILE;
    const dim3 grid((unsigned)((long)B * H * nt));
    float* lse = ws;
    float* part = ws + (size_t)B * H * T;
    const float sl = scale * CS_LOG2E;
    hipLaunchKernelGGL(colsum_rows_kernel<E>, grid, dim3(CS_THREADS), 0, st, (const E*)q, (const E*)k, lse, T, H, ldq, ldk, sl);
    if (st_check_launch("attention_colsum (rows)")) return 1;
    hipLaunchKernelGGL(colsum_cols_kernel<E>, grid, dim3(CS_THREADS), 0, st, (const E*)q, (const E*)k, (const float*)lse, part, T, H, ldq, ldk, sl);
    if (st_check_launch("attention_colsum (columns)")) return 1;
    hipLaunchKernelGGL(colsum_heads_kernel, dim3((unsigned)(((long)B * T + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0, st,
                       (const float*)part, out, B, T, H);
    return st_check_launch("attention_colsum (heads)");
}

}  // namespace

extern "C" long st_attention_colsum_workspace(int B, int T, int H) {
    if (B <= 0 || T <= 0 || H <= 0) return 0;
    return 2L * B * H * T;                        // lse and the per-head partials
}

extern "C" int st_attention_colsum(const void* q, const void* k, float* out, int B, int T, int H, int D, long ldq, long ldk, float scale,
                                   float* workspace, long workspace_floats, int dtype, void* stream) {
    ST_REQUIRE(q && k && out && workspace, "attention_colsum: null pointer");
    ST_REQUIRE(B > 0 && T > 0 && H > 0, "attention_colsum: bad sizes (B %d, T %d, H %d)", B, T, H);
    ST_REQUIRE(D == ATT_D, "attention_colsum: head size %d (the kernel is built for %d)", D, ATT_D);
    ST_REQUIRE(st_dtype_is16(dtype), "attention_colsum: dtype %d (bf16 or fp16 expected)", dtype);
    ST_REQUIRE(ldq >= (long)H * D && ldk >= (long)H * D && ldq % 8 == 0 && ldk % 8 == 0, "attention_colsum: ldq %ld / ldk %ld must be multiples of 8 and >= H * D", ldq, ldk);
    ST_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)workspace % 4 == 0,
               "attention_colsum: q and k must be 16-byte aligned");
    ST_REQUIRE(workspace_floats >= st_attention_colsum_workspace(B, T, H), "attention_colsum: the workspace holds %ld floats, %ld needed",
               workspace_floats, st_attention_colsum_workspace(B, T, H));
    ST_REQUIRE((long)B * H * ((T + CS_TILE - 1) / CS_TILE) <= 0x7fffffffL && (long)B * T <= 0x7fffffffL * CS_THREADS, "attention_colsum: grid too large");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return colsum_launch<bf16>(q, k, out, B, T, H, ldq, ldk, scale, workspace, st);
    return colsum_launch<f16>(q, k, out, B, T, H, ldq, ldk, scale, workspace, st);
}
