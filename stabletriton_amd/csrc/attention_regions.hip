// Regional cross-attention: several key/value segments behind one query, each with its OWN softmax, combined per query row.
//
//   out[b,t,h,:] = sum_r  w[b,r,t] * softmax_s(scale * q[b,t,h] . k[b, r*L+s, h]) v[b, r*L+s, h]        (s over segment r's L keys)
//
// q (B, T, H*64), k / v (B, R*L, H*64): R text contexts concatenated along the token axis (regional prompting: ComfyUI's
// conditioning masks / "attention couple", the diffusers community regional-prompting pipeline); w (B, R, T) fp32, dense, NOT
// normalised here: any finite weights are legal.
//
// One launch with the grid and block of the text-context launch of st_attention (attention.hip: 64 query rows per block of four
// waves, one head, one batch entry).  A block runs the body of that kernel (attn16_core_run, attention_core.h) once per segment,
// with K / V advanced by r * L rows and S = L: its tail handling (rows >= S read a zero line, their scores are masked) hides the
// next segment's real keys.  Nothing is shared between segments - reference maximum, row sum and O start over - and the
// normalised fp32 result of a segment stays in registers: acc = fma(w, o / l, acc), rounded to the storage type ONCE at the end.
// With w = 1 on one segment and 0 elsewhere that is fma(1, x, 0) = x and fma(0, y, x) = x (y finite): the bits of st_attention on
// that segment's slice.
//
// fp16 needs one more thing to keep those bits.  As compiled, st_attention's fp16 epilogue `(E)(o * inv)` rounds elements 0 and 3
// of every four ONCE, from the exact product (v_fma_mixlo_f16), and elements 1 and 2 twice (v_pk_mul_f32, v_cvt_pk_f16_f32); the
// two differ where the fp32 product lands on a binary16 midpoint, about 3 values in 10^5.  The fp32 value o * inv alone cannot
// give the first kind back, so for those elements the kernel also carries the product's fp32 residual fma(o, inv, -(o * inv))
// (exact), weighted like the value itself, and the final conversion is one rounding of value + residual (RegionsOut,
// fma_mix_f16 in attention_sum.h).  tests/test_regions_gpu.py pins the correspondence bit for bit; bf16 converts every element alike.
//
// Between two segments there is a block-wide barrier: the body ends on s_waitcnt vmcnt(0) with no barrier, and its prologue
// requests tiles 0 and 1 into ring slots 0 and 1 at once - without the barrier a fast wave's next-segment DMA could land in the
// slot a slow wave still reads V from.  No segment is skipped (a zero-weight segment's K / V must be finite: the caller's duty),
// so every wave of a block takes part in every cooperative tile load.
// No atomics; the only stores are the T * H * 64 values of `out`.  16-bit element types only (fp32 and the other head sizes go
// R times through st_attention: ops.attention_regions).
#include "attention_sum.h"      // RegionsOut, fma_mix_f16, regions_round, REGIONS_MAX: shared with attention_segments.hip

template <typename E>
__global__ __launch_bounds__(256) void attn_regions_kernel(const E* __restrict__ Q, const E* __restrict__ K, const E* __restrict__ V,
                                                           const float* __restrict__ W, E* __restrict__ O, int T, int R, int L,
                                                           long ldq, long ldk, long ldv, long ldo, float scale_log2e) {
    typedef typename V16<E>::x4 E4;
    __shared__ __attribute__((aligned(16))) char lds[3 * 2 * ATT_KV * 128];
    const int t_ = threadIdx.x, lane = t_ & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t_ >> 6);
    const int head = blockIdx.y, b = blockIdx.z;
    const int row0 = blockIdx.x * 64;
    const int c16 = lane & 15, g = lane >> 4;
    const int row = row0 + wave * 16 + c16;                  // this lane's query row; rows >= T are clamped on load, not stored
    const size_t S = (size_t)R * L;
    const E* Qb = Q + (size_t)b * T * ldq + (size_t)row0 * ldq + (size_t)head * ATT_D;
    const E* Kb = K + (size_t)b * S * ldk + (size_t)head * ATT_D;
    const E* Vb = V + (size_t)b * S * ldv + (size_t)head * ATT_D;
    const float* Wb = W + (size_t)b * R * T + min(row, T - 1);

    f32x4 acc[4], res[4];                                    // the weighted sum; res: the products' residuals (fused fp16 elements only)
#pragma unroll
    for (int db = 0; db < 4; ++db) { acc[db] = f32x4{0.f, 0.f, 0.f, 0.f}; res[db] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int r = 0; r < R; ++r) {
        const float w = Wb[(size_t)r * T];
        if (r) __builtin_amdgcn_s_barrier();                 // every wave is done with the ring of segment r - 1
        attn16_core_run<E, 4>(Qb, ldq, T - row0, Kb + (size_t)r * L * ldk, Vb + (size_t)r * L * ldv, ldk, ldv, L, scale_log2e, lds,
                              wave, lane, [&](const f32x4 (&o)[5], float inv, int, int) {
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = o[db][e] * inv;
                    acc[db][e] = __builtin_fmaf(w, x, acc[db][e]);
                    if constexpr (RegionsOut<E>::fused(0) || RegionsOut<E>::fused(1) || RegionsOut<E>::fused(2) || RegionsOut<E>::fused(3))
                        if (RegionsOut<E>::fused(e)) res[db][e] = __builtin_fmaf(w, __builtin_fmaf(o[db][e], inv, -x), res[db][e]);
                }
        });
    }
    if (row < T) {
        E* orow = O + (size_t)b * T * ldo + (size_t)row * ldo + (size_t)head * ATT_D;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            E4 a_;
#pragma unroll
            for (int e = 0; e < 4; ++e) a_[e] = RegionsOut<E>::fused(e) ? regions_round<E>(acc[db][e], res[db][e]) : (E)acc[db][e];
            *reinterpret_cast<E4*>(orow + 16 * db + 4 * g) = a_;
        }
    }
}

template <typename E>
static int attention_regions_launch(const void* q, const void* k, const void* v, const float* w, void* out, int B, int T, int R, int L,
                                    int H, long ldq, long ldk, long ldv, long ldo, float scale, hipStream_t st) {
    hipLaunchKernelGGL((attn_regions_kernel<E>), dim3(cdiv(T, 64), H, B), dim3(256), 0, st, (const E*)q, (const E*)k, (const E*)v, w,
                       (E*)out, T, R, L, ldq, ldk, ldv, ldo, scale * 1.4426950408889634f);
    return st_check_launch("attention_regions");
}

extern "C" int st_attention_regions(const void* q, const void* k, const void* v, const float* weights, void* out,
                                    int B, int T, int R, int seg_len, int H, int D,
                                    long ldq, long ldk, long ldv, long ldo, float scale, int dtype, void* stream) {
    ST_REQUIRE(q, "attention_regions: q is null");
    ST_REQUIRE(k, "attention_regions: k is null");
    ST_REQUIRE(v, "attention_regions: v is null");
    ST_REQUIRE(weights, "attention_regions: weights is null");
    ST_REQUIRE(out, "attention_regions: out is null");
    ST_REQUIRE(B > 0 && T > 0 && H > 0, "attention_regions: bad shape B=%d T=%d H=%d", B, T, H);
    ST_REQUIRE(dtype == ST_BF16 || dtype == ST_F16, "attention_regions: dtype %d not supported (ST_BF16 or ST_F16)", dtype);
    ST_REQUIRE(D == ATT_D, "attention_regions: D (head_dim) %d not supported (only %d)", D, ATT_D);
    ST_REQUIRE(R >= 1 && R <= REGIONS_MAX, "attention_regions: R %d outside [1, %d]", R, REGIONS_MAX);
    ST_REQUIRE(seg_len >= 1 && seg_len < 256, "attention_regions: seg_len %d outside [1, 255]", seg_len);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_regions: too many heads/batches for one launch (H=%d B=%d)", H, B);
    const long cols = (long)H * D;
    ST_REQUIRE(ldq % 8 == 0 && ldq >= cols, "attention_regions: ldq %ld must be a multiple of 8 elements (16-byte rows) and >= H*D", ldq);
    ST_REQUIRE(ldk % 8 == 0 && ldk >= cols, "attention_regions: ldk %ld must be a multiple of 8 elements (16-byte rows) and >= H*D", ldk);
    ST_REQUIRE(ldv % 8 == 0 && ldv >= cols, "attention_regions: ldv %ld must be a multiple of 8 elements (16-byte rows) and >= H*D", ldv);
    ST_REQUIRE(ldo % 4 == 0 && ldo >= cols, "attention_regions: ldo %ld must be a multiple of 4 elements and >= H*D", ldo);
    ST_REQUIRE((uintptr_t)q % 16 == 0, "attention_regions: q must be 16-byte aligned");
    ST_REQUIRE((uintptr_t)k % 16 == 0, "attention_regions: k must be 16-byte aligned");
    ST_REQUIRE((uintptr_t)v % 16 == 0, "attention_regions: v must be 16-byte aligned");
    ST_REQUIRE((uintptr_t)out % 16 == 0, "attention_regions: out must be 16-byte aligned");
    ST_REQUIRE((uintptr_t)weights % 4 == 0, "attention_regions: weights must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return attention_regions_launch<bf16>(q, k, v, weights, out, B, T, R, seg_len, H, ldq, ldk, ldv, ldo, scale, st);
    return attention_regions_launch<f16>(q, k, v, weights, out, B, T, R, seg_len, H, ldq, ldk, ldv, ldo, scale, st);
}
