// Ragged segmented cross-attention: several key/value segments behind one query, each with its OWN softmax, of DIFFERENT lengths,
// in DIFFERENT buffers, combined per query row under a live per-segment scale (IP-Adapter's decoupled cross-attention:
// out = Attn(q, K_text, V_text) + s * Attn(q, K_img, V_img); ip_adapter.py).
//
//   out[b,t,h,:] = sum_r  w_eff[b,r,t] * softmax_s(scale * q[b,t,h] . k_r[b,s,h]) v_r[b,s,h]        (s over segment r's len_r keys)
//   w_eff[b,r,t] = fl32(seg_scale[r] * weights[b,r,t])                                                (seg_scale NULL: all 1)
//
// The regional kernel (attention_regions.hip) with three things it cannot express: every segment brings its own descriptor
// (k, v, token strides, batch strides, length) - they travel BY VALUE in the kernel arguments, so a captured graph keeps them;
// `seg_scale` (S floats) and `weights` (B, S, T) are read from device memory at every launch: the live knobs; and a segment whose
// scale is 0 is skipped by the whole grid.
//
// Same grid and block as the regional kernel and the text-context launch of st_attention (64 query rows per block of four waves,
// one head, one batch entry).  Segments run in index order through attn16_core_run (attention_core.h) with their own Kb, Vb, ldk,
// ldv and S = len_r; its tail handling (rows >= len_r read a zero line, their scores are masked) bounds every read by the
// segment's own length.  acc = fma(w_eff, o / l, acc) in fp32, rounded ONCE at the end; fp16 carries the product residual as the
// regional kernel does (attention_sum.h), so one-hot weights give the bits of st_attention on that segment.
//
// Skip: seg_scale[r] == 0 -> the segment is not run: its K / V are never read (they need not be finite) and acc is untouched, which
// for finite data is what the non-skipping form computes (fma(0, y, x) = x).  The test is one scalar load of a value no launch
// writes, so it is uniform over the wave, the block and the grid: no vote, and every wave of a block takes part in every
// cooperative tile load of the segments that do run.  All segments skipped: out = 0.
// Barrier: attn16_core_run ends on s_waitcnt vmcnt(0) with no barrier and its prologue requests tiles 0 and 1 into ring slots 0
// and 1 at once, so a block-wide barrier goes in front of a segment exactly when a PREVIOUS SEGMENT RAN on this ring (`ran`; not
// `r > 0`: segment 0 may be the skipped one).
// No atomics; the only stores are the T * H * 64 values of `out`, plain vector stores.  16-bit element types, D = 64 (fp32 and the
// other head sizes go S times through st_attention: ops.attention_segments).
#include "attention_sum.h"

struct SegTable { st_kv_segment s[REGIONS_MAX]; };

template <typename E>
__global__ __launch_bounds__(256) void attn_segments_kernel(const E* __restrict__ Q, const SegTable segs, int S,
                                                            const float* __restrict__ W, const float* __restrict__ SC,
                                                            E* __restrict__ O, int T, long ldq, long ldo, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) char lds[3 * 2 * ATT_KV * 128];
    const int t_ = threadIdx.x, lane = t_ & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t_ >> 6);
    const int head = blockIdx.y, b = blockIdx.z;
    const int row0 = blockIdx.x * 64;
    const int c16 = lane & 15, g = lane >> 4;
    const int row = row0 + wave * 16 + c16;                  // this lane's query row; rows >= T are clamped on load, not stored
    const E* Qb = Q + (size_t)b * T * ldq + (size_t)row0 * ldq + (size_t)head * ATT_D;
    const float* Wb = W + (size_t)b * S * T + min(row, T - 1);

    f32x4 acc[4], res[4];                                    // the weighted sum; res: the products' residuals (fused fp16 elements only)
#pragma unroll
    for (int db = 0; db < 4; ++db) { acc[db] = f32x4{0.f, 0.f, 0.f, 0.f}; res[db] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    bool ran = false;                                        // a previous segment ran on this block's ring
    for (int r = 0; r < S; ++r) {
        const float sc = SC ? SC[r] : 1.0f;                  // uniform: one scalar load
        if (sc == 0.0f) continue;                            // skipped by the whole grid; K / V of this segment are never read
        const float w = sc * Wb[(size_t)r * T];              // w_eff, one fp32 rounding
        if (ran) __builtin_amdgcn_s_barrier();               // every wave is done with the ring of the segment that ran before
        ran = true;
        const E* Kb = (const E*)segs.s[r].k + (size_t)b * segs.s[r].bsk + (size_t)head * ATT_D;
        const E* Vb = (const E*)segs.s[r].v + (size_t)b * segs.s[r].bsv + (size_t)head * ATT_D;
        attn16_core_run<E, 4>(Qb, ldq, T - row0, Kb, Vb, segs.s[r].ldk, segs.s[r].ldv, segs.s[r].len, scale_log2e, lds, wave, lane,
                              [&](const f32x4 (&o)[5], float inv, int, int) { regions_accumulate<E>(acc, res, o, inv, w); });
    }
    if (row < T) regions_store<E>(O + (size_t)b * T * ldo + (size_t)row * ldo + (size_t)head * ATT_D, acc, res, g);
}

template <typename E>
static int attention_segments_launch(const void* q, const SegTable& segs, int S, const float* w, const float* sc, void* out, int B, int T,
                                     int H, long ldq, long ldo, float scale, hipStream_t st) {
    hipLaunchKernelGGL((attn_segments_kernel<E>), dim3(cdiv(T, 64), H, B), dim3(256), 0, st, (const E*)q, segs, S, w, sc, (E*)out, T,
                       ldq, ldo, scale * 1.4426950408889634f);
    return st_check_launch("attention_segments");
}

extern "C" int st_attention_segments(const void* q, const st_kv_segment* segs, int S, const float* weights, const float* seg_scale,
                                     void* out, int B, int T, int H, int D, long ldq, long ldo, float scale, int dtype, void* stream) {
    ST_REQUIRE(q, "attention_segments: q is null");
    ST_REQUIRE(segs, "attention_segments: segs is null");
    ST_REQUIRE(weights, "attention_segments: weights is null");
    ST_REQUIRE(out, "attention_segments: out is null");
    ST_REQUIRE(B > 0 && T > 0 && H > 0, "attention_segments: bad shape B=%d T=%d H=%d", B, T, H);
    ST_REQUIRE(dtype == ST_BF16 || dtype == ST_F16, "attention_segments: dtype %d not supported (ST_BF16 or ST_F16)", dtype);
    ST_REQUIRE(D == ATT_D, "attention_segments: D (head_dim) %d not supported (only %d)", D, ATT_D);
    ST_REQUIRE(S >= 1 && S <= REGIONS_MAX, "attention_segments: S %d outside [1, %d]", S, REGIONS_MAX);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_segments: too many heads/batches for one launch (H=%d B=%d)", H, B);
    const long cols = (long)H * D;
    ST_REQUIRE(ldq % 8 == 0 && ldq >= cols, "attention_segments: ldq %ld must be a multiple of 8 elements (16-byte rows) and >= H*D", ldq);
    ST_REQUIRE(ldo % 4 == 0 && ldo >= cols, "attention_segments: ldo %ld must be a multiple of 4 elements and >= H*D", ldo);
    ST_REQUIRE((uintptr_t)q % 16 == 0, "attention_segments: q must be 16-byte aligned");
    ST_REQUIRE((uintptr_t)out % 16 == 0, "attention_segments: out must be 16-byte aligned");
    ST_REQUIRE((uintptr_t)weights % 4 == 0, "attention_segments: weights must be 4-byte aligned");
    ST_REQUIRE((uintptr_t)seg_scale % 4 == 0, "attention_segments: seg_scale must be 4-byte aligned");
    SegTable tab;
    for (int r = 0; r < REGIONS_MAX; ++r) tab.s[r] = st_kv_segment{nullptr, nullptr, 0, 0, 0, 0, 0};
    for (int r = 0; r < S; ++r) {
        const st_kv_segment& g = segs[r];
        ST_REQUIRE(g.k, "attention_segments: segment %d: k is null", r);
        ST_REQUIRE(g.v, "attention_segments: segment %d: v is null", r);
        ST_REQUIRE(g.len >= 1 && g.len < 256, "attention_segments: segment %d: len %d outside [1, 255]", r, g.len);
        ST_REQUIRE(g.ldk % 8 == 0 && g.ldk >= cols, "attention_segments: segment %d: ldk %ld must be a multiple of 8 elements (16-byte rows) and >= H*D", r, g.ldk);
        ST_REQUIRE(g.ldv % 8 == 0 && g.ldv >= cols, "attention_segments: segment %d: ldv %ld must be a multiple of 8 elements (16-byte rows) and >= H*D", r, g.ldv);
        ST_REQUIRE(g.bsk % 8 == 0 && g.bsk >= 0, "attention_segments: segment %d: bsk %ld must be a non-negative multiple of 8 elements", r, g.bsk);
        ST_REQUIRE(g.bsv % 8 == 0 && g.bsv >= 0, "attention_segments: segment %d: bsv %ld must be a non-negative multiple of 8 elements", r, g.bsv);
        ST_REQUIRE((uintptr_t)g.k % 16 == 0, "attention_segments: segment %d: k must be 16-byte aligned", r);
        ST_REQUIRE((uintptr_t)g.v % 16 == 0, "attention_segments: segment %d: v must be 16-byte aligned", r);
        tab.s[r] = g;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return attention_segments_launch<bf16>(q, tab, S, weights, seg_scale, out, B, T, H, ldq, ldo, scale, st);
    return attention_segments_launch<f16>(q, tab, S, weights, seg_scale, out, B, T, H, ldq, ldo, scale, st);
}
