// Flash attention at head_dim 512 for gfx950, bf16 and fp16: out = softmax(q k^T * scale) v per head.  The shape of the SDXL
// VAE decoder's middle-block self-attention: ONE head of 512 channels over every latent cell (T = S = 16 384 at a 128 x 128
// latent), so B * H is 1 or 2 and all parallelism comes from the query axis.  DESIGN 4r holds the arithmetic behind the form.
//
//   * a block owns 64 query rows (256 blocks at T = 16 384, one per CU) and has four waves, one per SIMD, each free to use the
//     whole 512-register budget.  Wave w = 2 rh + ch owns the 32 query rows of row half rh and the 256 channels of channel half ch
//     (v_mfma_f32_32x32x16): a 128-register O^T accumulator and 64 registers of Q fragments, not 256 + 128;
//   * scores are computed transposed and SPLIT OVER THE CONTRACTION: wave (rh, ch) multiplies its 32 rows with all 64 keys of the
//     tile over its own 256 channels only (32 MFMAs), the two partial S^T meet through LDS (8 KiB per wave, fp32, lane for lane:
//     partners share the row and the register layout), and both partners then hold the same full scores (a + b = b + a), run the same
//     softmax and use their P^T, straight from the score registers, as the B operand of O^T = V^T P^T over their own channels
//     (32 MFMAs + 4 for the row sums through a ones block).  Per 64 MFMAs a wave reads half the K tile and half the V tile;
//   * K and V tiles of 64 keys (64 KiB each: a key row is 1 024 bytes, exactly one wave-wide LDS-DMA instruction) alternate: the
//     V tile flies while K Q^T runs, the next K tile while V^T P^T runs.  Two barriers per tile, 128 KiB + 32 KiB of exchange = the
//     whole 160 KiB of LDS;
//   * rows are XOR-swizzled per 16-byte chunk on the DMA's source side, K by (key & 15) (sixteen keys of one ds_read_b128 group hit
//     sixteen different chunks), V by 4 (key & 3) (the four keys x 64 bytes of a half-wave's ds_read_b64_tr_b16 tile 256 bytes);
//   * lazy reference maximum, keys past S zero-filled and masked, rows past T clamped on the read and not stored.
#include "attention_core.h"

namespace {

constexpr int D512 = 512;
constexpr int D512_ROWS = 64;                          // query rows per block
constexpr int D512_ROW_B = D512 * 2;                   // bytes of a key row
constexpr int D512_TILE_B = ATT_KV * D512_ROW_B;       // one K (or V) tile
constexpr int D512_X_B = 32 * 64 * 4;                  // a wave's partial scores: 32 fp32 per lane
constexpr size_t D512_LDS = 2 * (size_t)D512_TILE_B + 4 * D512_X_B;

template <typename E>
__global__ __launch_bounds__(256) void attn_d512_kernel(const E* __restrict__ Q, const E* __restrict__ K, const E* __restrict__ V,
                                                        E* __restrict__ O, int T, int S, long ldq, long ldk, long ldv, long ldo,
                                                        float scale_log2e, int H) {
    typedef typename V16<E>::x8 E8;
    typedef typename V16<E>::x4 E4;
    extern __shared__ __attribute__((aligned(16))) char lds[];          // K tile | V tile | 4 x partial scores
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rh = wave >> 1, ch = wave & 1;
    const int r32 = lane & 31, h = lane >> 5;
    int b, head, xblk;
    att_xcd_decode<true>(T, D512_ROWS, H, b, head, xblk);
    const int q0 = xblk * D512_ROWS + rh * 32;
    const int qrow = min(q0 + r32, T - 1);
    const E* Kb = K + (size_t)b * S * ldk + (size_t)head * D512;
    const E* Vb = V + (size_t)b * S * ldv + (size_t)head * D512;
    const E* zeros = reinterpret_cast<const E*>(g_att_zero16);
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(att_lds_offset(lds));
    char* kimg = lds;
    char* vimg = lds + D512_TILE_B;
    f32x4* xmine = reinterpret_cast<f32x4*>(lds + 2 * D512_TILE_B + wave * D512_X_B) + lane;
    const f32x4* xpeer = reinterpret_cast<const f32x4*>(lds + 2 * D512_TILE_B + (wave ^ 1) * D512_X_B) + lane;

    // ---- Q fragments (B operand of S^T): channels 256 ch + 16 ks + 8 h .. + 7 of this lane's row, times scale * log2(e) --------
    E8 qf[16];
    {
        const E* qp = Q + (size_t)b * T * ldq + (size_t)qrow * ldq + (size_t)head * D512 + 256 * ch + 8 * h;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const E8 raw = *reinterpret_cast<const E8*>(qp + 16 * ks);
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[ks][j] = (E)((float)raw[j] * scale_log2e);
        }
    }
    E8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (E)(r32 == 0 ? 1.0f : 0.0f);

    // ---- LDS-DMA: a wave brings rows 16 wave .. + 15 of a tile, one instruction per row; lane L fetches the chunk that belongs at
    //      position L of the swizzled row.  Keys past S read the zero line. ----------------------------------------------------
    auto dma_tile = [&](const E* base, long ld, int kt, unsigned img, bool is_v) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = 16 * wave + i, key = kt * ATT_KV + row;
            const int c = lane ^ (is_v ? (i & 3) << 2 : i);                  // (row & 3) << 2 / row & 15: 16 | the wave's first row
            const E* src = key < S ? base + (size_t)key * ld + c * 8 : zeros;
            att_dma16(src, img + row * D512_ROW_B);
        }
    };
    // K fragment (A operand of S^T): key row r32 of a 32-key block, chunk 32 ch + 2 ks + h, at position chunk ^ (key & 15)
    const int k_row = r32 * D512_ROW_B + ch * 512;
    const int k_xor = (r32 & 15) << 4;
    // V^T fragment (A operand of O^T) by two transposed 4 x 16 block reads: this lane addresses key 4 h + q4 (+ 8) of a 16-key
    // step, channels 256 ch + 32 cb + 16 (lane bit 4) + 4 (lane & 3) .. + 3 - the key order of the P^T registers
    const int q4 = (lane & 15) >> 2;
    const int v_row = (4 * h + q4) * D512_ROW_B + ch * 512 + (((lane >> 4) & 1) << 5) + ((lane & 3) << 3);
    int v_off[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v_off[c] = v_row + ((c ^ q4) << 6);          // 64-byte block (cb & 3) at position (cb & 3) ^ (key & 3)

    f32x16 o[8], osum;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        osum[r] = 0.f;
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) o[cb][r] = 0.f;
    }
    float m_ref = 0.f;                                 // reference maximum of this lane's query row (base-2 exponent units)
    const int nkt = (S + ATT_KV - 1) / ATT_KV;

    dma_tile(Kb, ldk, 0, lds0, false);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        // ---- phase A: V(kt) flies; partial scores over this wave's 256 channels ---------------------------------------------
        dma_tile(Vb, ldv, kt, lds0 + D512_TILE_B, true);
        f32x16 s0, s1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int off = k_row + ((((2 * ks + h) & 15) << 4) ^ k_xor) + (ks >> 3) * 256;
            const E8 k0 = *reinterpret_cast<const E8*>(kimg + off);
            const E8 k1 = *reinterpret_cast<const E8*>(kimg + 32 * D512_ROW_B + off);
            s0 = AttMma<E>::m32(k0, qf[ks], s0);
            s1 = AttMma<E>::m32(k1, qf[ks], s1);
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            xmine[64 * r4] = f32x4{s0[4 * r4], s0[4 * r4 + 1], s0[4 * r4 + 2], s0[4 * r4 + 3]};
            xmine[64 * (4 + r4)] = f32x4{s1[4 * r4], s1[4 * r4 + 1], s1[4 * r4 + 2], s1[4 * r4 + 3]};
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // own rows of V(kt) have landed ...
        __syncthreads();                                            // ... and everyone's; K(kt) is dead, the partials are visible

        // ---- phase B: K(kt + 1) flies; full scores, softmax, O^T += V^T P^T over this wave's 256 channels ---------------------
        if (kt + 1 < nkt) dma_tile(Kb, ldk, kt + 1, lds0, false);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 a = xpeer[64 * r4], c = xpeer[64 * (4 + r4)];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                s0[4 * r4 + e] = (s0[4 * r4 + e] + a[e]) - m_ref;
                s1[4 * r4 + e] = (s1[4 * r4 + e] + c[e]) - m_ref;
            }
        }
        if ((kt + 1) * ATT_KV > S) {                               // mask the tail keys (only the last tile has any)
            const int kbase = kt * ATT_KV + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kbase + (r & 3) + 8 * (r >> 2);
                if (key >= S) s0[r] = -INFINITY;
                if (key + 32 >= S) s1[r] = -INFINITY;
            }
        }
        float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = att_max3(mx, s0[r], s1[r]);
        if (kt == 0 || __any(mx > ATT_LAG)) {
            // exact path: the row maximum (the row's keys sit in lanes r32 and r32 + 32) becomes the reference of every row that
            // is on its first tile or has outrun the lag; O and the row sum move by the same amount
            const float rmx = xmax32(mx);
            const float delta = ((kt == 0 || rmx > ATT_LAG) && rmx > -INFINITY) ? rmx : 0.f;
            const float alpha = kt == 0 ? 1.f : fast_exp2(-delta);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s0[r] -= delta; s1[r] -= delta;
                osum[r] *= alpha;
#pragma unroll
                for (int cb = 0; cb < 8; ++cb) o[cb][r] *= alpha;
            }
            m_ref += delta;
        }
#pragma unroll
        for (int st = 0; st < 4; ++st) {                           // 16 keys a step: score registers 8 (st & 1) .. + 7 of s0 / s1
            const f32x16& sx = st < 2 ? s0 : s1;
            const int e = 8 * (st & 1);
            const E8 pb = pack8<E>(fast_exp2(sx[e]), fast_exp2(sx[e + 1]), fast_exp2(sx[e + 2]), fast_exp2(sx[e + 3]),
                                   fast_exp2(sx[e + 4]), fast_exp2(sx[e + 5]), fast_exp2(sx[e + 6]), fast_exp2(sx[e + 7]));
            const char* vb = vimg + st * 16 * D512_ROW_B;
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                const int off = v_off[cb & 3] + (cb >> 2) * 256;
                o[cb] = AttMma<E>::m32(v_frag<E>(vb, off, off + 8 * D512_ROW_B), pb, o[cb]);
            }
            osum = AttMma<E>::m32(ones, pb, osum);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // own rows of K(kt + 1) have landed ...
        __syncthreads();                                            // ... and everyone's; V(kt) and the partials are dead
    }

    // row sum: row 0 of the ones block lives in register 0 of the lanes with h == 0
    const float l = __shfl(osum[0], r32, 64);
    const float inv = 1.0f / l;
    if (q0 + r32 < T) {
        E* orow = O + (size_t)b * T * ldo + (size_t)(q0 + r32) * ldo + (size_t)head * D512 + 256 * ch + 4 * h;
#pragma unroll
        for (int cb = 0; cb < 8; ++cb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                E4 a_;
#pragma unroll
                for (int e = 0; e < 4; ++e) a_[e] = (E)(o[cb][4 * g + e] * inv);
                *reinterpret_cast<E4*>(orow + 32 * cb + 8 * g) = a_;
            }
    }
}

template <typename E>
int launch(const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H, long ldq, long ldk, long ldv, long ldo,
           float c, hipStream_t st) {
    static unsigned long long lds_ok = 0;                                     // bit mask over device ordinals
    ensure_dynamic_lds(attn_d512_kernel<E>, D512_LDS, &lds_ok);
    const long grid = (long)cdiv(T, D512_ROWS) * H * B;
    ST_REQUIRE(grid < (1L << 31), "attention: too many blocks");
    hipLaunchKernelGGL((attn_d512_kernel<E>), dim3((unsigned)grid), dim3(256), D512_LDS, st, (const E*)q, (const E*)k, (const E*)v,
                       (E*)out, T, S, ldq, ldk, ldv, ldo, c, H);
    return st_check_launch("attention");
}

}      // namespace

// (entry: st_attention for head_dim 512, attention.hip)
int attention_d512_launch(int dtype, const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H,
                          long ldq, long ldk, long ldv, long ldo, float scale, hipStream_t st) {
    const float c = scale * 1.4426950408889634f;
    if (dtype == ST_BF16) return launch<bf16>(q, k, v, out, B, T, S, H, ldq, ldk, ldv, ldo, c, st);
    if (dtype == ST_F16) return launch<f16>(q, k, v, out, B, T, S, H, ldq, ldk, ldv, ldo, c, st);
    return st_fail("attention: head_dim 512 takes bf16 or fp16 tensors, not dtype %d", dtype);
}
