// Shared device code of the attention kernels (attention.hip) and of the GEMM that fuses the text-context attention into
// the query projection (gemm.hip).  Internal to csrc/.
#pragma once
#include "common.h"
#include <stdlib.h>

static inline int att_dev_env_int(const char* name, int dflt) {      // developer knobs: -DST_DEV_CONFIGS builds only
#ifdef ST_DEV_CONFIGS
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

static constexpr int ATT_D = 64;
static constexpr int ATT_KV = 64;          // keys per tile

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

typedef __attribute__((address_space(3))) void att_lds_void_t;
typedef __attribute__((address_space(1))) const void att_gbl_cvoid_t;

// LDS-DMA issue in assembly.  The builtin form makes hipcc 7.2 treat every later ds_read_b64_tr_b16 (an intrinsic it
// takes for a possible LDS store) as dependent on the DMA: it puts s_waitcnt vmcnt(0) in front of the first transposed
// read after each issue, i.e. the wave waits out the flight time of the tile it has just requested.  Issued from asm,
// the DMA is invisible to that pass and only the kernel's own counted waits apply.  lds_off: wave-uniform byte offset.
__device__ __forceinline__ void att_dma16(const void* src, unsigned lds_off) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds_off) : "memory", "m0");
}
__device__ __forceinline__ unsigned att_lds_offset(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)p;
}

// max / sum with the lane 32 (or 16) away, through v_permlane32_swap / v_permlane16_swap instead of a
// ds_bpermute: no LDS round trip and, above all, no s_waitcnt lgkmcnt(0) in the middle of the softmax
// (that wait also drains the V fragment reads still in flight).  After the swap of two copies of x a lane
// holds its own value in one register and its partner's in the other.  Inline asm: hipcc 7.2 folds the two
// results of the builtin into one value (the sum came out as 2x); s_nop 1 covers the VALU-write hazard.
__device__ __forceinline__ void att_swap32(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void att_swap16(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ float xmax32(float x) { float a = x, b = x; att_swap32(a, b); return fmaxf(a, b); }
__device__ __forceinline__ float xmax16(float x) { float a = x, b = x; att_swap16(a, b); return fmaxf(a, b); }
__device__ __forceinline__ float xsum32(float x) { float a = x, b = x; att_swap32(a, b); return a + b; }
__device__ __forceinline__ float xsum16(float x) { float a = x, b = x; att_swap16(a, b); return a + b; }


__device__ __forceinline__ int swz_k(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int swz_v(int row) { return ((row >> 1) & 1) << 2; }

static __device__ __attribute__((aligned(16))) unsigned int g_att_zero16[4] = {0u, 0u, 0u, 0u};
__device__ __forceinline__ int swz_k16(int row) { return row & 7; }
__device__ __forceinline__ int swz_v16(int row) { return ((row >> 1) & 3) << 1; }

// ---- 16-row kernel (v_mfma_f32_16x16x32_bf16), used for the 77-token text context: one wave owns 16 query rows -----
//   S^T[key][q] = K Q^T : A = K rows (lane: key = l&15, d = 32ks + 8g..), B = Q^T (lane: q = l&15, same d);
//                         D: lane (q = l&15, g = l>>4) holds keys 16kb + 4g + r
//   O^T[d][q]  += V^T P^T: B = P^T straight from the S registers of key blocks (2kp, 2kp+1): k-slot 8g + j <-> key
//                         32kp + 16(j>>2) + 4g + (j&3); A = V^T through two transposed 4x16 block reads per fragment
//                         that follow the same key order.
// The softmax is cut to what the VALU cannot avoid.  At D = 64 the kernel is bound by the softmax arithmetic, not by the matrix pipe (per 16 x 64 score tile a wave
// issues 16-18 MFMAs = 290 pipe cycles, and the classic online softmax ~100 VALU instructions = 450 issue cycles).
// What is left here per score: one v_exp_f32, half a v_max3_f32, half a v_cvt_pk_bf16_f32:
//   * Q is pre-multiplied by scale * log2(e) once (bf16, like every MFMA operand), so scores are base-2 exponents;
//   * the S accumulators start at -m_ref (the row's reference maximum) instead of 0: the MFMA chain delivers
//     s - m_ref and the exponent needs no subtraction;
//   * m_ref follows the true row maximum lazily: a tile whose scores stay below m_ref + 2^ATT_LAG keeps it (softmax is
//     shift invariant; P <= 2^ATT_LAG is as exact in bf16 / fp32 as P <= 1); the first tile, and any tile that
//     exceeds the lag, takes the exact path (row maximum across lanes, rescale O, shift the pending scores);
//   * the row sums come out of the matrix pipe: a fifth "d block" of V^T that is 1 in its first row adds
//     sum_k P[k][q] to an accumulator (two MFMAs per tile instead of sixteen VALU adds), and being an accumulator
//     like O it is rescaled with O;
//   * the next tile's K Q^T is issued before this tile's softmax (runs under it).
// K/V tiles of 64 keys arrive by LDS-DMA into a ring of three swizzled buffers, one barrier per tile (the text context
// is two tiles: both are requested in the prologue).
// TAG only gives the cross-attention instantiation its own kernel name (profiles split the two).
static constexpr float ATT_LAG = 6.0f;

// V^T fragments through the compiler's own transposed LDS read (it places the two 8-byte halves of an MFMA operand
// in adjacent registers and counts the reads itself; the inline-asm form needed a v_mov per half)
// (the 16-bit-integer form of the builtin: the read moves bits, so one form serves bf16 and f16)
typedef __attribute__((ext_vector_type(4))) short att_s16x4;
typedef __attribute__((ext_vector_type(8))) short att_s16x8;
typedef __attribute__((address_space(3))) att_s16x4 att_lds_s16x4;
template <typename E>
__device__ __forceinline__ typename V16<E>::x8 v_frag(const char* lds_base, int off_lo, int off_hi) {
    const att_s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s16x4*)(lds_base + off_lo));
    const att_s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((att_lds_s16x4*)(lds_base + off_hi));
    return __builtin_bit_cast(typename V16<E>::x8, (att_s16x8)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}
// eight probabilities -> one MFMA operand: four packed conversions (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32)
template <typename E>
__device__ __forceinline__ typename V16<E>::x8 pack8(float a0, float a1, float a2, float a3, float a4, float a5, float a6, float a7) {
    typename V16<E>::x8 r;
    r[0] = (E)a0; r[1] = (E)a1; r[2] = (E)a2; r[3] = (E)a3; r[4] = (E)a4; r[5] = (E)a5; r[6] = (E)a6; r[7] = (E)a7;
    return r;
}
// the two MFMA shapes of the attention kernels, per 16-bit element type (same cycles for bf16 and f16)
template <typename E> struct AttMma;
template <> struct AttMma<bf16> {
    static __device__ __forceinline__ f32x4 m16(const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x16 m32(const bf16x8& a, const bf16x8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct AttMma<f16> {
    static __device__ __forceinline__ f32x4 m16(const f16x8& a, const f16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ f32x16 m32(const f16x8& a, const f16x8& b, const f32x16& c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// Three-way maximum, deliberately NOT inline asm: the scores it reads come straight out of MFMAs, and the hardware does
// not interlock an MFMA result against a VALU read - the compiler inserts the wait states, but only for instructions it
// can see.  An asm v_max3_f32 here read accumulators that were still being written whenever the matrix pipe was shared
// with another kernel (tools/att_race.py: output changed by 1 ulp when a second stream kept the CUs busy).
__device__ __forceinline__ float att_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// The body of the 16-row kernel as a device function, so that the GEMM that projects the queries of the text-context
// attention can run it as its epilogue on the Q tile it has just left in LDS (gemm.hip, st_ln_linear_xattn).
//   Qb / Ob: row 0 of this block's NW*16 queries / outputs of ONE head (global or LDS for Qb); rows >= q_rows are clamped,
//   rows >= o_rows not stored; Kb / Vb: key 0 of that head; lds: 3 * 16 KiB ring, 16-byte aligned.
// attn16_core_run is that body with the output left to the caller: `emit(o, inv, row, g)` receives the lane's un-normalised
// O^T registers (d = 16 db + 4 g + e of query `row` of the block), and inv = 1 / row sum; attn16_core, below it, stores
// (E)(o * inv).  The regional kernel (attention_regions.hip) runs the body once per key segment and keeps the fp32 result.
// The body ends on s_waitcnt vmcnt(0) WITHOUT a barrier: a caller that runs it again on the same ring puts one in between.
template <typename E, int NW, typename EMIT>
__device__ __forceinline__ void attn16_core_run(const E* Qb, long ldq, int q_rows, const E* Kb, const E* Vb, long ldk, long ldv,
                                                int S, float scale_log2e, char* lds, int wave, int lane, EMIT&& emit) {
    typedef typename V16<E>::x8 E8;
    constexpr int TILE_B = ATT_KV * 128;
    constexpr int BUF_B = 2 * TILE_B;
    constexpr int PIECES = 16 / NW;
    static_assert(NW <= 16 && 16 % NW == 0, "waves must divide the 16 DMA pieces of a tile");
    const int c16 = lane & 15, g = lane >> 4;
    const int q0 = wave * 16;
    const int qrow = min(q0 + c16, q_rows - 1);
    const E* zeros = reinterpret_cast<const E*>(g_att_zero16);

    E8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const E8 raw = *reinterpret_cast<const E8*>(Qb + (size_t)qrow * ldq + 32 * ks + 8 * g);
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (E)((float)raw[j] * scale_log2e);
    }
    // V^T "row 64": ones for the lanes that hold d = 0 of the extra block, zeros elsewhere
    E8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (E)(c16 == 0 ? 1.0f : 0.0f);

    // LDS-DMA sources: one running pointer per piece, advanced by 64 keys per tile (no per-tile address arithmetic);
    // only a tile that reaches past S takes the checked form (rows beyond S read a zero line)
    const int lr = lane >> 3, pc = lane & 7;
    const E* dsrc[PIECES];
    long dstep[PIECES];
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
        const int pce = wave * PIECES + i;
        const int isv = pce >> 3, row = (pce & 7) * 8 + lr;
        const int c = pc ^ (isv ? swz_v16(row) : swz_k16(row));
        dsrc[i] = isv ? Vb + (size_t)row * ldv + c * 8 : Kb + (size_t)row * ldk + c * 8;
        dstep[i] = (long)ATT_KV * (isv ? ldv : ldk);
    }
    auto dma_tile = [&](int kt, int buf) {           // tiles are issued in order: kt = 0, 1, 2, ...
        const bool tail = (kt + 1) * ATT_KV > S;
#pragma unroll
        for (int i = 0; i < PIECES; ++i) {
            const int pce = wave * PIECES + i;
            const int isv = pce >> 3, rb = pce & 7;
            const E* src = dsrc[i];
            if (tail && kt * ATT_KV + rb * 8 + lr >= S) src = zeros;
            __builtin_amdgcn_global_load_lds((att_gbl_cvoid_t*)src, (att_lds_void_t*)(lds + buf * BUF_B + isv * TILE_B + rb * 1024), 16, 0, 0);
            dsrc[i] += dstep[i];
        }
    };
    const int k_off0 = c16 * 128 + (((0 + g) ^ swz_k16(c16)) << 4);
    const int k_off1 = c16 * 128 + (((4 + g) ^ swz_k16(c16)) << 4);
    const int vkey = 4 * g + (c16 >> 2);
    const int vsw = swz_v16(vkey);
    const int vrow = vkey * 128 + 8 * (c16 & 1);
    const int vbit = (c16 & 3) >> 1;
    const int v_off0 = vrow + (((0 ^ vsw) + vbit) << 4), v_off1 = vrow + (((2 ^ vsw) + vbit) << 4);
    const int v_off2 = vrow + (((4 ^ vsw) + vbit) << 4), v_off3 = vrow + (((6 ^ vsw) + vbit) << 4);

    float m_ref = 0.f;                                // reference maximum of this lane's query row (base-2 exponent units)
    auto qk_tile = [&](int buf, f32x4 (&s)[4]) {
        const char* kb_ = lds + buf * BUF_B;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const E8 ka = *reinterpret_cast<const E8*>(kb_ + kb * 2048 + k_off0);
            const E8 kc = *reinterpret_cast<const E8*>(kb_ + kb * 2048 + k_off1);
            f32x4 acc = {-m_ref, -m_ref, -m_ref, -m_ref};
            acc = AttMma<E>::m16(ka, qf[0], acc);
            s[kb] = AttMma<E>::m16(kc, qf[1], acc);
        }
    };

    f32x4 o[5];                                       // O^T d blocks 0..3; o[4] row 0 = running row sum
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkt = (S + ATT_KV - 1) / ATT_KV;

    dma_tile(0, 0);
    if (nkt > 1) dma_tile(1, 1);
    if (nkt > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    f32x4 sa[4], sb[4];                               // scores of the current / next tile, trading places every trip
    qk_tile(0, sa);

    // one trip: tile kt (scores in `s`, V in buffer cur); leaves the scores of tile kt+1 in `sn`
    auto trip = [&](f32x4 (&s)[4], f32x4 (&sn)[4], int kt, int cur, int nb, int fb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // own pieces of tile kt+1 have landed ...
        __builtin_amdgcn_s_barrier();                              // ... and everyone's; tile kt-1 is dead
        if (kt + 2 < nkt) dma_tile(kt + 2, fb);
        // V^T fragments of this tile [key pair-block kp][d block]: issued now, first used after the softmax
        E8 vf[2][4];
        {
            const char* vb = lds + cur * BUF_B + TILE_B;
#pragma unroll
            for (int kp = 0; kp < 2; ++kp) {
                vf[kp][0] = v_frag<E>(vb, v_off0 + kp * 4096, v_off0 + kp * 4096 + 2048);
                vf[kp][1] = v_frag<E>(vb, v_off1 + kp * 4096, v_off1 + kp * 4096 + 2048);
                vf[kp][2] = v_frag<E>(vb, v_off2 + kp * 4096, v_off2 + kp * 4096 + 2048);
                vf[kp][3] = v_frag<E>(vb, v_off3 + kp * 4096, v_off3 + kp * 4096 + 2048);
            }
        }
        // scores of the next tile: the matrix pipe works on them under this softmax (after the last tile the ring
        // slot holds an old tile: computed all the same, never used)
        qk_tile(nb, sn);
        if ((kt + 1) * ATT_KV > S) {                               // mask the tail keys (only the last tile has any)
            const int kbase = kt * ATT_KV + 4 * g;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kbase + 16 * kb + r >= S) s[kb][r] = -INFINITY;
        }
        float mx = att_max3(s[0][0], s[0][1], s[0][2]);
        mx = att_max3(mx, s[0][3], s[1][0]);
        mx = att_max3(mx, s[1][1], s[1][2]);
        mx = att_max3(mx, s[1][3], s[2][0]);
        mx = att_max3(mx, s[2][1], s[2][2]);
        mx = att_max3(mx, s[2][3], s[3][0]);
        mx = att_max3(mx, s[3][1], s[3][2]);
        mx = fmaxf(mx, s[3][3]);
        if (kt == 0 || __any(mx > ATT_LAG)) {
            // exact path: the row maximum (over the four lanes that share the row) becomes the reference of every row
            // that is on its first tile or has outrun the lag; everything already expressed against the old reference
            // (O, the row sum, this tile's and the next tile's scores) moves by the same amount
            const float rmx = xmax32(xmax16(mx));
            const float delta = ((kt == 0 || rmx > ATT_LAG) && rmx > -INFINITY) ? rmx : 0.f;
            const float alpha = kt == 0 ? 1.f : fast_exp2(-delta);      // (nothing to rescale on the first tile; delta may be very negative there)
#pragma unroll
            for (int kb = 0; kb < 4; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) { s[kb][r] -= delta; sn[kb][r] -= delta; }
#pragma unroll
            for (int db = 0; db < 5; ++db)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[db][r] *= alpha;
            m_ref += delta;
        }
#pragma unroll
        for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kb][r] = fast_exp2(s[kb][r]);
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) {
            const E8 pb = pack8<E>(s[2 * kp][0], s[2 * kp][1], s[2 * kp][2], s[2 * kp][3],
                                    s[2 * kp + 1][0], s[2 * kp + 1][1], s[2 * kp + 1][2], s[2 * kp + 1][3]);
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db] = AttMma<E>::m16(vf[kp][db], pb, o[db]);
            o[4] = AttMma<E>::m16(ones, pb, o[4]);
        }
    };
    int cur = 0;
    for (int kt = 0; kt < nkt; kt += 2) {
        const int b1 = cur == 2 ? 0 : cur + 1, b2 = b1 == 2 ? 0 : b1 + 1;
        trip(sa, sb, kt, cur, b1, b2);
        if (kt + 1 < nkt) trip(sb, sa, kt + 1, b1, b2, cur);
        cur = b2;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // row sum: row 0 of the extra block lives in register 0 of the lanes with g == 0
    const float l = __shfl(o[4][0], c16, 64);
    const float inv = 1.0f / l;
    emit(o, inv, q0 + c16, g);
}

template <typename E, int NW>
__device__ __forceinline__ void attn16_core(const E* Qb, long ldq, int q_rows, const E* Kb, const E* Vb, long ldk, long ldv,
                                            int S, E* Ob, long ldo, int o_rows, float scale_log2e, char* lds, int wave, int lane) {
    typedef typename V16<E>::x4 E4;
    attn16_core_run<E, NW>(Qb, ldq, q_rows, Kb, Vb, ldk, ldv, S, scale_log2e, lds, wave, lane,
                           [&](const f32x4 (&o)[5], float inv, int row, int g) {
        if (row < o_rows) {
            E* orow = Ob + (size_t)row * ldo;
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                E4 a_;
#pragma unroll
                for (int e = 0; e < 4; ++e) a_[e] = (E)(o[db][e] * inv);
                *reinterpret_cast<E4*>(orow + 16 * db + 4 * g) = a_;
            }
        }
    });
}

// ---- 1-D XCD-aware grid of the self-attention kernels ---------------------------------------------------------------
// Consecutive block ids go round-robin to the eight XCDs, so XCD c takes the c-th contiguous eighth of the (batch, head,
// query block) list - the query blocks of one head (they all stream that head's K and V) meet in one L2 instead of eight
// (HBM-side bytes of the 4096-token launch: 4.5x the algorithmic bytes before).  rows = query rows per block.
// UNIFORM: say that the results are wave-uniform (the divisions run on the VALU); a kernel chooses per its register budget.
template <bool UNIFORM>
__device__ __forceinline__ void att_xcd_decode(int T, int rows, int H, int& b, int& head, int& xblk) {
    const int nb = gridDim.x, bid = blockIdx.x;
    const int xq = nb >> 3, xr = nb & 7, xcd = bid & 7;
    const int w = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    const int gx = (T + rows - 1) / rows;
    const int hb = w / gx;
    xblk = w - hb * gx;
    b = hb / H;
    head = hb - b * H;
    if constexpr (UNIFORM) {
        xblk = __builtin_amdgcn_readfirstlane(xblk);
        b = __builtin_amdgcn_readfirstlane(b);
        head = __builtin_amdgcn_readfirstlane(head);
    }
}

// ---- 32-row kernel, interleaved: softmax instructions placed in the gaps between the MFMAs of the same wave ----------
// At D = 64 a 64-key tile costs a wave 20 MFMAs (640 pipe cycles) and ~80 VALU instructions, 32 of them v_exp_f32 at
// 8 issue cycles: ~420 cycles of vector issue, which fit the 24 free issue cycles of each MFMA gap only if they are
// PLACED there (a wave issues in order: eight MFMAs in a row stall it at the second one, and the VALU behind them
// waits).  One trip of this kernel is a single scheduling region, pinned gap by gap with sched_barrier:
//     QK phase, 8 MFMAs  K(t+1) Q^T -> next scores   | exp + pack of the first half of tile t | V^T(t) fragment reads
//     PV phase, 12 MFMAs V^T(t) P(t) (+ ones block)  | exp + pack of the second half, max of the next scores | K(t+2) reads
// then the counted DMA wait, one block barrier, and the (rare) branch that moves the lazy maximum.  Because P(t) is
// multiplied in the trip that exponentiates it, nothing is pending when the maximum moves.
//
// attn32i_core is that body as a device function with the one varying part, where a key row comes from, passed in:
// attn32i_kernel (attention.hip) runs it on one K / V, attnj32i_kernel (attention_joint.hip) on two under one softmax.
//   Qb / Ob: row 0 of this (batch entry, head)'s T queries / outputs; xblk: the block's index among the blocks of 32 NW
//   query rows, wave w owns rows 32 (xblk NW + w) .. + 31 (rows >= T are clamped on the read and not stored); lds: ATT32_RING
//   bytes of dynamic LDS, 16-byte aligned; NW compute waves, and with LD one more (wave == NW) that issues every DMA of every
//   tile and returns from the core without storing.
// Wave and lane are read from threadIdx.x HERE, not passed in: as parameters the compiler simplifies the lane arithmetic of
// the function on its own, before it is inlined, and then no longer sees k_off[ks][1] = k_off[ks][0] + 4096 (the offset
// field of the K fragment reads): four more VGPRs in every form.
// The core owns the six-slot ring, the barrier sequence and the counted vmcnt waits, the Q loads, the swizzled fragment
// offsets, mask_tail, the lazy maximum, the 20-MFMA trip and the normalised store.  KEYS supplies:
//   keys.S                       total keys of this block: the tile count and mask_tail read it;
//   keys.seed(first, lr, pc)     running pointers of the lane's 16-byte piece (row lr of 8, chunk pc) of pieces first ..
//                                first + KEYS::N - 1 of tile 0 (piece p: V if p >> 3, key rows 8 (p & 7) .. + 7, source
//                                chunk pc ^ swz_v / swz_k(row)); N = 16 for the loader wave (first = 0), else 16 / NW;
//   keys.load_tile(kt, slot)     LD: the sixteen pieces of tile kt (< the tile count) to LDS byte offset slot;
//   keys.load_piece(kt, i, p, slot, dump, live)   !LD: piece p = first + i of tile kt to slot, or, when !live (kt is past
//                                the last tile), any 16 readable bytes to dump.
// ROWS is the second rule, where a token comes from: rows(r) = the token (in units of ldq / ldo from Qb / Ob) of query / output row r
// of this (batch entry, head).  The identity for attn32i_kernel and attnj32i_kernel; attnw32i_kernel (attention_windows.hip) maps
// a window row to its place in the token grid.  Evaluated twice per lane, both outside the key loop.
// Tiles are asked for in order kt = 0, 1, 2, ... and every piece of a tile exactly once, a wave's pieces in order i = 0, 1, ... N - 1
// (a rule may keep running state that it steps at a tile's last piece: AttKeysWin does), keys >= S as a zero line.  THE
// INVARIANT THE WAITS REST ON: load_tile issues exactly sixteen att_dma16 on every path and load_piece exactly one, and
// neither issues any other vector-memory instruction; piece p lands at slot + att32_piece_off(p).
static constexpr int ATT32_SLOTS = 6;                                        // ring slots of one (K, V) tile pair
static constexpr int ATT32_TILE_B = ATT_KV * 128, ATT32_BUF_B = 2 * ATT32_TILE_B;
static constexpr size_t ATT32_RING = ATT32_SLOTS * ATT32_BUF_B + 1024;       // + the dump line of the dummy DMAs
__device__ __forceinline__ unsigned att32_piece_off(int p) { return (p >> 3) * ATT32_TILE_B + (p & 7) * 1024; }

struct AttRowsId {                                     // the row rule of the two kernels whose queries are a contiguous token run
    __device__ __forceinline__ int operator()(int r) const { return r; }
};

template <typename E, int NW, bool LD, typename KEYS, typename ROWS = AttRowsId>
__device__ __forceinline__ void attn32i_core(const E* Qb, long ldq, int T, int xblk, E* Ob, long ldo, float scale_log2e,
                                             char* lds, KEYS& keys, const ROWS rows = ROWS()) {
    typedef typename V16<E>::x8 E8;
    typedef typename V16<E>::x4 E4;
    constexpr int TILE_B = ATT32_TILE_B, BUF_B = ATT32_BUF_B, RB = ATT32_SLOTS;
    constexpr int PIECES = 16 / NW;
    const int S = keys.S;
    const int t_ = threadIdx.x, lane = t_ & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t_ >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    const int q0 = (xblk * NW + wave) * 32;
    const int qrow = min(q0 + r32, T - 1);

    const int nkt = (S + ATT_KV - 1) / ATT_KV;
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(att_lds_offset(lds));
    if constexpr (LD) {
        // ---- loader wave (wave NW): with one wave per SIMD nobody multiplies while a compute wave queues in the load path
        //      (16 wave-instructions of 1 KiB per tile, 16 cycles each), so one extra wave issues every piece of every tile and
        //      the compute waves issue none.  It keeps the compute waves' barrier sequence: three in the prologue (tile 0, 1, 2
        //      landed), then one per trip (tile kt+3 landed, tile kt+4 in flight).
        if (wave == NW) {
            keys.seed(0, lane >> 3, lane & 7);
            int slot_i = 0;
            auto load_tile = [&](int kt) __attribute__((always_inline)) {            // tile kt (< nkt) into the next ring slot
                keys.load_tile(kt, lds0 + slot_i * BUF_B);
                slot_i = slot_i == RB - 1 ? 0 : slot_i + 1;
            };
            // prologue: tiles 0..2 requested, barrier when tile 0 / 1 / 2 has landed; tile 3 joins after the first barrier
            // (at most 48 DMAs in flight: the vmcnt immediate ends at 63)
            const int n0 = min(nkt, 3);
            for (int kt = 0; kt < n0; ++kt) load_tile(kt);
            if (n0 == 3) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
            else if (n0 == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (nkt > 3) { load_tile(3); asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); }      // tile 1 landed (2, 3 fly)
            else if (n0 == 3) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (nkt > 3) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");                          // tile 2 landed (3 flies)
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            for (int kt = 0; kt < nkt; ++kt) {
                if (kt + 4 < nkt) { load_tile(kt + 4); asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); }   // tile kt+3 landed
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            return;
        }
    }

    // Q through asm loads: a compiler-counted wait would not know about the DMAs issued behind them and would drain those too
    typedef unsigned int q_raw_t __attribute__((ext_vector_type(4)));
    q_raw_t qraw[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(qraw[ks]) : "v"(Qb + (size_t)rows(qrow) * ldq + 16 * ks + 8 * h) : "memory");
    E8 qf[4];
    E8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (E)(r32 == 0 ? 1.0f : 0.0f);

    if constexpr (!LD) keys.seed(wave * PIECES, lane >> 3, lane & 7);
    // tiles are issued in order; past the last tile the pieces become dummies (a zero line into the dump area) so that
    // every trip issues the same number of DMAs and the counted waits stay valid
    int dbuf = 0;
    const unsigned dump_off = lds0 + RB * BUF_B;
    auto dma_piece = [&](int kt, int i) __attribute__((always_inline)) {             // piece i of tile kt into ring slot dbuf
        if constexpr (!LD) keys.load_piece(kt, i, wave * PIECES + i, lds0 + dbuf * BUF_B, dump_off, kt < nkt);      // (LD: the loader wave issues them)
    };
    auto dma_next = [&]() { dbuf = dbuf == RB - 1 ? 0 : dbuf + 1; };
    auto dma_tile = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PIECES; ++i) dma_piece(kt, i);
        dma_next();
    };
    int v_base0, v_base1;
    {
        const int q4 = (lane & 15) >> 2;
        const int key = 4 * h + q4;
        const int ch0 = 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1);
        const int row = key * 128 + 8 * (lane & 1);
        v_base0 = row + ((ch0 ^ swz_v(key)) << 4);
        v_base1 = row + (((ch0 + 4) ^ swz_v(key)) << 4);
    }
    int k_off[4][2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const int c = 2 * ks + h;
        k_off[ks][0] = r32 * 128 + ((c ^ swz_k(r32)) << 4);
        k_off[ks][1] = (32 + r32) * 128 + ((c ^ swz_k(32 + r32)) << 4);
    }
    f32x16 negm;                                       // -m_ref of this lane's query row in every register: the C operand of a tile's first MFMAs
    f32x16 o0 = {0}, o1 = {0}, o2 = {0};
    E8 kf0[4], kf1[4], vf[4][2], pb[4];
    auto mask_tail = [&](f32x16& s0, f32x16& s1, int kt) {
        const int kbase = kt * ATT_KV + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kbase + (r & 3) + 8 * (r >> 2);
            if (key >= S) s0[r] = -INFINITY;
            if (key + 32 >= S) s1[r] = -INFINITY;
        }
    };
    auto max32 = [&](const f32x16& s0, const f32x16& s1) {
        float ma = att_max3(s0[0], s0[1], s0[2]), mb = att_max3(s0[8], s0[9], s0[10]);
        float mc = att_max3(s1[0], s1[1], s1[2]), md = att_max3(s1[8], s1[9], s1[10]);
        ma = att_max3(ma, s0[3], s0[4]); mb = att_max3(mb, s0[11], s0[12]); mc = att_max3(mc, s1[3], s1[4]); md = att_max3(md, s1[11], s1[12]);
        ma = att_max3(ma, s0[5], s0[6]); mb = att_max3(mb, s0[13], s0[14]); mc = att_max3(mc, s1[5], s1[6]); md = att_max3(md, s1[13], s1[14]);
        ma = att_max3(ma, s0[7], mb); mc = att_max3(mc, s1[7], md);
        return att_max3(ma, s0[15], att_max3(mc, s1[15], mc));
    };

    // prologue: four tiles in flight, the first three landed; exact scores of tile 0; K fragments of tile 1
    dma_tile(0); dma_tile(1); dma_tile(2); dma_tile(3);
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(qraw[0]), "+v"(qraw[1]), "+v"(qraw[2]), "+v"(qraw[3]) : "n"(LD ? 0 : 3 * PIECES) : "memory");   // Q and tile 0: start on them while the others fly
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const E8 raw = __builtin_bit_cast(E8, qraw[ks]);
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (E)((float)raw[j] * scale_log2e);
    }
    f32x16 sa0, sa1, sb0, sb1;
    {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf0[ks] = *reinterpret_cast<const E8*>(lds + k_off[ks][0]);
            kf1[ks] = *reinterpret_cast<const E8*>(lds + k_off[ks][1]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) { sa0[r] = 0.f; sa1[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            sa0 = AttMma<E>::m32(kf0[ks], qf[ks], sa0);
            sa1 = AttMma<E>::m32(kf1[ks], qf[ks], sa1);
        }
        if (ATT_KV > S) mask_tail(sa0, sa1, 0);
        const float rmx = xmax32(max32(sa0, sa1));
        const float m0 = rmx > -INFINITY ? rmx : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sa0[r] -= m0; sa1[r] -= m0; negm[r] = -m0; }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PIECES) : "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            kf0[ks] = *reinterpret_cast<const E8*>(lds + BUF_B + k_off[ks][0]);
            kf1[ks] = *reinterpret_cast<const E8*>(lds + BUF_B + k_off[ks][1]);
        }
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");           // tile 2: its K fragments are read in the first trip
        __builtin_amdgcn_s_barrier();
    }

    int vslot = 0, kslot = 2;                         // ring slots of tile kt (V^T) and tile kt+2 (K)
    auto trip = [&](f32x16& s0, f32x16& s1, f32x16& n0, f32x16& n1, int kt) __attribute__((always_inline)) {
        const char* vb = lds + vslot * BUF_B + TILE_B;
        const char* kb = lds + kslot * BUF_B;
        float mch[4];                                  // four maximum chains over the next tile's scores
        // ---- QK phase: gap g carries MFMA g, two exponentials + their pack, one V^T fragment (two transposed reads) ----
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int ks = g >> 1;
            if ((g & 1) == 0) n0 = AttMma<E>::m32(kf0[ks], qf[ks], ks == 0 ? negm : n0);
            else              n1 = AttMma<E>::m32(kf1[ks], qf[ks], ks == 0 ? negm : n1);
            const float e0 = fast_exp2(s0[2 * g]), e1 = fast_exp2(s0[2 * g + 1]);
            pb[g >> 2][2 * (g & 3)] = (E)e0; pb[g >> 2][2 * (g & 3) + 1] = (E)e1;
            vf[g >> 1][g & 1] = v_frag<E>(vb, ((g & 1) ? v_base1 : v_base0) + (g >> 1) * 2048, ((g & 1) ? v_base1 : v_base0) + (g >> 1) * 2048 + 1024);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- PV phase: gap p carries MFMA p; gaps 0-7 the other sixteen exponentials, gaps 2-11 the maximum of the next
        //      tile's scores, gaps 4-11 the K fragments of tile kt+2 ----
#pragma unroll
        for (int p = 0; p < 12; ++p) {
            const int s_ = p / 3, w = p % 3;
            if (w == 0)      o0 = AttMma<E>::m32(vf[s_][0], pb[s_], o0);
            else if (w == 1) o1 = AttMma<E>::m32(vf[s_][1], pb[s_], o1);
            else             o2 = AttMma<E>::m32(ones, pb[s_], o2);
            if (p < 8) {
                const float e0 = fast_exp2(s1[2 * p]), e1 = fast_exp2(s1[2 * p + 1]);
                pb[2 + (p >> 2)][2 * (p & 3)] = (E)e0; pb[2 + (p >> 2)][2 * (p & 3) + 1] = (E)e1;
            }
            if (p >= 2 && p < 6) {                     // one chain start per gap
                const int c = p - 2;
                const f32x16& sx = c < 2 ? n0 : n1;
                const int e = 8 * (c & 1);
                mch[c] = att_max3(sx[e], sx[e + 1], sx[e + 2]);
            }
            if (p >= 6 && p < 8) {
#pragma unroll
                for (int c = 2 * (p - 6); c < 2 * (p - 6) + 2; ++c) {
                    const f32x16& sx = c < 2 ? n0 : n1;
                    const int e = 8 * (c & 1);
                    mch[c] = att_max3(mch[c], sx[e + 3], sx[e + 4]);
                }
            }
            if (p >= 8) {
                const int c = p - 8;
                const f32x16& sx = c < 2 ? n0 : n1;
                const int e = 8 * (c & 1);
                mch[c] = att_max3(mch[c], sx[e + 5], sx[e + 6]);
                mch[c] = att_max3(mch[c], sx[e + 7], sx[e + 7]);
            }
            // LDS-DMA of tile kt+4 (spreading the pieces over the gaps by wave was tried: the per-gap branches cost more
            // than the queueing of sixteen simultaneous wave-instructions in the CU's load path)
            if (p >= 12 - PIECES) dma_piece(kt + 4, p - (12 - PIECES));
            if (p >= 4) {
                const int i = p - 4, ks = i >> 1;
                if ((i & 1) == 0) kf0[ks] = *reinterpret_cast<const E8*>(kb + k_off[ks][0]);
                else              kf1[ks] = *reinterpret_cast<const E8*>(kb + k_off[ks][1]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float mx = att_max3(mch[0], mch[1], att_max3(mch[2], mch[3], mch[3]));
        vslot = vslot == RB - 1 ? 0 : vslot + 1;
        kslot = kslot == RB - 1 ? 0 : kslot + 1;
        if (kt + 1 < nkt) {
            if ((kt + 2) * ATT_KV > S) { mask_tail(n0, n1, kt + 1); mx = max32(n0, n1); }
            if (__any(mx > ATT_LAG)) {
                // a row outran the lag: move its reference maximum (nothing is pending: P of this trip is already in O)
                const float rmx = xmax32(mx);
                const float delta = (rmx > ATT_LAG && rmx > -INFINITY) ? rmx : 0.f;
                const float alpha = fast_exp2(-delta);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    n0[r] -= delta; n1[r] -= delta; negm[r] -= delta;
                    o0[r] *= alpha; o1[r] *= alpha; o2[r] *= alpha;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES) : "memory");   // own pieces of tile kt+3 have landed; tile kt+4's may fly
        dma_next();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    for (int kt = 0; kt < nkt; kt += 2) {
        trip(sa0, sa1, sb0, sb1, kt);
        if (kt + 1 < nkt) trip(sb0, sb1, sa0, sa1, kt + 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    const float l = __shfl(o2[0], r32, 64);
    const float inv = 1.0f / l;
    if (q0 + r32 < T) {
        E* orow = Ob + (size_t)rows(q0 + r32) * ldo;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            E4 a_, c_;
#pragma unroll
            for (int e = 0; e < 4; ++e) { a_[e] = (E)(o0[4 * g + e] * inv); c_[e] = (E)(o1[4 * g + e] * inv); }
            *reinterpret_cast<E4*>(orow + 8 * g + 4 * h) = a_;
            *reinterpret_cast<E4*>(orow + 32 + 8 * g + 4 * h) = c_;
        }
    }
}

// One key source (st_attention): a running pointer per piece, advanced by 64 keys per tile (no per-tile address
// arithmetic); only a tile that reaches past S takes the checked form (rows beyond S read the zero line).
template <typename E, int NW, bool LD>
struct AttKeys1 {
    static constexpr int N = LD ? 16 : 16 / NW;
    const E *Kb, *Vb;                                  // key 0 of this (batch entry, head)
    long ldk, ldv;
    int S;
    const E* src[N];
    long step[N];
    int lr;
    __device__ __forceinline__ void seed(int first, int lr_, int pc) {
        lr = lr_;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int pce = first + i;
            const int isv = pce >> 3, row = (pce & 7) * 8 + lr;
            const int c = pc ^ (isv ? swz_v(row) : swz_k(row));
            src[i] = isv ? Vb + (size_t)row * ldv + c * 8 : Kb + (size_t)row * ldk + c * 8;
            step[i] = (long)ATT_KV * (isv ? ldv : ldk);
        }
    }
    __device__ __forceinline__ void load_tile(int kt, unsigned slot) {
        const E* zeros = reinterpret_cast<const E*>(g_att_zero16);
        const bool whole = (kt + 1) * ATT_KV <= S;
#pragma unroll
        for (int pce = 0; pce < 16; ++pce) {
            const E* sp = (whole || kt * ATT_KV + (pce & 7) * 8 + lr < S) ? src[pce] : zeros;
            att_dma16(sp, slot + att32_piece_off(pce));
            src[pce] += step[pce];
        }
    }
    __device__ __forceinline__ void load_piece(int kt, int i, int pce, unsigned slot, unsigned dump, bool live) {
        if ((kt + 1) * ATT_KV <= S) {
            att_dma16(src[i], slot + att32_piece_off(pce));
        } else {
            const E* zeros = reinterpret_cast<const E*>(g_att_zero16);
            const E* sp = (live && kt * ATT_KV + (pce & 7) * 8 + lr < S) ? src[i] : zeros;
            att_dma16(sp, live ? slot + att32_piece_off(pce) : dump);
        }
        src[i] += step[i];
    }
};

// The form of a 32-row launch, from (T, H, B) alone: compute waves per block, each form but the last with one extra wave
// that issues every LDS-DMA of every tile (a compute wave that queues in the CU's load path multiplies nothing meanwhile:
// 16 wave-instructions of 1 KiB per tile, 16 cycles each).  (tests/edge_util.py's attention_kernel is the tests' own model of it.)
// Seven compute waves (224 query rows; with the loader two waves per SIMD) share a K/V ring unless that leaves half
// the CUs idle: SDXL's 32x32 level at batch 1 is then 160 blocks of four waves, one per SIMD (15.4 us against 20.2).
// Against eight self-loading waves: 4096 tokens 73 -> 70 us (batch 1), 215 -> 206 us (batch 4); 1024 tokens at
// batch 4 43.8 -> 39.2 us.
// Three compute waves (96 rows) when four would still leave a third of the CUs without a block: the 32x32 level at batch 1
// is 220 blocks instead of 160 (15.3 -> 13.9 us).
// Eight self-loading waves (256 rows per block) where that saves a whole round of blocks over seven + loader (224 rows): a round
// of the eight-wave blocks takes 1.2x as long (tools/attn_nw_sweep.py: the refiner's 12 heads x 4,096 tokens at batch 4 are 878
// blocks = 4 rounds of 65 us against 768 = 3 rounds of 77 us)
struct Att32Form {                                     // (the dynamic LDS of every form is the constant ATT32_RING)
    int nw;                                            // compute waves: 3, 4, 7 (+ a loader wave) or 8 (self-loading); 5, 6 by the developer knob only
    int threads;                                       // loader wave included
    long grid;                                         // blocks (1-D); the caller checks that it fits a launch
};
static inline Att32Form att32_form(int T, int H, int B) {
    static const int force_nw = att_dev_env_int("ST_ATT_NW", 0);       // dev knob: waves per block of the self-attention kernels
    int nw = (long)cdiv(T, 256) * H * B <= 128 ? 4 : 7;
    if (nw == 4 && (long)cdiv(T, 128) * H * B <= 176 && (long)cdiv(T, 96) * H * B <= 256) nw = 3;
    if (nw == 7) {
        const long r7 = cdiv((long)cdiv(T, 224) * H * B, 256L), r8 = cdiv((long)cdiv(T, 256) * H * B, 256L);
        if (6 * r8 < 5 * r7) nw = 8;
    }
    if (force_nw >= 3 && force_nw <= 8) nw = force_nw;
    return {nw, (nw + (nw != 8 ? 1 : 0)) * 64, (long)cdiv(T, 32 * nw) * H * B};
}
