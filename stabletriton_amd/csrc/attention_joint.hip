// Two-source self-attention for gfx950 (include/stabletriton_amd.h, st_attention_joint): every query row of batch entry b
// attends to its own S1 keys AND to the S2 keys of entry b % B2 of a second K / V, under ONE softmax - reference-only control,
// where a generated row also reads the reference row's tokens.  Entries >= lead, and every entry while the device gate is off,
// see the first source alone.
//
// attnj32i_kernel runs attn32i_core (attention_core.h), the body of attn32i_kernel (attention.hip), with one thing of its own: where
// a key row comes from.  Tile partition, six-slot ring, counted waits, lazy maximum, mask_tail (on the total S1 + S2_eff), MFMA order,
// the 1-D XCD-aware grid and the launch form are shared code, so the LDS images are those of st_attention on the contiguous
// concatenation of the two sources, and so are the bits.  This file is the address rule (AttKeys2), the gate, the launcher and the
// entry point.  Per lane and 16-byte piece, key s = kt*64 + row reads
//     k  + b*S1*ldk + s*ldk                     if s < S1
//     k2 + (b % B2)*bsk2 + (s - S1)*ldk2        if s < S1 + S2_eff
//     the zero line                             otherwise
// at the swizzled chunk of the core.  Tiles that lie whole in one source keep running pointers (re-seeded once, at the first whole
// tile of the second source); only a tile that holds the boundary or the tail evaluates the rule per lane.
// S2_eff is 0 unless b < lead and the gate is on; the gate is one scalar load of a value no launch writes, uniform over the grid,
// and with S2_eff = 0 no address of k2 / v2 is ever formed into a load.
//
// st_attention_shared (StyleAligned, style_aligned.py) is the same kernel under another prologue, the block rule: k2 / v2 are k / v,
// S2 = S1, entry b reads entry b - b % per, and S2_eff is 0 for the first entry of every block of `per` (the style row).
#include "attention_core.h"

template <typename E>
struct JointArgs {
    const E *Q, *K, *V, *K2, *V2;
    E* O;
    int T, S1, S2, B2, lead, H;
    int per;                                           // 0: the rule above; > 0: the block rule of st_attention_shared
    int ldq, ldk, ldv, ldk2, ldv2, ldo;                // token strides (the host checks that they fit: fewer scalar registers than long)
    long bsk2, bsv2;
    float scale_log2e;
    const float* table;
    const int* step;
    int n;
};

// The two-source key rule of attn32i_core (attention_core.h: the KEYS contract).  Every path of load_tile issues sixteen DMAs
// and load_piece one, whichever source a tile lies in.
template <typename E, int NW, bool LD>
struct AttKeys2 {
    static constexpr int N = LD ? 16 : 16 / NW;
    const E *Kb, *Vb, *K2b, *V2b;                      // key 0 of this (batch entry, head) in the first / the second source
    long ldk, ldv, ldk2, ldv2;
    int S1, S;                                         // S = S1 + S2_eff
    const E* src[N];
    const E* src2[N];                                  // (self-loading waves only)
    long step[N], step2[N];
    int lr, pc;
    // the address rule: where this lane's 16 bytes of piece pce of the tile that starts at key s0 come from
    __device__ __forceinline__ const E* piece_src(int pce, int s0) const {
        const int isv = pce >> 3, row = (pce & 7) * 8 + lr;
        const int c = pc ^ (isv ? swz_v(row) : swz_k(row));
        const int s = s0 + row;
        if (s < S1) return (isv ? Vb + (size_t)s * ldv : Kb + (size_t)s * ldk) + c * 8;
        if (s < S) return (isv ? V2b + (size_t)(s - S1) * ldv2 : K2b + (size_t)(s - S1) * ldk2) + c * 8;
        return reinterpret_cast<const E*>(g_att_zero16);
    }
    // The loader wave keeps one running pointer per piece (S1 >= 256: tile 0 lies in the first source).  Self-loading waves keep
    // TWO, both advanced by 64 keys per tile: key (tile start + row) of the first source, and of the second source's line continued
    // backwards to key 0 (an address only until the tile reaches S1); the rule per lane is then a select between them and the zero line.
    __device__ __forceinline__ void seed(int first, int lr_, int pc_) {
        lr = lr_; pc = pc_;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int pce = first + i;
            const int isv = pce >> 3, row = (pce & 7) * 8 + lr;
            const int c = pc ^ (isv ? swz_v(row) : swz_k(row));
            step[i] = (long)ATT_KV * (isv ? ldv : ldk);
            step2[i] = (long)ATT_KV * (isv ? ldv2 : ldk2);
            if constexpr (LD) {
                src[i] = piece_src(pce, 0);
            } else {
                src[i] = (isv ? Vb + (size_t)row * ldv : Kb + (size_t)row * ldk) + c * 8;
                src2[i] = (isv ? V2b : K2b) + (long)(row - S1) * (isv ? ldv2 : ldk2) + c * 8;
            }
        }
    }
    __device__ __forceinline__ void load_tile(int kt, unsigned slot) {
        const int s0 = kt * ATT_KV;
        if (s0 + ATT_KV <= S1) {                  // whole tile in the first source
#pragma unroll
            for (int pce = 0; pce < 16; ++pce) {
                att_dma16(src[pce], slot + att32_piece_off(pce));
                src[pce] += step[pce];
            }
        } else if (s0 >= S1 && s0 + ATT_KV <= S) {      // whole tile in the second source
            if (s0 - S1 < ATT_KV) {               // the first of them: the running pointers move over
#pragma unroll
                for (int pce = 0; pce < 16; ++pce) src[pce] = piece_src(pce, s0);
            }
#pragma unroll
            for (int pce = 0; pce < 16; ++pce) {
                att_dma16(src[pce], slot + att32_piece_off(pce));
                src[pce] += step2[pce];
            }
        } else {                                  // the tile holds the boundary, the tail or both: the rule per lane
#pragma unroll
            for (int pce = 0; pce < 16; ++pce) att_dma16(piece_src(pce, s0), slot + att32_piece_off(pce));
        }
    }
    __device__ __forceinline__ void load_piece(int kt, int i, int pce, unsigned slot, unsigned dump, bool live) {
        const int s0 = kt * ATT_KV;
        const int s = s0 + (pce & 7) * 8 + lr;
        // whole tile in the first source / in the second / the boundary, the tail, or a dummy past the last tile (every key >= S)
        // (two issue sites behind ONE wave-uniform branch, the code the rule compiled to as a lambda of the kernel: written as one
        //  select chain in this method it is if-converted before inlining, every tile then pays the rule's per-lane arithmetic,
        //  and the pointers that keeps live cost three VGPRs)
        const bool all1 = s0 + ATT_KV <= S1, all2 = s0 >= S1 && s0 + ATT_KV <= S;
        const unsigned dst = __builtin_amdgcn_readfirstlane(live ? slot + att32_piece_off(pce) : dump);
        if (all1 || all2) att_dma16(all1 ? src[i] : src2[i], dst);
        else att_dma16(s < S1 ? src[i] : s < S ? src2[i] : reinterpret_cast<const E*>(g_att_zero16), dst);
        src[i] += step[i];
        src2[i] += step2[i];
    }
};

template <typename E, int NW, bool LD>
__global__ __launch_bounds__((NW + (LD ? 1 : 0)) * 64) void attnj32i_kernel(const JointArgs<E> a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];      // the ring, then a 1-KiB dump for the dummy DMAs
    const int T = a.T, S1 = a.S1;
    int head, b, xblk;
    att_xcd_decode<true>(T, 32 * NW, a.H, b, head, xblk);

    // the gate: scalar loads of values no launch writes; S = keys this entry attends to
    // which entry reads a second source, and whose: b < lead reads entry b % B2 of k2 / v2; under the block rule (per > 0) entry b
    // reads the first entry of its own block of `per`, b - b % per, of k2 / v2 (the host passes k / v), and that first entry nothing
    const int rem = a.per ? b % a.per : 0;
    int s2 = 0;
    if (a.per ? rem != 0 : b < a.lead) {
        bool on = true;
        if (a.table) {
            const int i = *a.step;
            on = a.table[i < 0 ? 0 : (i >= a.n ? a.n - 1 : i)] != 0.f;
        }
        s2 = on ? a.S2 : 0;
    }
    AttKeys2<E, NW, LD> keys;
    keys.ldk = a.ldk; keys.ldv = a.ldv; keys.ldk2 = a.ldk2; keys.ldv2 = a.ldv2;
    keys.S1 = S1;
    keys.S = __builtin_amdgcn_readfirstlane(S1 + s2);
    keys.Kb = a.K + (size_t)b * S1 * keys.ldk + (size_t)head * ATT_D;
    keys.Vb = a.V + (size_t)b * S1 * keys.ldv + (size_t)head * ATT_D;
    if (a.per) {                                       // the block rule forms no address of the second source unless it is read
        keys.K2b = s2 ? a.K2 + (size_t)(b - rem) * a.bsk2 + (size_t)head * ATT_D : keys.Kb;
        keys.V2b = s2 ? a.V2 + (size_t)(b - rem) * a.bsv2 + (size_t)head * ATT_D : keys.Vb;
    } else {
        const int b2 = b % a.B2;
        keys.K2b = a.K2 + (size_t)b2 * a.bsk2 + (size_t)head * ATT_D;
        keys.V2b = a.V2 + (size_t)b2 * a.bsv2 + (size_t)head * ATT_D;
    }
    const long ldq = a.ldq, ldo = a.ldo;
    attn32i_core<E, NW, LD>(a.Q + (size_t)b * T * ldq + (size_t)head * ATT_D, ldq, T, xblk,
                            a.O + (size_t)b * T * ldo + (size_t)head * ATT_D, ldo, a.scale_log2e, lds, keys);
}

template <typename E>
static int attention_joint_launch(const JointArgs<E>& a, int B, hipStream_t st) {
    // att32_form reads T, H and B only: the gated-off launch and st_attention at S = S1 run the same form and the same tile partition
    const Att32Form f = att32_form(a.T, a.H, B);
    auto kfn = f.nw == 8 ? attnj32i_kernel<E, 8, false> : f.nw == 7 ? attnj32i_kernel<E, 7, true> : f.nw == 3 ? attnj32i_kernel<E, 3, true> : attnj32i_kernel<E, 4, true>;
#ifdef ST_DEV_CONFIGS
    if (f.nw == 5) kfn = attnj32i_kernel<E, 5, true>;
    if (f.nw == 6) kfn = attnj32i_kernel<E, 6, true>;
#endif
    static unsigned long long lds_ok[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // per kernel: bit mask over device ordinals
    ensure_dynamic_lds(kfn, ATT32_RING, &lds_ok[f.nw - 1]);
    ST_REQUIRE(f.grid < (1L << 31), "attention_joint: too many blocks");
    hipLaunchKernelGGL(kfn, dim3((unsigned)f.grid), dim3(f.threads), ATT32_RING, st, a);
    return st_check_launch("attention_joint");
}

extern "C" int st_attention_joint(const void* q, const void* k, const void* v, const void* k2, const void* v2, void* out,
                                  int B, int T, int S1, int S2, int B2, int lead, int H, int D,
                                  long ldq, long ldk, long ldv, long ldk2, long ldv2, long bsk2, long bsv2, long ldo, float scale,
                                  const float* gate_table, const int* gate_step, int gate_n, int dtype, void* stream) {
    ST_REQUIRE(q && k && v && k2 && v2 && out, "attention_joint: null pointer");
    ST_REQUIRE(B > 0 && T > 0 && S2 >= 1 && H > 0 && B2 >= 1, "attention_joint: bad shape B=%d T=%d S2=%d H=%d B2=%d", B, T, S2, H, B2);
    ST_REQUIRE(dtype == ST_BF16 || dtype == ST_F16, "attention_joint: 16-bit types only (dtype %d); other types take the host's slow path", dtype);
    ST_REQUIRE(D == ATT_D, "attention_joint: head_dim %d not supported (only %d)", D, ATT_D);
    ST_REQUIRE(S1 >= 256, "attention_joint: S1 = %d, the kernel starts at 256 keys in the first source", S1);
    ST_REQUIRE((long)S1 + S2 <= (1L << 30), "attention_joint: S1 + S2 too large");
    ST_REQUIRE(lead >= 0 && lead <= B, "attention_joint: lead %d outside [0, B = %d]", lead, B);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_joint: too many heads/batches for one launch");
    ST_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldk2 % 8 == 0 && ldv2 % 8 == 0 && bsk2 % 8 == 0 && bsv2 % 8 == 0 && ldo % 4 == 0,
               "attention_joint: strides must keep 16-byte alignment");
    ST_REQUIRE((ldq | ldk | ldv | ldk2 | ldv2 | ldo) >= 0 && (ldq | ldk | ldv | ldk2 | ldv2 | ldo) < (1L << 31), "attention_joint: token strides must fit 31 bits");
    ST_REQUIRE(ldk2 >= (long)H * D && ldv2 >= (long)H * D && bsk2 >= 0 && bsv2 >= 0, "attention_joint: second-source strides must hold a row of H*D values and not be negative");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)k2 | (uintptr_t)v2 | (uintptr_t)out) % 16 == 0,
               "attention_joint: pointers must be 16-byte aligned");
    ST_REQUIRE((gate_table == nullptr) == (gate_step == nullptr), "attention_joint: the gate is a table AND a step, or neither");
    ST_REQUIRE(!gate_table || gate_n > 0, "attention_joint: gate table of %d entries", gate_n);
    ST_REQUIRE((((uintptr_t)gate_table | (uintptr_t)gate_step) & 3) == 0, "attention_joint: misaligned gate pointer");
    void* out_split = nullptr;
    if (int e = st_take_split_arm("attention_joint", (long)B * T, H * D, false, &out_split)) return e;
    hipStream_t st = (hipStream_t)stream;
    const float c = scale * 1.4426950408889634f;
    if (dtype == ST_BF16) {
        const JointArgs<bf16> a{(const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)k2, (const bf16*)v2, (bf16*)out, T, S1, S2, B2, lead, H, 0,
                                (int)ldq, (int)ldk, (int)ldv, (int)ldk2, (int)ldv2, (int)ldo, bsk2, bsv2, c, gate_table, gate_step, gate_n};
        return attention_joint_launch<bf16>(a, B, st);
    }
    const JointArgs<f16> a{(const f16*)q, (const f16*)k, (const f16*)v, (const f16*)k2, (const f16*)v2, (f16*)out, T, S1, S2, B2, lead, H, 0,
                           (int)ldq, (int)ldk, (int)ldv, (int)ldk2, (int)ldv2, (int)ldo, bsk2, bsv2, c, gate_table, gate_step, gate_n};
    return attention_joint_launch<f16>(a, B, st);
}

// StyleAligned's shared attention: the same kernel under the block rule.  The second source is k / v themselves (entry b - b % per,
// S1 keys), so the launch needs no second pair of pointers and a style row (b % per == 0) is st_attention on that row.
extern "C" int st_attention_shared(const void* q, const void* k, const void* v, void* out, int B, int T, int S1, int H, int D, int per,
                                   long ldq, long ldk, long ldv, long ldo, float scale,
                                   const float* gate_table, const int* gate_step, int gate_n, int dtype, void* stream) {
    ST_REQUIRE(q && k && v && out, "attention_shared: null pointer");
    ST_REQUIRE(B > 0 && T > 0 && H > 0 && per >= 1, "attention_shared: bad shape B=%d T=%d H=%d per=%d", B, T, H, per);
    ST_REQUIRE(dtype == ST_BF16 || dtype == ST_F16, "attention_shared: 16-bit types only (dtype %d); other types take the host's slow path", dtype);
    ST_REQUIRE(D == ATT_D, "attention_shared: head_dim %d not supported (only %d)", D, ATT_D);
    ST_REQUIRE(S1 >= 256, "attention_shared: S1 = %d, the kernel starts at 256 keys per entry", S1);
    ST_REQUIRE(2L * S1 <= (1L << 30), "attention_shared: S1 too large");
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_shared: too many heads/batches for one launch");
    ST_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "attention_shared: strides must keep 16-byte alignment");
    ST_REQUIRE((ldq | ldk | ldv | ldo) >= 0 && (ldq | ldk | ldv | ldo) < (1L << 31), "attention_shared: token strides must fit 31 bits");
    ST_REQUIRE(ldk >= (long)H * D && ldv >= (long)H * D, "attention_shared: key / value strides must hold a row of H*D values");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16 == 0, "attention_shared: pointers must be 16-byte aligned");
    ST_REQUIRE((gate_table == nullptr) == (gate_step == nullptr), "attention_shared: the gate is a table AND a step, or neither");
    ST_REQUIRE(!gate_table || gate_n > 0, "attention_shared: gate table of %d entries", gate_n);
    ST_REQUIRE((((uintptr_t)gate_table | (uintptr_t)gate_step) & 3) == 0, "attention_shared: misaligned gate pointer");
    void* out_split = nullptr;
    if (int e = st_take_split_arm("attention_shared", (long)B * T, H * D, false, &out_split)) return e;
    hipStream_t st = (hipStream_t)stream;
    const float c = scale * 1.4426950408889634f;
    const long bsk = (long)S1 * ldk, bsv = (long)S1 * ldv;
    if (dtype == ST_BF16) {
        const JointArgs<bf16> a{(const bf16*)q, (const bf16*)k, (const bf16*)v, (const bf16*)k, (const bf16*)v, (bf16*)out, T, S1, S1, B, 0, H, per,
                                (int)ldq, (int)ldk, (int)ldv, (int)ldk, (int)ldv, (int)ldo, bsk, bsv, c, gate_table, gate_step, gate_n};
        return attention_joint_launch<bf16>(a, B, st);
    }
    const JointArgs<f16> a{(const f16*)q, (const f16*)k, (const f16*)v, (const f16*)k, (const f16*)v, (f16*)out, T, S1, S1, B, 0, H, per,
                           (int)ldq, (int)ldk, (int)ldv, (int)ldk, (int)ldv, (int)ldo, bsk, bsv, c, gate_table, gate_step, gate_n};
    return attention_joint_launch<f16>(a, B, st);
}
