// Fused attention core for gfx950: out = softmax(q k^T * scale) v, per head, no
// mask, head_dim 64 (every SDXL-base/refiner head).  Row A of SURVEY.md 8a:
// replaces the eager matmul/softmax/matmul of unet_pt.py:133-142 without ever
// materialising the (B,H,T,S) score tensor.
//
// bf16 kernels (flash style):
//   * attn32i_kernel - self-attention (S >= 256): a wave owns 32 query rows (v_mfma_f32_32x32x16_bf16), a block of
//     seven (or four) such waves plus a loader wave walks the keys in tiles of 64 that arrive by LDS-DMA in a six-slot ring;
//     the softmax instructions are placed in the gaps between the MFMAs of the same wave.  Its body is attn32i_core
//     (attention_core.h), which the two-source kernel of attention_joint.hip runs too: the kernel here is the grid decode
//     and the one-source key rule (AttKeys1);
//   * attn16v2_kernel - the 77-token text context (S < 256): a wave owns 16 query rows (v_mfma_f32_16x16x32_bf16),
//     so that the two-tile loop still has enough waves to fill the chip;
//   * both compute the scores transposed, S^T = K Q^T, so a lane holds the scores of ONE query row; the S^T accumulator
//     is reused directly as the B operand of O^T = V^T P^T (no LDS round trip for P); V^T fragments come from
//     ds_read_b64_tr_b16 on the row-major V image; K and V images are XOR-swizzled per 16-byte chunk on the DMA source
//     side so the fragment reads are conflict-free; keys beyond S are zero-filled and masked.
// fp32 ("strict" parity mode): attention_f32.hip.
#include "attention_core.h"

template <typename E, int NW, int TAG>
__global__ __launch_bounds__(NW * 64) void attn16v2_kernel(const E* __restrict__ Q, const E* __restrict__ K,
                                                           const E* __restrict__ V, E* __restrict__ O,
                                                           int T, int S, long ldq, long ldk, long ldv, long ldo, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) char lds[3 * 2 * ATT_KV * 128];
    const int t_ = threadIdx.x, lane = t_ & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t_ >> 6);
    const int head = blockIdx.y, b = blockIdx.z;
    const int row0 = blockIdx.x * NW * 16;
    attn16_core<E, NW>(Q + (size_t)b * T * ldq + (size_t)row0 * ldq + (size_t)head * ATT_D, ldq, T - row0,
                    K + (size_t)b * S * ldk + (size_t)head * ATT_D, V + (size_t)b * S * ldv + (size_t)head * ATT_D, ldk, ldv, S,
                    O + (size_t)b * T * ldo + (size_t)row0 * ldo + (size_t)head * ATT_D, ldo, T - row0, scale_log2e, lds, wave, lane);
}

// ---- 32-row kernel: attn32i_core (attention_core.h) on one key source ------------------------------------------------
template <typename E, int NW, bool LD>
__global__ __launch_bounds__((NW + (LD ? 1 : 0)) * 64) void attn32i_kernel(const E* __restrict__ Q, const E* __restrict__ K,
                                                      const E* __restrict__ V, E* __restrict__ O,
                                                      int T, int S, long ldq, long ldk, long ldv, long ldo, float scale_log2e,
                                                      int H) {
    extern __shared__ __attribute__((aligned(16))) char lds[];      // the ring, then a 1-KiB dump for the dummy DMAs
    int head, b, xblk;
    att_xcd_decode<false>(T, 32 * NW, H, b, head, xblk);
    AttKeys1<E, NW, LD> keys;
    keys.Kb = K + (size_t)b * S * ldk + (size_t)head * ATT_D;
    keys.Vb = V + (size_t)b * S * ldv + (size_t)head * ATT_D;
    keys.ldk = ldk; keys.ldv = ldv; keys.S = S;
    attn32i_core<E, NW, LD>(Q + (size_t)b * T * ldq + (size_t)head * ATT_D, ldq, T, xblk,
                            O + (size_t)b * T * ldo + (size_t)head * ATT_D, ldo, scale_log2e, lds, keys);
}


// fp32 ("strict" parity mode): attention_f32.hip - split operands on the 16-bit matrix pipe, fp32 softmax
int attention_f32_launch(const float* q, const float* k, const float* v, float* out, int B, int T, int S, int H,
                         long ldq, long ldk, long ldv, long ldo, float scale, void* out_split, bool presplit, hipStream_t st);

// head_dim 16, 32, 128 (attention_anyd.hip)
int attention_anyd_launch(int dtype, const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H, int D,
                          long ldq, long ldk, long ldv, long ldo, float scale, void* out_split, hipStream_t st);

// head_dim 512, bf16 / fp16 (attention_d512.hip)
int attention_d512_launch(int dtype, const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H,
                          long ldq, long ldk, long ldv, long ldo, float scale, hipStream_t st);

template <typename E>
static int attention16_launch(const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H,
                              long ldq, long ldk, long ldv, long ldo, float scale, hipStream_t st) {
    const float c = scale * 1.4426950408889634f;
    static const int force_16 = att_dev_env_int("ST_ATT_R16", -1);     // dev knob: 1 = 16-row kernel for every S, 0 = never
    const bool rows16 = force_16 >= 0 ? force_16 != 0 : S < 256;
    if (rows16) {
        // measured (tools/op_bench.py): 16-row waves win for the 77-key text context (more waves for a two-tile loop);
        // TAG 1 only gives these launches their own kernel name in the profiles
        hipLaunchKernelGGL((attn16v2_kernel<E, 4, 1>), dim3(cdiv(T, 64), H, B), dim3(256), 0, st, (const E*)q, (const E*)k,
                           (const E*)v, (E*)out, T, S, ldq, ldk, ldv, ldo, c);
        return st_check_launch("attention");
    }
    const Att32Form f = att32_form(T, H, B);
    auto kfn = f.nw == 8 ? attn32i_kernel<E, 8, false> : f.nw == 7 ? attn32i_kernel<E, 7, true> : f.nw == 3 ? attn32i_kernel<E, 3, true> : attn32i_kernel<E, 4, true>;
#ifdef ST_DEV_CONFIGS
    if (f.nw == 5) kfn = attn32i_kernel<E, 5, true>;
    if (f.nw == 6) kfn = attn32i_kernel<E, 6, true>;
#endif
    static unsigned long long lds_ok[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // per kernel: bit mask over device ordinals
    ensure_dynamic_lds(kfn, ATT32_RING, &lds_ok[f.nw - 1]);
    ST_REQUIRE(f.grid < (1L << 31), "attention: too many blocks");
    hipLaunchKernelGGL(kfn, dim3((unsigned)f.grid), dim3(f.threads), ATT32_RING, st, (const E*)q, (const E*)k, (const E*)v,
                       (E*)out, T, S, ldq, ldk, ldv, ldo, c, H);
    return st_check_launch("attention");
}

extern "C" int st_attention(const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H, int D,
                            long ldq, long ldk, long ldv, long ldo, float scale, int dtype, void* stream) {
    ST_REQUIRE(q && k && v && out, "attention: null pointer");
    ST_REQUIRE(B > 0 && T > 0 && S > 0 && H > 0, "attention: bad shape B=%d T=%d S=%d H=%d", B, T, S, H);
    ST_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128 || D == 512, "attention: head_dim %d not supported (16, 32, 64, 128, 512)", D);
    ST_REQUIRE(D != 512 || st_dtype_is16(dtype), "attention: head_dim 512 takes bf16 or fp16 tensors, not dtype %d", dtype);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention: too many heads/batches for one launch");
    const int vec = st_dtype_is16(dtype) ? 8 : 4;
    ST_REQUIRE(ldq % vec == 0 && ldk % vec == 0 && ldv % vec == 0 && ldo % 4 == 0, "attention: strides must keep 16-byte alignment");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16 == 0, "attention: pointers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    void* out_split = nullptr;
    if (int e = st_take_split_arm("attention", (long)B * T, H * D, dtype == ST_F32, &out_split)) return e;
    if (D == 512) return attention_d512_launch(dtype, q, k, v, out, B, T, S, H, ldq, ldk, ldv, ldo, scale, st);
#ifdef ST_DEV_CONFIGS
    static const int force_anyd = att_dev_env_int("ST_ATT_ANYD", 0);       // dev knob: head_dim 64 on the generic kernel too
    if (force_anyd) return attention_anyd_launch(dtype, q, k, v, out, B, T, S, H, D, ldq, ldk, ldv, ldo, scale, out_split, st);
#endif
    if (D != ATT_D) return attention_anyd_launch(dtype, q, k, v, out, B, T, S, H, D, ldq, ldk, ldv, ldo, scale, out_split, st);
    if (dtype == ST_BF16) return attention16_launch<bf16>(q, k, v, out, B, T, S, H, ldq, ldk, ldv, ldo, scale, st);
    if (dtype == ST_F16) return attention16_launch<f16>(q, k, v, out, B, T, S, H, ldq, ldk, ldv, ldo, scale, st);
    if (dtype == ST_F32) return attention_f32_launch((const float*)q, (const float*)k, (const float*)v, (float*)out, B, T, S, H, ldq, ldk, ldv, ldo, scale, out_split, false, st);
    return st_fail("attention: unsupported dtype %d", dtype);
}

// st_attention for fp32 tensors whose K and V a producer left as split images (the q|k|v projection of self-attention:
// st_arm_split_output): ks / vs = first byte of head 0's columns in row 0 of the image(s), k_cols / v_cols = values per image
// row; q, out and everything else as st_attention with ST_F32.  Same arithmetic as st_attention (which splits K / V itself,
// tile by tile): the same bits.
extern "C" int st_attention_split(const void* q, const void* ks, const void* vs, void* out, int B, int T, int S, int H, int D,
                                  long ldq, long k_cols, long v_cols, long ldo, float scale, void* stream) {
    ST_REQUIRE(q && ks && vs && out, "attention_split: null pointer");
    ST_REQUIRE(B > 0 && T > 0 && S > 0 && H > 0, "attention_split: bad shape B=%d T=%d S=%d H=%d", B, T, S, H);
    ST_REQUIRE(D == ATT_D, "attention_split: head_dim %d not supported (only %d)", D, ATT_D);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_split: too many heads/batches for one launch");
    ST_REQUIRE(ldq % 4 == 0 && ldo % 4 == 0 && k_cols % 32 == 0 && v_cols % 32 == 0, "attention_split: strides must keep 16-byte alignment, image rows whole segments");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)out) % 16 == 0 && ((uintptr_t)ks | (uintptr_t)vs) % 128 == 0, "attention_split: q / out 16-byte, image columns segment (128-byte) aligned");
    void* out_split = nullptr;
    if (int e = st_take_split_arm("attention_split", (long)B * T, H * D, true, &out_split)) return e;
    return attention_f32_launch((const float*)q, (const float*)ks, (const float*)vs, (float*)out, B, T, S, H, ldq, k_cols, v_cols, ldo, scale, out_split, true,
                                (hipStream_t)stream);
}
