// Stem convolution of a UNet whose input has 5..16 channels that come from one or two places (include/stabletriton_amd.h,
// st_conv_stem): 3x3, stride 1, zero padding 1, bias epilogue, NHWC output.  The nine-channel conv_in of the SDXL inpainting
// checkpoints is the shape it is built for: channels [0, C0) are source a (the loop's 4-channel x_in, rewritten every step), channels
// [C0, C0 + C1) source b (mask | masked-image latent, constant over the trajectory); image n reads a[n % Na] and b[n % Nb].
//
// Work split.  A block of four waves owns an 8 x 16 tile of output pixels of one image (blockIdx.x: image, tile row, tile column) and
// a range of output channels (blockIdx.y: `chunk` channels, a multiple of 32, chosen by the launch so the grid has two to four blocks
// per CU - at 128 x 128 one image is only 128 pixel tiles).  Wave w owns tile rows 2w and 2w + 1: two 16-pixel MFMA columns.
//
// LDS.  (1) The tile's halo, 10 x 18 pixels, one padded channel vector of 16 elements per pixel (32 bytes in the 16-bit types, 64 in
// fp32), zero beyond C0 + C1 and outside the image.  It is read from global memory once: a source whose pixel is 8 or 16 bytes and
// aligned so (the loop's x_in: 4 x 16 bit) goes in with one vector load per pixel, every other channel by element loads (one
// 18-byte pixel of a single nine-channel tensor, the five condition channels).  (2) The weights of up to 64 output channels at a time,
// read LIVE from conv.weight in torch's channels-last order (Cout, 3, 3, C) and reordered while they are staged: k = tap * 16 + c
// ("tap-major at 16"), zero for c >= C and for the padding k, rows padded to 168 (fp32: 148) elements so that the 16 rows of a
// fragment read fall on different banks, and rows permuted inside each group of 32 channels (below).  No host-side repack exists, so
// an in-place weight update (LoRA merge) is seen by the next launch.
//
// Registers.  The product is computed transposed, D[channel][pixel] = W[channel][k] * X[k][pixel], so a lane ends up with consecutive
// channels of ONE pixel.  The pixel operand of a wave is built once from the halo and stays in registers over the whole channel loop:
//   16-bit types  v_mfma_f32_16x16x32: K = 160 = 5 steps; step s, lane group g = lane / 16 covers tap 2s + g / 2, channels
//                 8 (g % 2) .. + 7: one 16-byte LDS read at a fixed offset from the lane's pixel.  Tap 9 (second half of step 4) is zero.
//                 2 pixel columns x 5 steps x 4 VGPRs = 40 VGPRs.
//   fp32          v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation: the arithmetic class of the thin kernel): step
//                 (tap, q) has lane group g hold channel 4q + g; the steps with 4q >= C are skipped (uniformly), 27 steps at C = 9.
//                 2 x 36 VGPRs.
// The K order was chosen for the addressing, not for density: K is 160 for 81 real terms, and the launch is bound by its output write
// and its boundary, not by the matrix pipe.
//
// Output.  Channels are processed 32 at a time with two MFMAs per pixel column; MFMA q's row m is channel 8 (m / 4) + 4q + m % 4 of
// the group (the weight rows are stored in LDS in that order), so lane (g, pixel) holds channels 8g .. 8g + 7: one 16-byte store in
// the 16-bit types (two in fp32), and the four lane groups of a pixel write 64 (128) contiguous bytes.  Every output element is written
// by exactly one lane from a sum of fixed order: two launches give the same bits, and the two-source and the one-tensor form of the
// same values share one K order and give the same bits too.  All global index arithmetic is 64-bit.
//
// Resources (hipcc -O3, gfx950; -Rpass-analysis=kernel-resource-usage):
//   bf16   VGPRs  94  SGPRs 62  LDS 27264 bytes  scratch 0   (5 waves per SIMD)
//   fp16   VGPRs  94  SGPRs 62  LDS 27264 bytes  scratch 0   (5 waves per SIMD)
//   fp32   VGPRs 120  SGPRs 62  LDS 49408 bytes  scratch 0   (3 waves per SIMD)
#include "common.h"

namespace {

constexpr int CS_TH = 8, CS_TW = 16;                        // output pixels of a block
constexpr int CS_HW = CS_TW + 2, CS_HALO = (CS_TH + 2) * CS_HW;      // halo row length and pixel count (180)
constexpr int CS_CP = 16;                                   // padded channels per pixel and per tap
constexpr int CS_WC = 64;                                   // output channels staged in LDS at a time
constexpr int CS_THREADS = 256;

struct StemArgs {
    const void *a, *b, *w, *bias;
    void* out;
    long a_px, a_img, b_px, b_img;
    int Na, Nb, C0, C1, H, W, Cout, tiles_x, tiles_y, chunk, veca, vecb;
};

template <typename T> struct StemK {                        // K of the staged weights, their padded row length, elements per 16 bytes
    static constexpr int KTOT = 160, KLD = 168, VEC = 8;
    typedef typename V16<T>::x8 X8;                          // one MFMA operand of a lane
};
template <> struct StemK<float> {
    static constexpr int KTOT = 144, KLD = 148, VEC = 4;
    typedef f32x4 X8;                                        // (unused: the fp32 MFMA takes one float per lane)
};

__device__ __forceinline__ void copy_vec(void* dst, const void* src, int bytes) {
    if (bytes == 8) *reinterpret_cast<u32x2*>(dst) = *reinterpret_cast<const u32x2*>(src);
    else *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
}

// weight row of group-local channel c (0..31) -> LDS row: MFMA q = (c / 4) % 2 reads rows 16q .. 16q + 15, row m = 4 (c / 8) + c % 4
__device__ __forceinline__ int stem_row(int c) { return (c & ~31) + ((c >> 2) & 1) * 16 + ((c & 31) >> 3) * 4 + (c & 3); }

template <typename T>
__device__ __forceinline__ void stage_weights(T* wsm, const T* __restrict__ w, int n0, int valid, int C) {
    typedef StemK<T> K;
    constexpr int ITEMS = K::KTOT / K::VEC;                  // 16-byte items per row
    const int rows = (valid + 31) & ~31;                     // whole groups: the rows past `valid` are zero
    for (int i = threadIdx.x; i < rows * ITEMS; i += CS_THREADS) {
        const int row = i / ITEMS, k0 = (i - row * ITEMS) * K::VEC;
        const int tap = k0 >> 4, c0 = k0 & 15;
        alignas(16) T v[K::VEC];
        const T* src = w + ((long)(n0 + row) * 9 + tap) * C + c0;
#pragma unroll
        for (int e = 0; e < K::VEC; ++e) v[e] = (row < valid && tap < 9 && c0 + e < C) ? src[e] : (T)0.f;
        *reinterpret_cast<u32x4*>(wsm + stem_row(row) * K::KLD + k0) = *reinterpret_cast<const u32x4*>(v);
    }
}

template <typename T>
__global__ __launch_bounds__(CS_THREADS) void conv_stem_kernel(const StemArgs p) {
    typedef StemK<T> K;
    __shared__ __attribute__((aligned(16))) T halo[CS_HALO * CS_CP];
    __shared__ __attribute__((aligned(16))) T wsm[CS_WC * K::KLD];
    const int C = p.C0 + p.C1;
    long t = blockIdx.x;
    const int tx = (int)(t % p.tiles_x); t /= p.tiles_x;
    const int ty = (int)(t % p.tiles_y);
    const long img = t / p.tiles_y;
    const int oy0 = ty * CS_TH, ox0 = tx * CS_TW;
    const T* ai = (const T*)p.a + (img % p.Na) * p.a_img;
    const T* bi = p.C1 > 0 ? (const T*)p.b + (img % p.Nb) * p.b_img : nullptr;

    // ---- halo: every element of the padded vectors by element loads, but the channels a vector load serves
    for (int i = threadIdx.x; i < CS_HALO * CS_CP; i += CS_THREADS) {
        const int hp = i >> 4, c = i & 15;
        const int hy = hp / CS_HW, hx = hp - hy * CS_HW;
        const int iy = oy0 + hy - 1, ix = ox0 + hx - 1;
        const bool inside = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        const long px = (long)iy * p.W + ix;
        T v = (T)0.f;
        if (inside && c < C) {
            if (c < p.C0) {
                if (p.veca) continue;
                v = ai[px * p.a_px + c];
            } else {
                if (p.vecb) continue;
                v = bi[px * p.b_px + (c - p.C0)];
            }
        }
        halo[i] = v;
    }
    if ((p.veca | p.vecb) && threadIdx.x < CS_HALO) {
        const int hp = threadIdx.x;
        const int hy = hp / CS_HW, hx = hp - hy * CS_HW;
        const int iy = oy0 + hy - 1, ix = ox0 + hx - 1;
        if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
            const long px = (long)iy * p.W + ix;
            if (p.veca) copy_vec(halo + hp * CS_CP, ai + px * p.a_px, p.veca);
            if (p.vecb) copy_vec(halo + hp * CS_CP + p.C0, bi + px * p.b_px, p.vecb);
        }
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;                  // pixel column of the MFMA (and weight row), lane group
    const int n_lo = blockIdx.y * p.chunk, n_hi = min(p.Cout, n_lo + p.chunk);

    // the wave's pixel operand: [pixel column j][k step], built behind the first barrier
    typedef typename K::X8 X8;
    X8 xb[2][5];
    float xf[2][9][4];

    for (int s0 = n_lo; s0 < n_hi; s0 += CS_WC) {
        if (s0 != n_lo) __syncthreads();                     // every wave has read the previous weights
        const int valid = min(CS_WC, n_hi - s0);
        stage_weights<T>(wsm, (const T*)p.w, s0, valid, C);
        __syncthreads();
        if (s0 == n_lo) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int row = 2 * wave + j;
                if constexpr (sizeof(T) == 2) {
#pragma unroll
                    for (int s = 0; s < 5; ++s) {
                        const int tap = 2 * s + (g >> 1), tc = min(tap, 8);      // (tap 9 is padding: no halo address is formed for it)
                        const int r = tc / 3, sx = tc - r * 3;
                        const int hp = (row + r) * CS_HW + n + sx;
                        const X8 z = {};
                        xb[j][s] = tap < 9 ? *reinterpret_cast<const X8*>(halo + hp * CS_CP + (g & 1) * 8) : z;
                    }
                } else {
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        const int hp = (row + tap / 3) * CS_HW + n + tap % 3;
#pragma unroll
                        for (int q = 0; q < 4; ++q) xf[j][tap][q] = (float)halo[hp * CS_CP + q * 4 + g];
                    }
                }
            }
        }
        for (int c0 = 0; c0 < valid; c0 += 32) {             // one group of 32 channels: two MFMA row blocks
            f32x4 acc[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 2; ++q) acc[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            const T* wr = wsm + (c0 + n) * K::KLD;
            if constexpr (sizeof(T) == 2) {
#pragma unroll
                for (int s = 0; s < 5; ++s)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const X8 wa = *reinterpret_cast<const X8*>(wr + q * 16 * K::KLD + s * 32 + g * 8);
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if constexpr (std::is_same<T, bf16>::value) acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa, xb[j][s], acc[j][q], 0, 0, 0);
                            else acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, xb[j][s], acc[j][q], 0, 0, 0);
                        }
                    }
            } else {
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        if (qq * 4 >= C) continue;           // (uniform) channels past C are zero on both sides
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const float wa = (float)wr[q * 16 * K::KLD + tap * 16 + qq * 4 + g];
#pragma unroll
                            for (int j = 0; j < 2; ++j) acc[j][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa, xf[j][tap][qq], acc[j][q], 0, 0, 0);
                        }
                    }
            }
            // lane (g, n): channels co .. co + 7 of pixel n in both of the wave's tile rows
            const int co = s0 + c0 + g * 8;
            if (co >= n_hi) continue;
            float bv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) bv[e] = p.bias ? Elem<T>::to_f(((const T*)p.bias)[co + e]) : 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int oy = oy0 + 2 * wave + j, ox = ox0 + n;
                if (oy >= p.H || ox >= p.W) continue;
                alignas(16) T o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = Elem<T>::from_f(acc[j][e >> 2][e & 3] + bv[e]);
                T* dst = (T*)p.out + ((img * p.H + oy) * p.W + ox) * p.Cout + co;
#pragma unroll
                for (int e = 0; e < 8; e += K::VEC) *reinterpret_cast<u32x4*>(dst + e) = *reinterpret_cast<const u32x4*>(o + e);
            }
        }
    }
}

bool ranges_overlap(uintptr_t a0, uintptr_t a_bytes, uintptr_t b0, uintptr_t b_bytes) { return a0 < b0 + b_bytes && b0 < a0 + a_bytes; }

// 8 or 16 when one pixel of the source is that many bytes and every pixel (and its place in the halo vector) is aligned so, else 0
int vector_bytes(const void* ptr, long px, long img, int count, int C, int lds_first, long esz) {
    const long bytes = C * esz;
    if (bytes != 8 && bytes != 16) return 0;
    if ((uintptr_t)ptr % bytes || (px * esz) % bytes || (count > 1 && (img * esz) % bytes) || (lds_first * esz) % bytes) return 0;
    return (int)bytes;
}

template <typename T>
int conv_stem_launch(const StemArgs& a, long tiles, hipStream_t st) {
    // split the output channels over blockIdx.y until the launch has a few blocks per CU
    const int groups = cdiv(a.Cout, 32);
    int ny = cdiv(1024, tiles);
    if (ny > groups) ny = groups;
    StemArgs p = a;
    p.chunk = cdiv(groups, ny) * 32;
    ny = cdiv(a.Cout, p.chunk);
    hipLaunchKernelGGL(conv_stem_kernel<T>, dim3((unsigned)tiles, ny), dim3(CS_THREADS), 0, st, p);
    return st_check_launch("conv_stem");
}

}  // namespace

extern "C" int st_conv_stem(const void* a, long a_px, long a_img, int Na, int C0, const void* b, long b_px, long b_img, int Nb, int C1,
                            const void* w, const void* bias, void* out, int N, int H, int W, int Cout, int epi, int dtype, void* stream) {
    ST_REQUIRE(a && w && out && (C1 <= 0 || b), "conv_stem: null pointer");
    ST_REQUIRE(st_dtype_ok(dtype), "conv_stem: unsupported dtype %d", dtype);
    ST_REQUIRE(N > 0 && H > 0 && W > 0 && Cout > 0 && C0 >= 1 && C1 >= 0 && Na > 0 && (C1 == 0 || Nb > 0),
               "conv_stem: bad shape N=%d H=%d W=%d Cout=%d C0=%d C1=%d Na=%d Nb=%d", N, H, W, Cout, C0, C1, Na, Nb);
    ST_REQUIRE((long)C0 + C1 <= CS_CP, "conv_stem: C0 + C1 = %d channels; at most %d (wider inputs go to conv2d)", C0 + C1, CS_CP);
    ST_REQUIRE(Cout % 16 == 0, "conv_stem: Cout=%d must be a multiple of 16", Cout);
    ST_REQUIRE(N % Na == 0 && (C1 == 0 || N % Nb == 0), "conv_stem: image counts Na=%d, Nb=%d must divide N=%d (image n reads a[n %% Na], b[n %% Nb])",
               Na, Nb, N);
    ST_REQUIRE((epi & ~ST_EPI_BIAS) == 0, "conv_stem: epilogue flags 0x%x; only ST_EPI_BIAS is supported", epi);
    ST_REQUIRE(!(epi & ST_EPI_BIAS) || bias, "conv_stem: ST_EPI_BIAS without a bias pointer");
    ST_REQUIRE(a_px >= C0 && a_img >= 0 && (C1 == 0 || (b_px >= C1 && b_img >= 0)), "conv_stem: bad strides a_px=%ld a_img=%ld b_px=%ld b_img=%ld",
               a_px, a_img, b_px, b_img);
    const long esz = dtype == ST_F32 ? 4 : 2;
    ST_REQUIRE(((uintptr_t)out & 15) == 0, "conv_stem: output not 16-byte aligned");
    ST_REQUIRE(((uintptr_t)a % esz) == 0 && ((uintptr_t)b % esz) == 0 && ((uintptr_t)w % esz) == 0 && ((uintptr_t)bias % esz) == 0,
               "conv_stem: pointer not aligned to its element type");
    const long limit = 0x7fffffffffffL / 4;                      // bytes stay far inside 63 bits
    const long HW = (long)H * W;
    ST_REQUIRE(HW <= limit / Cout / N && a_px <= limit / HW && a_img <= limit / Na && (C1 == 0 || (b_px <= limit / HW && b_img <= limit / Nb)),
               "conv_stem: tensor too large");
    const long tiles_x = cdiv(W, CS_TW), tiles_y = cdiv(H, CS_TH);
    const long tiles = tiles_x * tiles_y * N;
    ST_REQUIRE(tiles <= 0x7fffffffL, "conv_stem: tensor too large (too many workgroups)");
    const uintptr_t o0 = (uintptr_t)out, o_bytes = (uintptr_t)(N * HW * Cout * esz);
    ST_REQUIRE(!ranges_overlap(o0, o_bytes, (uintptr_t)a, (uintptr_t)(((Na - 1) * a_img + (HW - 1) * a_px + C0) * esz)),
               "conv_stem: the output must not overlap source a");
    ST_REQUIRE(C1 == 0 || !ranges_overlap(o0, o_bytes, (uintptr_t)b, (uintptr_t)(((Nb - 1) * b_img + (HW - 1) * b_px + C1) * esz)),
               "conv_stem: the output must not overlap source b");
    StemArgs p;
    p.a = a; p.b = C1 > 0 ? b : nullptr; p.w = w; p.bias = (epi & ST_EPI_BIAS) ? bias : nullptr; p.out = out;
    p.a_px = a_px; p.a_img = a_img; p.b_px = C1 > 0 ? b_px : 0; p.b_img = C1 > 0 ? b_img : 0;
    p.Na = Na; p.Nb = C1 > 0 ? Nb : 1; p.C0 = C0; p.C1 = C1; p.H = H; p.W = W; p.Cout = Cout;
    p.tiles_x = (int)tiles_x; p.tiles_y = (int)tiles_y; p.chunk = 0;
    p.veca = vector_bytes(a, a_px, a_img, Na, C0, 0, esz);
    p.vecb = C1 > 0 ? vector_bytes(b, b_px, b_img, Nb, C1, C0, esz) : 0;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return conv_stem_launch<bf16>(p, tiles, st);
    if (dtype == ST_F16) return conv_stem_launch<f16>(p, tiles, st);
    return conv_stem_launch<float>(p, tiles, st);
}
