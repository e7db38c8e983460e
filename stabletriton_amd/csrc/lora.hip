// LoRA merge: ONE grouped launch rebuilds every adapted weight from its base snapshot (include/stabletriton_amd.h, st_lora_merge).
//
//   W_t[n][k] = round_to_dtype( fp32(Base_t[n][k]) + sum_j scale[slot_j] * sum_r Up_tj[n][r] * DownT_tj[k][r] )
//
// The work list is flat: workgroup b reads tiles[b] = (target, tile index inside the target), the target's row of the
// descriptor table, and owns one 64 (n) x 128 (k) tile of that weight.  Every output element is produced by exactly one lane
// from a fixed sequence of operations (no atomics, no split over the rank), so two launches give the same bits.  A weight
// is rebuilt from its base, never updated: with every scale that touches it zero the base's bits are copied through.
//
// 16-bit models run on the matrix pipe (v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation), as the product D = DownT . Up^T:
// the MFMA's row index is k and its column index is n, so a lane ends up with values that are consecutive in k, the
// contiguous direction of W.  The rows of a PAIR of MFMA tiles are interleaved - row i of tile t is k = 8 (i >> 2) + 4 t +
// (i & 3) of the pair's 32 columns - so that lane group g = lane >> 4 holds k = 8 g .. 8 g + 7 in the two accumulators: one
// 16-byte base read and one 16-byte store per lane and pair.  A workgroup stages the factor rows of its tile in LDS first: they
// are contiguous in memory, so the copy is coalesced, where operand reads straight from memory take one cache line per lane
// (measured on SDXL-base at rank 128: 5.4 ms against this form's figure in DESIGN.md).  The ranks are zero-padded to the
// MFMA's k = 32 by the host, which is exact and leaves no remainder path.  fp32 models use plain fp32 FMAs, ranks padded to 4.
//
// DoRA renormalises a segment's rows: V_j = Base + s_j Up_j Down_j, g_j[n] = m_j[n] / ||V_j[n, :]||,
//
//   W_t[n][k] = round_to_dtype( (1 + sum_j (g_j[n] - 1)) fp32(Base_t[n][k]) + sum_j g_j[n] s_j sum_r Up_tj[n][r] DownT_tj[k][r] )
//
// with g_j = 1 for a segment without a magnitude.  The norm is a reduction over every K-tile of a row, which one tile per
// workgroup cannot hold, so the merge takes two launches of the SAME kernel body (MODE below):
//   norm pass   one workgroup per (row block, K-tile) of every target that has a DoRA segment.  It forms the tile of
//               fp32(Base) + s * acc (acc the unrounded fp32 product) exactly as the merge does, squares it, and writes each
//               row's sum over the tile's <= 128 columns into the workspace: partial[segment][K-tile][n].
//   merge pass  today's tile loop; the lanes that share a row add its partials (four interleaved chains in K-tile order, joined
//               by a fixed xor tree), take g = m / sqrt(sum), and scale.
// Partials in a workspace, not one workgroup walking all K-tiles of its 64 rows: SDXL's largest conv weight is
// (1280, 11520), 20 row blocks against 90 K-tiles, and a walk would leave 236 of 256 CUs idle on the weights that carry most
// of the bytes; with partials the norm pass has the merge's own grid.  The price is 4 N ceil(K / 128) bytes per DoRA segment
// written once and read by the 64-row blocks that need them - 1/64 of the weight's bytes in a 16-bit model.  Every partial is
// one lane's fixed-order sum followed by a fixed xor-shuffle tree, and the partials of a row are added in the same fixed
// order by every workgroup that needs them: no atomics, two merges give the same bits.  A segment at scale 0 is skipped whole in both
// passes, magnitude included, so "all scales zero" still copies the base's bits.
//
// Other factorisations: a segment has a KIND, and the kind only decides how the segment's fp32 tile
// `acc` is formed; the scale-0 skip, the DoRA norm and gain, sum = fma(coef, acc, sum) and the final rounding are shared.
//   PLAIN  acc = Up . Down                                    (the code above)
//   HADA   acc = (Up_1 . Down_1) (.) (Up_2 . Down_2)          LoHa: two products, multiplied elementwise in fp32.  The two
//          factor pairs go through the SAME LDS images one after the other (one more barrier pair) and into two accumulator
//          sets that both stay in registers; both pairs resident at rank 128 would take 102 KiB and one workgroup per CU.
//   KRON   acc[n][k] = W1[n / c][j(k)] * W2[n % c][col(k)]    LoKr: no matrix product, no staging.  W1 (a, b) and W2
//          (c, d taps) are small fp32 tables read through the cache.  k = tap I + j d + q for a channels_last conv weight
//          (layout 1, I = b d), k = (j d + q) taps + tap for a contiguous one (layout 0), a Linear has one tap; col is
//          tap d + q resp. q taps + tap, so in both layouts W2's row is read contiguously where W1's scalar is constant, and
//          with d (layout 1) or d taps (layout 0) a multiple of the 16-byte vector one index computation serves the whole vector.
// HADA and KRON live in their own kernel instantiations (FORMS): they cost registers - an occupancy step - that a table of
// PLAIN segments, the common case, does not pay.  The host states which a table needs; the lean kernels skip what they cannot form.
#include "common.h"

namespace {

constexpr int LORA_THREADS = 256;
constexpr int LORA_TN = ST_LORA_TILE_N;      // 64: four waves of 16 rows
constexpr int LORA_TK = ST_LORA_TILE_K;      // 128: four pairs of MFMA tiles
constexpr int TGT_WORDS = 6;
enum { MODE_PLAIN = 0, MODE_DORA = 1, MODE_NORM = 2 };      // the merge without magnitudes; the DoRA merge pass; the DoRA norm pass
enum { KIND_PLAIN = ST_LORA_KIND_PLAIN, KIND_HADA = ST_LORA_KIND_HADA, KIND_KRON = ST_LORA_KIND_KRON };
constexpr int SEG_WORDS = ST_LORA_FORM_WORDS;      // one row format (the header's) for every kernel

struct Segment {
    int kind, slot;
    long long mag, ws;                    // magnitude (device address of N floats, or 0) and workspace offset in floats
    const void *p0, *p1;                  // Up_1, DownT_1;  KRON: W1, W2
    long long x[6];                       // [rp1, Up_2, DownT_2, rp2, 0, 0];  KRON: [a, b, c, d, taps, layout]
    __device__ __forceinline__ int rp() const { return (int)x[0]; }
    __device__ __forceinline__ const void* p2() const { return (const void*)x[1]; }
    __device__ __forceinline__ const void* p3() const { return (const void*)x[2]; }
    __device__ __forceinline__ int rp2() const { return (int)x[3]; }
    __device__ __forceinline__ int b() const { return (int)x[1]; }
    __device__ __forceinline__ int c() const { return (int)x[2]; }
    __device__ __forceinline__ int d() const { return (int)x[3]; }
    __device__ __forceinline__ int taps() const { return (int)x[4]; }
    __device__ __forceinline__ int layout() const { return (int)x[5]; }
};

__device__ __forceinline__ Segment load_segment(const long long* __restrict__ segments, int j) {
    const long long* sg = segments + (long)j * SEG_WORDS;
    Segment s;
    s.kind = (int)sg[0], s.slot = (int)sg[1], s.mag = sg[2], s.ws = sg[3];
    s.p0 = (const void*)sg[4], s.p1 = (const void*)sg[5];
#pragma unroll
    for (int i = 0; i < 6; ++i) s.x[i] = sg[6 + i];
    return s;
}

// KRON's index map for column k of the weight's (N, K) view: W1's column j and W2's column col (see the header of this file)
struct KronMap {
    int I, dd;      // columns per tap; consecutive columns that share W1's scalar
    __device__ __forceinline__ KronMap(const Segment& s) : I(s.layout() ? s.b() * s.d() : s.b() * s.d() * s.taps()), dd(s.layout() ? s.d() : s.d() * s.taps()) {}
    __device__ __forceinline__ void at(int k, int& j, int& col) const {
        const int tap = k / I, ch = k - tap * I;
        j = ch / dd;
        col = tap * dd + ch - j * dd;
    }
    // (j, col) of column k and of the columns after it: two divisions at the start, compares and adds from there on
    struct Walk {
        int j, col, q, ch;
    };
    __device__ __forceinline__ Walk start(int k) const {
        const int tap = k / I, ch = k - tap * I, j = ch / dd, q = ch - j * dd;
        return Walk{j, tap * dd + q, q, ch};
    }
    __device__ __forceinline__ void next(Walk& w) const {
        ++w.col, ++w.q, ++w.ch;
        if (w.q == dd) w.q = 0, ++w.j, w.col -= dd;              // W1's next column: W2's row starts over
        if (w.ch == I) w.ch = 0, w.j = 0, w.col += dd;           // the next tap: W1's row starts over, W2's row runs on
    }
};

struct Target {
    char* w;
    const char* base;
    int N, K, seg0, nseg;
};

__device__ __forceinline__ Target load_target(const long long* __restrict__ targets, int t) {
    const long long* d = targets + (long)t * TGT_WORDS;
    Target r;
    r.w = (char*)d[0];
    r.base = (const char*)d[1];
    r.N = (int)d[2];
    r.K = (int)d[3];
    r.seg0 = (int)d[4];
    r.nseg = (int)d[5];
    return r;
}

// base + delta for VEC consecutive k of row n, rounded once; 16-byte accesses when the target allows them (K a multiple of
// VEC and both images 16-byte aligned), elementwise with a bound check per value otherwise.  `merged` false: the base's bits.
// DORA: the base is scaled by `bcoef` (one fma; bcoef == 1 gives the plain form's bits).
template <typename T, bool DORA = false>
__device__ __forceinline__ void finish_row(const Target& tg, int n, int k, const float* delta, bool merged, bool vec, float bcoef = 1.f) {
    constexpr int VEC = Elem<T>::VEC;
    if (n >= tg.N || k >= tg.K) return;
    const long at = (long)n * tg.K + k;
    const T* b = reinterpret_cast<const T*>(tg.base) + at;
    T* w = reinterpret_cast<T*>(tg.w) + at;
    if (vec) {                                   // k + VEC <= K: k and K are multiples of VEC
        Vec16<T> v = load16(b);
        if (merged) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) v.set(i, DORA ? fmaf(bcoef, v.get(i), delta[i]) : v.get(i) + delta[i]);
        }
        store16(w, v);
    } else {
        for (int i = 0; i < VEC && k + i < tg.K; ++i)
            w[i] = merged ? Elem<T>::from_f(DORA ? fmaf(bcoef, Elem<T>::to_f(b[i]), delta[i]) : Elem<T>::to_f(b[i]) + delta[i]) : b[i];
    }
}

// fp32 base values of VEC consecutive k of row n, 0 past the weight's edge (never read there): the norm pass's operand
template <typename T>
__device__ __forceinline__ void base_row(const Target& tg, int n, int k, bool vec, float* out) {
    constexpr int VEC = Elem<T>::VEC;
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] = 0.f;
    if (n >= tg.N || k >= tg.K) return;
    const T* b = reinterpret_cast<const T*>(tg.base) + (long)n * tg.K + k;
    if (vec) {
        const Vec16<T> v = load16(b);
#pragma unroll
        for (int i = 0; i < VEC; ++i) out[i] = v.get(i);
    } else {
        for (int i = 0; i < VEC && k + i < tg.K; ++i) out[i] = Elem<T>::to_f(b[i]);
    }
}

// One of the `stride` interleaved chains of a row's partial sums of squares (one partial per K-tile): K-tiles first,
// first + stride, ...  The lanes that share a row take one chain each and join them by a fixed xor tree, so the row's
// ceil(K / 128) loads (90 for SDXL's widest conv) are neither repeated by every lane nor one serial chain.
__device__ __forceinline__ float dora_chain(const float* __restrict__ partials, int n, int N, int tiles_k, int first, int stride) {
    float ss = 0.f;
#pragma unroll 4
    for (int kt = first; kt < tiles_k; kt += stride) ss += partials[(long)kt * N + n];
    return ss;
}

// g[n] = m[n] / ||V[n, :]|| from the row's sum of squares.  A row of V that is exactly zero has no direction to scale (PEFT
// divides by zero there): its gain is 0, so the row's g V is the zero it already was and nothing non-finite reaches the weight.
__device__ __forceinline__ float dora_gain(float ss, float m) { return ss > 0.f ? m / sqrtf(ss) : 0.f; }

template <typename T> struct Mfma16;
template <> struct Mfma16<bf16> {
    static __device__ __forceinline__ f32x4 run(const bf16x8& a, const bf16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma16<f16> {
    static __device__ __forceinline__ f32x4 run(const f16x8& a, const f16x8& b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

// LDS images of one segment's factor tiles.  Rows are padded by 16 bytes: (rp + 8) * 2 bytes = 4 (rp / 8 + 1) banks, an odd
// multiple of 4 for every rp that is a multiple of 32, so 16 consecutive rows read as 16-byte chunks cover all 64 banks
// once.  The images are sized by the launch's largest padded rank (15 KiB at rank <= 32, 51 KiB at 128), which sets how many
// workgroups share a CU.  The DownT rows are stored in MFMA order - tile row k = 32 p + 8 a + 4 h + b lives in
// image row 32 p + 16 h + 4 a + b - so the 16 lanes of an operand read take 16 consecutive image rows.
static inline int lora_lds_row(int max_rank) { return (max_rank + 8) * 2; }      // bytes

// One factor pair's product for the workgroup's tile, acc += DownT . Up^T over the pair's padded rank: the factor rows of the
// tile are staged in the LDS images (after a barrier when an earlier product still reads them), then multiplied.
// Both tiles are contiguous in memory (whole rows of row-major factors): coalesced 16-byte copies.  Rows past the
// weight's edge are not read; what the image holds there only reaches outputs that are never stored.
template <typename T>
__device__ __forceinline__ void lora_product16(const T* __restrict__ up, const T* __restrict__ down_t, int rp, int rows_n, int rows_k,
                                               char* lds_down, char* lds_up, int lds_row, bool& staged, f32x4 (&acc)[8]) {
    typedef typename V16<T>::x8 frag;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int chunks = rp >> 3;                                  // 16-byte chunks per factor row
    if (staged) __syncthreads();                                // the previous product's images have been read
    staged = true;
    for (int q = threadIdx.x; q < rows_k * chunks; q += LORA_THREADS) {
        const int row = q / chunks, col = q - row * chunks;
        const int img = (row & ~31) + 16 * ((row >> 2) & 1) + 4 * ((row >> 3) & 3) + (row & 3);
        *reinterpret_cast<frag*>(lds_down + img * lds_row + col * 16) = *reinterpret_cast<const frag*>(down_t + (long)q * 8);
    }
    for (int q = threadIdx.x; q < rows_n * chunks; q += LORA_THREADS) {
        const int row = q / chunks, col = q - row * chunks;
        *reinterpret_cast<frag*>(lds_up + row * lds_row + col * 16) = *reinterpret_cast<const frag*>(up + (long)q * 8);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < rp; r0 += 32) {
        const int col = (r0 + 8 * g) * 2;
        const frag b = *reinterpret_cast<const frag*>(lds_up + (wave * 16 + c) * lds_row + col);
#pragma unroll
        for (int i = 0; i < 8; ++i) {                           // i = 2 p + h: image rows 16 i .. 16 i + 15
            const frag a = *reinterpret_cast<const frag*>(lds_down + (16 * i + c) * lds_row + col);
            acc[i] = Mfma16<T>::run(a, b, acc[i]);
        }
    }
}

// KRON: the lane's 4 x 8 values of row n (acc[2 p] and acc[2 p + 1] hold k = kb + 32 p .. + 7, as the MFMA layout leaves
// them).  Rows and columns past the weight's edge are clamped to it: such values are never stored and count as 0 in a norm.
__device__ __forceinline__ void kron_tile16(const Segment& sg, const Target& tg, int n, int kb, f32x4 (&acc)[8]) {
    const KronMap map(sg);
    n = min(n, tg.N - 1);
    const int i1 = n / sg.c();
    const float* __restrict__ w1 = (const float*)sg.p0 + (long)i1 * sg.b();
    const float* __restrict__ w2 = (const float*)sg.p1 + (long)(n - i1 * sg.c()) * (sg.d() * sg.taps());
    const bool kvec = map.dd % 8 == 0;                          // then I and K are multiples of 8 too: 8 aligned columns share j and the tap
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int k = kb + 32 * p;
        if (kvec) {
            int j, col;
            map.at(min(k, tg.K - 8), j, col);
            const float s = w1[j];
            const f32x4 lo = *reinterpret_cast<const f32x4*>(w2 + col), hi = *reinterpret_cast<const f32x4*>(w2 + col + 4);
            acc[2 * p] = s * lo;
            acc[2 * p + 1] = s * hi;
        } else {
            KronMap::Walk at = map.start(min(k, tg.K - 1));
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                acc[2 * p + (e >> 2)][e & 3] = w1[at.j] * w2[at.col];
                if (k + e + 1 < tg.K) map.next(at);
            }
        }
    }
}

template <typename T, int MODE, bool FORMS>
__global__ __launch_bounds__(LORA_THREADS) void lora_merge16_kernel(const long long* __restrict__ targets, const long long* __restrict__ segments,
                                                                   const int* __restrict__ tiles, const float* __restrict__ scales, int lds_row,
                                                                   float* __restrict__ workspace) {
    extern __shared__ __attribute__((aligned(16))) char lds_down[];
    char* lds_up = lds_down + LORA_TK * lds_row;
    const int t = tiles[2 * blockIdx.x], tile = tiles[2 * blockIdx.x + 1];
    const Target tg = load_target(targets, t);
    const int tiles_k = (tg.K + LORA_TK - 1) / LORA_TK;
    const int nt = (tile / tiles_k) * LORA_TN, k0 = (tile % tiles_k) * LORA_TK;
    const int wave = threadIdx.x >> 6, n0 = nt + wave * 16;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const bool vec = tg.K % 8 == 0 && (((uintptr_t)tg.w | (uintptr_t)tg.base) & 15) == 0;
    const int rows_k = min(LORA_TK, tg.K - k0), rows_n = min(LORA_TN, tg.N - nt);      // rows of the factors this tile may read
    // the base's 16-byte vectors are requested first: they come from HBM while the factors are staged and multiplied
    Vec16<T> basev[4];
    float basef[MODE == MODE_NORM ? 4 : 1][8];                  // (norm pass) the same values as floats, 0 past the edge
    if constexpr (MODE == MODE_NORM) {
#pragma unroll
        for (int p = 0; p < 4; ++p) base_row<T>(tg, n0 + c, k0 + 32 * p + 8 * g, vec, basef[p]);
    } else if (vec && n0 + c < tg.N) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (k0 + 32 * p + 8 * g < tg.K)
                basev[p] = load16(reinterpret_cast<const T*>(tg.base) + (long)(n0 + c) * tg.K + k0 + 32 * p + 8 * g);
    }
    f32x4 sum[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) sum[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bcoef = 1.f;                                          // (DoRA) 1 + sum_j (g_j[n] - 1), what the base is scaled by
    bool merged = false, staged = false;
    for (int j = 0; j < tg.nseg; ++j) {
        const Segment sg = load_segment(segments, tg.seg0 + j);
        const float s = scales[sg.slot];
        if (s == 0.f) continue;                                 // (uniform) an adapter at scale 0 contributes nothing, whatever it holds
        if (!FORMS && sg.kind != KIND_PLAIN) continue;          // (uniform) a wrong `forms` flag drops a segment; its tables are never read as factors
        if (MODE == MODE_NORM && sg.mag == 0) continue;         // (uniform) a plain segment has no norm
        // (uniform; a table that breaks the max_rank contract: no image overrun)
        if (sg.kind != KIND_KRON && ((sg.rp() + 8) * 2 > lds_row || (sg.rp2() + 8) * 2 > lds_row)) continue;
        merged = true;
        // ---- the segment's fp32 tile: the only part that knows the kind (every branch is workgroup-uniform) ----
        f32x4 acc[8];
        if (FORMS && sg.kind == KIND_KRON) {
            kron_tile16(sg, tg, n0 + c, k0 + 8 * g, acc);
        } else {
            lora_product16<T>((const T*)sg.p0 + (long)nt * sg.rp(), (const T*)sg.p1 + (long)k0 * sg.rp(), sg.rp(), rows_n, rows_k, lds_down, lds_up,
                              lds_row, staged, acc);
            if (FORMS && sg.kind == KIND_HADA) {
                f32x4 acc2[8];
                lora_product16<T>((const T*)sg.p2() + (long)nt * sg.rp2(), (const T*)sg.p3() + (long)k0 * sg.rp2(), sg.rp2(), rows_n, rows_k, lds_down,
                                  lds_up, lds_row, staged, acc2);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] *= acc2[i];
            }
        }
        if constexpr (MODE == MODE_NORM) {
            // the lane's 32 values of row n0 + c in a fixed order (values past the edge - the images hold anything there -
            // count as 0), then the row's four lane groups by a fixed xor tree: every one of them ends with the same sum
            float ss = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = k0 + 32 * (i >> 1) + 8 * g + 4 * (i & 1) + e;
                    const float v = (n0 + c < tg.N && k < tg.K) ? fmaf(s, acc[i][e], basef[i >> 1][4 * (i & 1) + e]) : 0.f;
                    ss = fmaf(v, v, ss);
                }
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            if (g == 0 && n0 + c < tg.N) workspace[sg.ws + (long)(tile % tiles_k) * tg.N + n0 + c] = ss;
        } else {
            float coef = s;
            if constexpr (MODE == MODE_DORA) {
                if (sg.mag != 0) {                              // (uniform) rows past the edge take the last row's gain and are never stored
                    // a row's four lane groups add one chain of its partials each; the xor tree leaves the same sum in all four
                    const int n = min(n0 + c, tg.N - 1);
                    float ss = dora_chain(workspace + sg.ws, n, tg.N, tiles_k, g, 4);
                    ss += __shfl_xor(ss, 16);
                    ss += __shfl_xor(ss, 32);
                    const float gain = dora_gain(ss, ((const float*)sg.mag)[n]);
                    bcoef += gain - 1.f;
                    coef = gain * s;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[i][e] = fmaf(coef, acc[i][e], sum[i][e]);
        }
    }
    if constexpr (MODE == MODE_NORM) return;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float delta[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            delta[e] = sum[2 * p][e];
            delta[4 + e] = sum[2 * p + 1][e];
        }
        const int n = n0 + c, k = k0 + 32 * p + 8 * g;
        if (!vec) {
            finish_row<T, MODE == MODE_DORA>(tg, n, k, delta, merged, false, bcoef);
        } else if (n < tg.N && k < tg.K) {                      // k + 8 <= K: k and K are multiples of 8
            if (merged) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    basev[p].set(e, MODE == MODE_DORA ? fmaf(bcoef, basev[p].get(e), delta[e]) : basev[p].get(e) + delta[e]);
            }
            store16(reinterpret_cast<T*>(tg.w) + (long)n * tg.K + k, basev[p]);
        }
    }
}

// fp32: thread (rg, cg) owns rows 8 rg .. 8 rg + 7 and columns 4 cg .. 4 cg + 3 of the tile; factors are read four ranks at a time
__device__ __forceinline__ void lora_product32(const float* __restrict__ up, const float* __restrict__ down_t, int rp, const Target& tg, int n0,
                                               int k0, float (&acc)[8][4]) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
    for (int r0 = 0; r0 < rp; r0 += 4) {
        f32x4 d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            d[e] = *reinterpret_cast<const f32x4*>(down_t + (long)min(k0 + e, tg.K - 1) * rp + r0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 u = *reinterpret_cast<const f32x4*>(up + (long)min(n0 + i, tg.N - 1) * rp + r0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][e] = fmaf(u[q], d[e][q], acc[i][e]);
        }
    }
}

// KRON in fp32: the thread's four columns are mapped once, its eight rows then read two small tables through the cache
__device__ __forceinline__ void kron_tile32(const Segment& sg, const Target& tg, int n0, int k0, float (&acc)[8][4]) {
    const KronMap map(sg);
    int jj[4], cc[4];
    KronMap::Walk at = map.start(min(k0, tg.K - 1));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        jj[e] = at.j, cc[e] = at.col;
        if (k0 + e + 1 < tg.K) map.next(at);
    }
    const float* __restrict__ w1 = (const float*)sg.p0;
    const float* __restrict__ w2 = (const float*)sg.p1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int n = min(n0 + i, tg.N - 1), i1 = n / sg.c();
        const float* r1 = w1 + (long)i1 * sg.b();
        const float* r2 = w2 + (long)(n - i1 * sg.c()) * (sg.d() * sg.taps());
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = r1[jj[e]] * r2[cc[e]];
    }
}

template <int MODE, bool FORMS>
__global__ __launch_bounds__(LORA_THREADS) void lora_merge32_kernel(const long long* __restrict__ targets, const long long* __restrict__ segments,
                                                                   const int* __restrict__ tiles, const float* __restrict__ scales,
                                                                   float* __restrict__ workspace) {
    const int t = tiles[2 * blockIdx.x], tile = tiles[2 * blockIdx.x + 1];
    const Target tg = load_target(targets, t);
    const int tiles_k = (tg.K + LORA_TK - 1) / LORA_TK;
    const int n0 = (tile / tiles_k) * LORA_TN + (threadIdx.x >> 5) * 8, k0 = (tile % tiles_k) * LORA_TK + (threadIdx.x & 31) * 4;
    const bool vec = tg.K % 4 == 0 && (((uintptr_t)tg.w | (uintptr_t)tg.base) & 15) == 0;
    float sum[8][4];
    float basef[MODE == MODE_NORM ? 8 : 1][4];
    float bcoef[MODE == MODE_DORA ? 8 : 1];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[i][e] = 0.f;
        if constexpr (MODE == MODE_NORM) base_row<float>(tg, n0 + i, k0, vec, basef[i]);
        if constexpr (MODE == MODE_DORA) bcoef[i] = 1.f;
    }
    bool merged = false;
    for (int j = 0; j < tg.nseg; ++j) {
        const Segment sg = load_segment(segments, tg.seg0 + j);
        const float s = scales[sg.slot];
        if (s == 0.f) continue;
        if (!FORMS && sg.kind != KIND_PLAIN) continue;          // (uniform; see the 16-bit kernel)
        if (MODE == MODE_NORM && sg.mag == 0) continue;
        merged = true;
        float acc[8][4];
        if (FORMS && sg.kind == KIND_KRON) {
            kron_tile32(sg, tg, n0, k0, acc);
        } else {
            lora_product32((const float*)sg.p0, (const float*)sg.p1, sg.rp(), tg, n0, k0, acc);
            if (FORMS && sg.kind == KIND_HADA) {
                float acc2[8][4];
                lora_product32((const float*)sg.p2(), (const float*)sg.p3(), sg.rp2(), tg, n0, k0, acc2);
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][e] *= acc2[i][e];
            }
        }
        if constexpr (MODE == MODE_NORM) {
            // a row's 128 columns sit in the 32 lanes of one half wave: four values per lane, then a fixed xor tree inside the half
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float ss = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = (n0 + i < tg.N && k0 + e < tg.K) ? fmaf(s, acc[i][e], basef[i][e]) : 0.f;
                    ss = fmaf(v, v, ss);
                }
#pragma unroll
                for (int m = 1; m < 32; m <<= 1) ss += __shfl_xor(ss, m);
                if ((threadIdx.x & 31) == 0 && n0 + i < tg.N) workspace[sg.ws + (long)(tile % tiles_k) * tg.N + n0 + i] = ss;
            }
        } else {
            // (DoRA) the 32 lanes of a half wave share their 8 rows: lane l adds chain l >> 3 (of four) of row l & 7, an xor tree
            // joins the chains, and every lane then takes row i's gain from lane i of its half
            float mine = 0.f;
            if constexpr (MODE == MODE_DORA) {
                if (sg.mag != 0) {                              // (uniform)
                    const int l = threadIdx.x & 31, n = min(n0 + (l & 7), tg.N - 1);
                    float ss = dora_chain(workspace + sg.ws, n, tg.N, tiles_k, l >> 3, 4);
                    ss += __shfl_xor(ss, 8);
                    ss += __shfl_xor(ss, 16);
                    mine = dora_gain(ss, ((const float*)sg.mag)[n]);
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float coef = s;
                if constexpr (MODE == MODE_DORA) {
                    if (sg.mag != 0) {                          // (uniform)
                        const float gain = __shfl(mine, (int)(threadIdx.x & 32) + i);
                        bcoef[i] += gain - 1.f;
                        coef = gain * s;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[i][e] = fmaf(coef, acc[i][e], sum[i][e]);
            }
        }
    }
    if constexpr (MODE == MODE_NORM) return;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        finish_row<float, MODE == MODE_DORA>(tg, n0 + i, k0, sum[i], merged, vec, MODE == MODE_DORA ? bcoef[i] : 1.f);
}

template <int MODE, bool FORMS>
static int lora_launch(const char* what, const long long* targets, const long long* segments, int max_rank, const int* tiles, long n_tiles,
                       const float* scales, float* workspace, int dtype, hipStream_t st) {
    const dim3 grid((unsigned)n_tiles), block(LORA_THREADS);
    const int lds_row = lora_lds_row((max_rank + 31) / 32 * 32);
    const size_t lds = (size_t)(LORA_TK + LORA_TN) * lds_row;
    if (dtype == ST_BF16)
        hipLaunchKernelGGL((lora_merge16_kernel<bf16, MODE, FORMS>), grid, block, lds, st, targets, segments, tiles, scales, lds_row, workspace);
    else if (dtype == ST_F16)
        hipLaunchKernelGGL((lora_merge16_kernel<f16, MODE, FORMS>), grid, block, lds, st, targets, segments, tiles, scales, lds_row, workspace);
    else                                                          // ST_F32: the entry point has checked the dtype
        hipLaunchKernelGGL((lora_merge32_kernel<MODE, FORMS>), grid, block, 0, st, targets, segments, tiles, scales, workspace);
    return st_check_launch(what);
}

// the norm pass (when any segment has a magnitude), then the merge, in the FORMS instantiations or the lean ones
template <bool FORMS>
static int lora_passes(const long long* targets, const long long* segments, int max_rank, const int* tiles, long n_tiles, const int* norm_tiles,
                       long n_norm_tiles, const float* scales, float* workspace, int dtype, hipStream_t st) {
    if (!FORMS && n_norm_tiles == 0)
        return lora_launch<MODE_PLAIN, false>("lora_merge", targets, segments, max_rank, tiles, n_tiles, scales, nullptr, dtype, st);
    if (n_norm_tiles > 0) {
        const int rc = lora_launch<MODE_NORM, FORMS>("lora_merge (norm pass)", targets, segments, max_rank, norm_tiles, n_norm_tiles, scales,
                                                     workspace, dtype, st);
        if (rc) return rc;
    }
    return lora_launch<MODE_DORA, FORMS>("lora_merge", targets, segments, max_rank, tiles, n_tiles, scales, workspace, dtype, st);
}

}  // namespace

extern "C" int st_lora_merge(const long long* targets, int n_targets, const long long* segments, int n_segments, int max_rank,
                             const int* tiles, long n_tiles, const int* norm_tiles, long n_norm_tiles, const float* scales, int n_scales,
                             float* workspace, size_t workspace_bytes, int dtype, int forms, void* stream) {
    ST_REQUIRE(targets && tiles && scales && (segments || n_segments == 0), "lora_merge: null pointer");
    ST_REQUIRE(n_targets > 0 && n_segments >= 0 && n_scales > 0, "lora_merge: bad sizes (targets %d, segments %d, scales %d)",
               n_targets, n_segments, n_scales);      // (a target without segments is restored to its base)
    ST_REQUIRE(n_tiles > 0 && n_tiles <= 0x7fffffffL && n_norm_tiles >= 0 && n_norm_tiles <= n_tiles,
               "lora_merge: %ld tiles, %ld norm tiles (a launch takes 1 .. 2^31 - 1; the norm pass covers a subset of the targets)",
               n_tiles, n_norm_tiles);
    ST_REQUIRE(n_norm_tiles == 0 || (norm_tiles && workspace && workspace_bytes >= 4),
               "lora_merge: the norm pass needs its tile list and a workspace");
    ST_REQUIRE((uintptr_t)targets % 8 == 0 && (uintptr_t)segments % 8 == 0 && (uintptr_t)tiles % 4 == 0 && (uintptr_t)norm_tiles % 4 == 0 &&
               (uintptr_t)scales % 4 == 0 && (uintptr_t)workspace % 4 == 0, "lora_merge: misaligned table");
    // (0: no segment, or every segment is a Kronecker one - nothing is staged)
    ST_REQUIRE(max_rank >= 0 && max_rank <= ST_LORA_MAX_RANK && (max_rank > 0 || n_segments == 0 || forms),
               "lora_merge: max_rank %d (the largest padded rank of any factor pair, 1 .. %d; 0 when nothing is staged)", max_rank,
               (int)ST_LORA_MAX_RANK);
    ST_REQUIRE(dtype == ST_BF16 || dtype == ST_F16 || dtype == ST_F32, "lora_merge: unsupported dtype %d", dtype);
    hipStream_t st = (hipStream_t)stream;
    return forms ? lora_passes<true>(targets, segments, max_rank, tiles, n_tiles, norm_tiles, n_norm_tiles, scales, workspace, dtype, st)
                 : lora_passes<false>(targets, segments, max_rank, tiles, n_tiles, norm_tiles, n_norm_tiles, scales, workspace, dtype, st);
}
