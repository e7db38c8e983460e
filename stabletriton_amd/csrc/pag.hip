// Perturbed-attention guidance (PAG; Ahn et al. 2024): the attention core with an identity tail.
//
// In a perturbed self-attention site the softmax matrix of the perturbed batch entries is replaced by the identity, so their
// attention output is v (diffusers' PAGCFGIdentitySelfAttnProcessor2_0).  The perturbed entries are the LAST ident_count of the
// batch, a property of the batch layout ([negative | positive | perturbed] or [positive | perturbed]) that is fixed for a capture,
// so the range is a host argument and the entry point is two launches of code that does not know about each other:
//   st_attention, unmodified, on the leading B - ident_count entries (batches are dense: the same pointers with a smaller B;
//   skipped when that number is 0), and
//   pag_identity_kernel on the tail: a strided row copy of ident_count * T rows of H * D values from row stride ldv to row stride
//   ldo, one 16-byte vector per lane, no matrix work, no atomics, nothing written outside those rows.
// Strict (fp32) mode: the split image armed for the whole output (st_arm_split_output; the output projection reads the image, not
// `out`) is handed on to the attention launch for the rows of its sub-batch; the identity kernel writes the image rows of the
// tail from the values it copies, with split.h's own split_f32 - bit-equal to st_split_f32 of the same values.
#include "common.h"
#include "split.h"

constexpr int PAG_THREADS = 256;

// vector `g` of the tail: row g / vecs_per_row, columns (g % vecs_per_row) * VEC ... + VEC - 1
template <typename T, bool SPLIT>
__global__ __launch_bounds__(PAG_THREADS) void pag_identity_kernel(const T* __restrict__ v, T* __restrict__ out, char* __restrict__ image,
                                                                    long n_vec, int vecs_per_row, long ldv, long ldo, int cols) {
    constexpr int VEC = Elem<T>::VEC;
    const long g = (long)blockIdx.x * PAG_THREADS + threadIdx.x;
    if (g >= n_vec) return;
    const long row = g / vecs_per_row;
    const int col = (int)(g - row * vecs_per_row) * VEC;
    const Vec16<T> x = load16(v + row * ldv + col);
    store16(out + row * ldo + col, x);
    if constexpr (SPLIT) {                       // fp32 only: VEC == 4, col % 4 == 0, cols % 32 == 0
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = x.get(i);
        split_store4(image + (size_t)row * (size_t)cols * 4, col, f);
    }
}

template <typename T>
static int pag_identity_launch(const void* v, void* out, void* image, long rows, int cols, long ldv, long ldo, hipStream_t st) {
    const int vecs_per_row = cols / Elem<T>::VEC;
    const long n_vec = rows * vecs_per_row;
    const long blocks = (n_vec + PAG_THREADS - 1) / PAG_THREADS;
    ST_REQUIRE(blocks < (1L << 31), "attention_pag: too many blocks");
    if constexpr (sizeof(T) == 4) {
        if (image) {
            hipLaunchKernelGGL((pag_identity_kernel<T, true>), dim3((unsigned)blocks), dim3(PAG_THREADS), 0, st, (const T*)v, (T*)out,
                               (char*)image, n_vec, vecs_per_row, ldv, ldo, cols);
            return st_check_launch("attention_pag (identity)");
        }
    }
    hipLaunchKernelGGL((pag_identity_kernel<T, false>), dim3((unsigned)blocks), dim3(PAG_THREADS), 0, st, (const T*)v, (T*)out,
                       (char*)nullptr, n_vec, vecs_per_row, ldv, ldo, cols);
    return st_check_launch("attention_pag (identity)");
}

extern "C" int st_attention_pag(const void* q, const void* k, const void* v, void* out, int B, int T, int S, int H, int D,
                                long ldq, long ldk, long ldv, long ldo, float scale, int dtype, int ident_count, void* stream) {
    ST_REQUIRE(q && k && v && out, "attention_pag: null pointer");
    ST_REQUIRE(B > 0 && T > 0 && S > 0 && H > 0, "attention_pag: bad shape B=%d T=%d S=%d H=%d", B, T, S, H);
    ST_REQUIRE(D == 16 || D == 32 || D == 64 || D == 128, "attention_pag: head_dim %d not supported (16, 32, 64, 128)", D);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_pag: too many heads/batches for one launch");
    ST_REQUIRE(st_dtype_ok(dtype), "attention_pag: unsupported dtype %d", dtype);
    ST_REQUIRE(ident_count >= 0 && ident_count <= B, "attention_pag: ident_count %d outside [0, B = %d]", ident_count, B);
    ST_REQUIRE(ident_count == 0 || T == S, "attention_pag: the identity tail needs self-attention shapes (T == S), got T=%d S=%d", T, S);
    const int vec = st_dtype_is16(dtype) ? 8 : 4;
    const size_t esz = st_dtype_is16(dtype) ? 2 : 4;
    ST_REQUIRE(ldq % vec == 0 && ldk % vec == 0 && ldv % vec == 0 && ldo % vec == 0, "attention_pag: strides must be 16-byte multiples");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16 == 0, "attention_pag: pointers must be 16-byte aligned");
    const int cols = H * D;
    ST_REQUIRE(ldv >= cols && ldo >= cols, "attention_pag: row strides shorter than a row of H * D = %d values", cols);
    void* image = nullptr;
    if (int e = st_take_split_arm("attention_pag", (long)B * T, cols, dtype == ST_F32, &image)) return e;
    const int lead = B - ident_count;
    if (lead > 0) {
        if (image)
            if (int e = st_arm_split_output(image, (long)lead * T, cols)) return e;
        if (int e = st_attention(q, k, v, out, lead, T, S, H, D, ldq, ldk, ldv, ldo, scale, dtype, stream)) return e;
    }
    if (ident_count == 0) return 0;
    const long first = (long)lead * T, rows = (long)ident_count * T;      // (T == S: v's token rows are the output's)
    const char* vt = (const char*)v + (size_t)first * (size_t)ldv * esz;
    char* ot = (char*)out + (size_t)first * (size_t)ldo * esz;
    void* it = image ? (void*)((char*)image + (size_t)first * (size_t)cols * 4) : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) return pag_identity_launch<bf16>(vt, ot, nullptr, rows, cols, ldv, ldo, st);
    if (dtype == ST_F16) return pag_identity_launch<f16>(vt, ot, nullptr, rows, cols, ldv, ldo, st);
    return pag_identity_launch<float>(vt, ot, it, rows, cols, ldv, ldo, st);
}
