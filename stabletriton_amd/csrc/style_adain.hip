// Token-axis AdaIN on column slices of the fused q|k|v projection (include/stabletriton_amd.h, st_style_adain) - StyleAligned's
// renormalisation of the queries and keys: within every block of `per` batch entries, entry b (b % per != 0) is rewritten in place as
//     x[b,t,c] <- (x[b,t,c] - mu[b,c]) / sd[b,c] * sd[s,c] + mu[s,c],        s = b - b % per, the block's style row,
// mu / sd the mean and sqrt(unbiased variance + 1e-5) over the T tokens of one (entry, channel).  Style rows are never written.
//
// Two launches over the same tiling: a slab of SA_SLAB tokens x a strip of SA_STRIP channels x slice x batch entry.
//   stats  every entry.  A lane owns 8 channels (one 16-byte load) of every 16th token row of the slab: 16 lanes span the strip, a wave
//          load covers 4 rows, the four waves 16.  Per channel a running (count, mean, M2) in fp32 - Welford, because q and k have
//          means as large as their spread, so sum / sum of squares would cancel; the four rows of a wave meet by two shuffles, the
//          four waves through LDS in wave order, every meeting Chan's pairwise combination.  One (mean, M2) partial per (slice, entry,
//          slab, channel) goes to the workspace; its count is the slab's row count, which the reader knows.
//   apply  the non-style entries only.  The first 128 threads of a block each combine one channel's slab partials, in slab order, for
//          the block's entry and for its style row, and leave a = sd_s / sd_o, c = mu_s - mu_o * a in LDS; then the block streams its
//          slab: 16-byte load, one fp32 fma per value, one rounding, 16-byte store in place.
// The combination tree is fixed by the shape: no atomics, no tickets, the same bits from every run.  Token and channel tails are
// predicated.  With the device gate off (table[clamp(*step)] == 0: two scalar loads of values no launch writes) both kernels leave
// before touching x or the workspace.
#include "common.h"

namespace {

constexpr int SA_THREADS = 256;
constexpr int SA_SLAB = 256;           // token rows per block
constexpr int SA_STRIP = 128;          // channels per block: 16 lanes x 8 values
constexpr int SA_ROWS = 16;            // token rows per block pass: 4 waves x 4 rows
constexpr float SA_EPS = 1e-5f;

template <typename E>
struct AdainArgs {
    E* x[3];
    long ld[3];
    int B, T, C, per, nslab;
    float2* ws;                        // [slice][b][slab][C] (mean, M2)
    const float* table;
    const int* step;
    int n;
};

__device__ __forceinline__ bool sa_gate_on(const float* table, const int* step, int n) {
    if (!table) return true;
    const int i = *step;
    return table[i < 0 ? 0 : (i >= n ? n - 1 : i)] != 0.f;
}

// Chan, Golub, LeVeque: (na, ma, Ma) <- the statistics of the union with (nb, mb, Mb)
__device__ __forceinline__ void sa_combine(int na, float& ma, float& Ma, int nb, float mb, float Mb) {
    const int n = na + nb;
    const float f = n ? (float)nb / (float)n : 0.f;
    const float d = mb - ma;
    ma = fmaf(d, f, ma);
    Ma = (Ma + Mb) + d * d * ((float)na * f);
}

template <typename E>
__device__ __forceinline__ E* sa_slice(const AdainArgs<E>& a, int s, long& ld) {
    ld = s == 0 ? a.ld[0] : s == 1 ? a.ld[1] : a.ld[2];
    return s == 0 ? a.x[0] : s == 1 ? a.x[1] : a.x[2];
}

template <typename E>
__global__ __launch_bounds__(SA_THREADS) void style_adain_stats_kernel(const AdainArgs<E> a) {
    __shared__ float red[4][2][SA_STRIP];
    __shared__ int cnt[4];
    if (!sa_gate_on(a.table, a.step, a.n)) return;                // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, rl = lane >> 4;
    const int slab = blockIdx.x, strip = blockIdx.y, s = blockIdx.z / a.B, b = blockIdx.z % a.B;
    long ld;
    const E* x = sa_slice(a, s, ld);
    const int c = strip * SA_STRIP + cl * 8;
    const int t0 = slab * SA_SLAB, t1 = min(a.T, t0 + SA_SLAB);
    float mean[8], m2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) mean[e] = m2[e] = 0.f;
    int n = 0;
    if (c < a.C) {                                                // C % 8 == 0: the whole vector is inside
        const E* p = x + ((long)b * a.T + t0 + wave * 4 + rl) * ld + c;
        for (int t = t0 + wave * 4 + rl; t < t1; t += SA_ROWS, p += SA_ROWS * ld) {
            const Vec16<E> v = load16(p);
            n += 1;
            const float rn = 1.0f / (float)n;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = v.get(e), d = f - mean[e];
                mean[e] = fmaf(d, rn, mean[e]);
                m2[e] = fmaf(d, f - mean[e], m2[e]);
            }
        }
    }
    // the four rows of the wave: rows (0, 1), then ((0, 1), (2, 3)); lanes 0..15 hold the wave's result
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const int nb = __shfl_down(n, off, 64);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float mb = __shfl_down(mean[e], off, 64), Mb = __shfl_down(m2[e], off, 64);
            sa_combine(n, mean[e], m2[e], nb, mb, Mb);
        }
        n += nb;
    }
    if (lane < 16) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            red[wave][0][cl * 8 + e] = mean[e];
            red[wave][1][cl * 8 + e] = m2[e];
        }
        if (lane == 0) cnt[wave] = n;                             // (lane 0's channels are inside: the strip starts below C)
    }
    __syncthreads();
    const int ch = strip * SA_STRIP + tid;
    if (tid < SA_STRIP && ch < a.C) {
        int na = cnt[0];
        float ma = red[0][0][tid], Ma = red[0][1][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            sa_combine(na, ma, Ma, cnt[w], red[w][0][tid], red[w][1][tid]);
            na += cnt[w];
        }
        a.ws[(((long)s * a.B + b) * a.nslab + slab) * a.C + ch] = make_float2(ma, Ma);
    }
}

template <typename E>
__global__ __launch_bounds__(SA_THREADS) void style_adain_apply_kernel(const AdainArgs<E> a) {
    __shared__ float sa[SA_STRIP], sc[SA_STRIP];
    if (!sa_gate_on(a.table, a.step, a.n)) return;                // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 15, rl = lane >> 4;
    const int slab = blockIdx.x, strip = blockIdx.y;
    const int nns = a.B - (a.B + a.per - 1) / a.per;              // non-style entries; the host launches none when this is 0
    const int s = blockIdx.z / nns, j = blockIdx.z % nns;
    const int bs = j / (a.per - 1) * a.per, b = bs + j % (a.per - 1) + 1;      // the j-th non-style entry and its style row
    const int ch = strip * SA_STRIP + tid;
    if (tid < SA_STRIP && ch < a.C) {
        const float2* po = a.ws + (((long)s * a.B + b) * a.nslab) * a.C + ch;
        const float2* ps = a.ws + (((long)s * a.B + bs) * a.nslab) * a.C + ch;
        float2 o = po[0], y = ps[0];
        int na = min(a.T, SA_SLAB);
        for (int k = 1; k < a.nslab; ++k) {                       // in slab order
            const int nb = min(a.T - k * SA_SLAB, SA_SLAB);
            const float2 o2 = po[(long)k * a.C], y2 = ps[(long)k * a.C];
            sa_combine(na, o.x, o.y, nb, o2.x, o2.y);
            sa_combine(na, y.x, y.y, nb, y2.x, y2.y);
            na += nb;
        }
        const float inv = 1.0f / (float)(a.T - 1);
        const float sd_o = sqrtf(fmaf(o.y, inv, SA_EPS)), sd_s = sqrtf(fmaf(y.y, inv, SA_EPS));
        const float g = sd_s / sd_o;
        sa[tid] = g;
        sc[tid] = fmaf(-o.x, g, y.x);
    }
    __syncthreads();
    const int c = strip * SA_STRIP + cl * 8;
    if (c >= a.C) return;
    float g[8], h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        g[e] = sa[cl * 8 + e];
        h[e] = sc[cl * 8 + e];
    }
    long ld;
    E* x = sa_slice(a, s, ld);
    const int t0 = slab * SA_SLAB, t1 = min(a.T, t0 + SA_SLAB);
    E* p = x + ((long)b * a.T + t0 + wave * 4 + rl) * ld + c;
    for (int t = t0 + wave * 4 + rl; t < t1; t += SA_ROWS, p += SA_ROWS * ld) {
        Vec16<E> v = load16(p);
#pragma unroll
        for (int e = 0; e < 8; ++e) v.set(e, fmaf(v.get(e), g[e], h[e]));
        store16(p, v);
    }
}

template <typename E>
int style_adain_launch(const AdainArgs<E>& a, int n_slices, hipStream_t st) {
    const int nstrip = (a.C + SA_STRIP - 1) / SA_STRIP;
    hipLaunchKernelGGL(style_adain_stats_kernel<E>, dim3(a.nslab, nstrip, n_slices * a.B), dim3(SA_THREADS), 0, st, a);
    if (int e = st_check_launch("style_adain (stats)")) return e;
    const int nns = a.B - (a.B + a.per - 1) / a.per;
    hipLaunchKernelGGL(style_adain_apply_kernel<E>, dim3(a.nslab, nstrip, n_slices * nns), dim3(SA_THREADS), 0, st, a);
    return st_check_launch("style_adain (apply)");
}

}  // namespace

extern "C" long st_style_adain_workspace(int B, int T, int C, int n_slices) {
    if (B < 1 || T < 1 || C < 1 || n_slices < 1) return 0;
    return 2L * n_slices * B * ((T + SA_SLAB - 1) / SA_SLAB) * C;
}

extern "C" int st_style_adain(void* x0, void* x1, void* x2, int n_slices, int B, int T, int C, long ld0, long ld1, long ld2, int per,
                              float* workspace, long workspace_floats, const float* gate_table, const int* gate_step, int gate_n,
                              int dtype, void* stream) {
    ST_REQUIRE(n_slices >= 1 && n_slices <= 3, "style_adain: %d slices (1 to 3)", n_slices);
    void* const xs[3] = {x0, x1, x2};
    const long lds[3] = {ld0, ld1, ld2};
    ST_REQUIRE(B > 0 && C > 0 && per >= 1, "style_adain: bad shape B=%d C=%d per=%d", B, C, per);
    ST_REQUIRE(T >= 2, "style_adain: T = %d, the unbiased variance needs two tokens", T);
    ST_REQUIRE(dtype == ST_BF16 || dtype == ST_F16, "style_adain: 16-bit types only (dtype %d); other types take the host's slow path", dtype);
    ST_REQUIRE(C % 8 == 0, "style_adain: C = %d must be a multiple of 8", C);
    for (int s = 0; s < n_slices; ++s) {
        ST_REQUIRE(xs[s], "style_adain: null pointer (slice %d)", s);
        ST_REQUIRE((uintptr_t)xs[s] % 16 == 0 && lds[s] % 8 == 0, "style_adain: slices and their token strides must keep 16-byte alignment");
        ST_REQUIRE(lds[s] >= C && lds[s] < (1L << 31), "style_adain: token stride %ld must hold C = %d values and fit 31 bits", lds[s], C);
    }
    // the affine is in place: two slices that share an element would race.  Slices whose byte ranges meet must be column slices of
    // one buffer (the same token stride) whose column ranges do not meet
    for (int i = 0; i < n_slices; ++i)
        for (int j = i + 1; j < n_slices; ++j) {
            const long span_i = ((long)B * T - 1) * lds[i] + C, span_j = ((long)B * T - 1) * lds[j] + C;      // in elements
            const long d = ((char*)xs[j] - (char*)xs[i]) / 2;                                                  // 16-bit elements
            if (d >= span_i || -d >= span_j) continue;
            const long m = lds[i] == lds[j] ? ((d % lds[i]) + lds[i]) % lds[i] : 0;
            ST_REQUIRE(lds[i] == lds[j] && m >= C && m <= lds[i] - C, "style_adain: slices %d and %d overlap", i, j);
        }
    ST_REQUIRE((gate_table == nullptr) == (gate_step == nullptr), "style_adain: the gate is a table AND a step, or neither");
    ST_REQUIRE(!gate_table || gate_n > 0, "style_adain: gate table of %d entries", gate_n);
    ST_REQUIRE((((uintptr_t)gate_table | (uintptr_t)gate_step) & 3) == 0, "style_adain: misaligned gate pointer");
    const int nns = B - (B + per - 1) / per;
    if (nns == 0) return 0;                                       // every entry is a style row: nothing to rewrite
    const int nslab = (T + SA_SLAB - 1) / SA_SLAB;
    ST_REQUIRE((long)n_slices * B <= 65535 && (C + SA_STRIP - 1) / SA_STRIP <= 65535, "style_adain: too many entries / channels for one launch");
    ST_REQUIRE(workspace && (uintptr_t)workspace % 8 == 0 && workspace_floats >= st_style_adain_workspace(B, T, C, n_slices),
               "style_adain: workspace of %ld floats, %ld needed (st_style_adain_workspace), 8-byte aligned", workspace_floats,
               st_style_adain_workspace(B, T, C, n_slices));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == ST_BF16) {
        const AdainArgs<bf16> a{{(bf16*)x0, (bf16*)x1, (bf16*)x2}, {ld0, ld1, ld2}, B, T, C, per, nslab, (float2*)workspace, gate_table, gate_step, gate_n};
        return style_adain_launch<bf16>(a, n_slices, st);
    }
    const AdainArgs<f16> a{{(f16*)x0, (f16*)x1, (f16*)x2}, {ld0, ld1, ld2}, B, T, C, per, nslab, (float2*)workspace, gate_table, gate_step, gate_n};
    return style_adain_launch<f16>(a, n_slices, st);
}
