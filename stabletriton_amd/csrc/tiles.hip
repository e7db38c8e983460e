// Tiled denoising (MultiDiffusion / Mixture of Diffusers; include/stabletriton_amd.h, st_tile_gather and st_tile_blend): a canvas
// (rows, H, W, C) dense NHWC and its T = ny * nx overlapping windows (rows * T, h, w, C), window t = iy * nx + ix at (ys[iy], xs[ix]),
// columns taken mod W when `wrap_w`.
//
// gather: windows[r T + t][py][px] = canvas[r][ys[iy] + py][(xs[ix] + px) mod W], a copy of 4-element vectors; one thread per window
// pixel vector, every workgroup inside one window (its starts are workgroup-uniform, scalar reads of the launch arguments).
// blend:  one thread per canvas pixel vector walks the grid in ascending t and keeps, per element, num = fma(w_t, e_t, num) and
// den += w_t over the n windows that cover its pixel; n == 1 stores the window's bits, otherwise round(num / den).  No atomics and a
// fixed order: two launches give the same bits.  The weight map is read through its pointer when the kernel runs.
//
// The window starts travel BY VALUE in the launch arguments, after the entry point has checked them against the canvas: there is no
// device table an unchecked index could come from.  All index arithmetic is 64-bit.  Memory-bound, no LDS.
#include "common.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_MAX = 16;                                       // window starts per axis

struct TileGeom {
    int ys[TL_MAX], xs[TL_MAX];
    int ny, nx, H, W, h, w, cv, wrap;                           // cv: 4-element vectors per pixel (C / 4)
};

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef f32x4 type; };
template <> struct Vec4<bf16> { typedef bf16x4 type; };
template <> struct Vec4<f16> { typedef f16x4 type; };

template <typename T>
__global__ __launch_bounds__(TL_THREADS) void tile_gather_kernel(const T* __restrict__ canvas, T* __restrict__ windows, TileGeom g,
                                                                 int blocks_per_window) {
    typedef typename Vec4<T>::type V;
    const long win = blockIdx.x / blocks_per_window;            // r T + t, workgroup-uniform
    const int T_ = g.ny * g.nx;
    const long r = win / T_;
    const int t = (int)(win - r * T_), iy = t / g.nx, ix = t - iy * g.nx;
    const int y0 = g.ys[iy], x0 = g.xs[ix];
    const long per_window = (long)g.h * g.w * g.cv;
    const long i = (long)(blockIdx.x - win * blocks_per_window) * TL_THREADS + threadIdx.x;
    if (i >= per_window) return;
    const int c = (int)(i % g.cv);
    const long p = i / g.cv;
    const int py = (int)(p / g.w), px = (int)(p - (long)py * g.w);
    int X = x0 + px;
    if (X >= g.W) X -= g.W;                                      // only with wrap: the entry point keeps x0 + w <= W otherwise
    const long src = (((r * g.H + (y0 + py)) * g.W + X) * g.cv + c) * 4;
    const long dst = (win * per_window + i) * 4;
    *reinterpret_cast<V*>(windows + dst) = *reinterpret_cast<const V*>(canvas + src);
}

template <typename T>
__global__ __launch_bounds__(TL_THREADS) void tile_blend_kernel(const T* __restrict__ windows, T* __restrict__ canvas,
                                                                const float* __restrict__ weights, TileGeom g, long total) {
    typedef typename Vec4<T>::type V;
    const long i = (long)blockIdx.x * TL_THREADS + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % g.cv);
    long p = i / g.cv;
    const int X = (int)(p % g.W);
    p /= g.W;
    const int Y = (int)(p % g.H);
    const long r = p / g.H;
    const int T_ = g.ny * g.nx;
    const long per_window = (long)g.h * g.w * g.cv;
    V first = {};
    float num[4] = {0.f, 0.f, 0.f, 0.f}, den = 0.f;
    int n = 0;
    for (int iy = 0; iy < g.ny; ++iy) {                         // ascending t = iy nx + ix
        const int py = Y - g.ys[iy];
        if (py < 0 || py >= g.h) continue;
        for (int ix = 0; ix < g.nx; ++ix) {
            int px = X - g.xs[ix];
            if (px < 0 && g.wrap) px += g.W;
            if (px < 0 || px >= g.w) continue;
            const long cell = (long)py * g.w + px;
            const V e = *reinterpret_cast<const V*>(windows + ((r * T_ + (iy * g.nx + ix)) * per_window + cell * g.cv + c) * 4);
            const float wt = weights[cell];
            if (n == 0) first = e;
#pragma unroll
            for (int k = 0; k < 4; ++k) num[k] = fmaf(wt, (float)e[k], num[k]);
            den += wt;
            ++n;
        }
    }
    V out = first;                                               // n == 1: the window's bits (the entry point saw every pixel covered: n >= 1)
    if (n > 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = (T)(num[k] / den);
    }
    *reinterpret_cast<V*>(canvas + i * 4) = out;
}

// every cell of an axis of L cells lies in some [s, s + len) (mod L when wrap): the uncovered set, if any, begins at cell 0 or right
// behind a window, so those are the cells to look at
bool axis_covered(const int* s, int n, int len, int L, bool wrap) {
    auto inside = [&](long p) {
        for (int i = 0; i < n; ++i) {
            long d = p - s[i];
            if (wrap && d < 0) d += L;
            if (d >= 0 && d < len) return true;
        }
        return false;
    };
    if (!wrap && !inside(0)) return false;
    for (int i = 0; i < n; ++i) {
        long e = (long)s[i] + len;
        if (wrap) e %= L; else if (e >= L) continue;
        if (!inside(e)) return false;
    }
    return true;
}

int tile_check(const char* who, const void* canvas, const void* windows, int rows, int H, int W, int h, int w, int C, const int* ys,
               int ny, const int* xs, int nx, int wrap_w, int dtype, TileGeom* g, long* canvas_vecs, long* window_vecs) {
    ST_REQUIRE(canvas && windows && ys && xs, "%s: null pointer", who);
    ST_REQUIRE(st_dtype_ok(dtype), "%s: unsupported dtype %d", who, dtype);
    ST_REQUIRE(rows > 0 && H > 0 && W > 0 && h > 0 && w > 0 && C > 0, "%s: bad shape rows=%d canvas %dx%d window %dx%d C=%d", who, rows, H, W,
               h, w, C);
    ST_REQUIRE(C % 4 == 0, "%s: channel count %d must be a multiple of 4 (one 4-element vector per access)", who, C);
    ST_REQUIRE(h <= H && w <= W, "%s: window %dx%d larger than the canvas %dx%d", who, h, w, H, W);
    ST_REQUIRE(ny >= 1 && ny <= TL_MAX && nx >= 1 && nx <= TL_MAX, "%s: %d x %d window starts; 1 to %d per axis", who, ny, nx, TL_MAX);
    for (int i = 0; i < ny; ++i)
        ST_REQUIRE(ys[i] >= 0 && ys[i] <= H - h, "%s: window row start ys[%d]=%d outside the canvas (0 <= y <= %d)", who, i, ys[i], H - h);
    for (int i = 0; i < nx; ++i) {
        if (wrap_w) ST_REQUIRE(xs[i] >= 0 && xs[i] < W, "%s: window column start xs[%d]=%d outside the canvas (wrap: 0 <= x < %d)", who, i, xs[i], W);
        else ST_REQUIRE(xs[i] >= 0 && xs[i] <= W - w, "%s: window column start xs[%d]=%d outside the canvas (0 <= x <= %d)", who, i, xs[i], W - w);
    }
    ST_REQUIRE(axis_covered(ys, ny, h, H, false), "%s: canvas rows not covered by the windows", who);
    ST_REQUIRE(axis_covered(xs, nx, w, W, wrap_w != 0), "%s: canvas columns not covered by the windows", who);
    const long esz = dtype == ST_F32 ? 4 : 2, T_ = (long)ny * nx;
    const long limit = 0x7fffffffffffL / (esz * C);               // elements stay far inside 63 bits
    ST_REQUIRE((long)rows * H <= limit / W && (long)rows * T_ <= limit / w / h, "%s: tensor too large", who);
    const uintptr_t c0 = (uintptr_t)canvas, c1 = c0 + (uintptr_t)((long)rows * H * W * C * esz);
    const uintptr_t w0 = (uintptr_t)windows, w1 = w0 + (uintptr_t)((long)rows * T_ * h * w * C * esz);
    ST_REQUIRE(((c0 | w0) & (uintptr_t)(4 * esz - 1)) == 0, "%s: misaligned pointer (%ld-byte vectors)", who, 4 * esz);
    ST_REQUIRE(c1 <= w0 || w1 <= c0, "%s: canvas and windows must not alias or overlap", who);
    for (int i = 0; i < TL_MAX; ++i) { g->ys[i] = i < ny ? ys[i] : 0; g->xs[i] = i < nx ? xs[i] : 0; }
    g->ny = ny; g->nx = nx; g->H = H; g->W = W; g->h = h; g->w = w; g->cv = C / 4; g->wrap = wrap_w != 0;
    *canvas_vecs = (long)rows * H * W * (C / 4);
    *window_vecs = (long)h * w * (C / 4);
    return 0;
}

}  // namespace

extern "C" int st_tile_gather(const void* canvas, void* windows, int rows, int H, int W, int h, int w, int C, const int* ys, int ny,
                              const int* xs, int nx, int wrap_w, int dtype, void* stream) {
    TileGeom g;
    long canvas_vecs, window_vecs;
    if (int rc = tile_check("tile_gather", canvas, windows, rows, H, W, h, w, C, ys, ny, xs, nx, wrap_w, dtype, &g, &canvas_vecs, &window_vecs))
        return rc;
    const long bpw = (window_vecs + TL_THREADS - 1) / TL_THREADS, blocks = bpw * rows * ny * nx;
    ST_REQUIRE(blocks <= 0x7fffffffL, "tile_gather: too many workgroups");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(TL_THREADS);
    if (dtype == ST_BF16) hipLaunchKernelGGL(tile_gather_kernel<bf16>, grid, block, 0, st, (const bf16*)canvas, (bf16*)windows, g, (int)bpw);
    else if (dtype == ST_F16) hipLaunchKernelGGL(tile_gather_kernel<f16>, grid, block, 0, st, (const f16*)canvas, (f16*)windows, g, (int)bpw);
    else hipLaunchKernelGGL(tile_gather_kernel<float>, grid, block, 0, st, (const float*)canvas, (float*)windows, g, (int)bpw);
    return st_check_launch("tile_gather");
}

extern "C" int st_tile_blend(const void* windows, void* canvas, const float* weights, int rows, int H, int W, int h, int w, int C,
                             const int* ys, int ny, const int* xs, int nx, int wrap_w, int dtype, void* stream) {
    TileGeom g;
    long canvas_vecs, window_vecs;
    if (int rc = tile_check("tile_blend", canvas, windows, rows, H, W, h, w, C, ys, ny, xs, nx, wrap_w, dtype, &g, &canvas_vecs, &window_vecs))
        return rc;
    ST_REQUIRE(weights != nullptr && ((uintptr_t)weights & 3) == 0, "tile_blend: null or misaligned weight map");
    {
        const uintptr_t esz = dtype == ST_F32 ? 4 : 2;
        const uintptr_t c0 = (uintptr_t)canvas, c1 = c0 + (uintptr_t)canvas_vecs * 4 * esz;
        const uintptr_t m0 = (uintptr_t)weights, m1 = m0 + (uintptr_t)h * (uintptr_t)w * 4;
        ST_REQUIRE(c1 <= m0 || m1 <= c0, "tile_blend: the weight map must not overlap the canvas");
    }
    const long blocks = (canvas_vecs + TL_THREADS - 1) / TL_THREADS;
    ST_REQUIRE(blocks <= 0x7fffffffL, "tile_blend: too many workgroups");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks), block(TL_THREADS);
    if (dtype == ST_BF16) hipLaunchKernelGGL(tile_blend_kernel<bf16>, grid, block, 0, st, (const bf16*)windows, (bf16*)canvas, weights, g, canvas_vecs);
    else if (dtype == ST_F16) hipLaunchKernelGGL(tile_blend_kernel<f16>, grid, block, 0, st, (const f16*)windows, (f16*)canvas, weights, g, canvas_vecs);
    else hipLaunchKernelGGL(tile_blend_kernel<float>, grid, block, 0, st, (const float*)windows, (float*)canvas, weights, g, canvas_vecs);
    return st_check_launch("tile_blend");
}
