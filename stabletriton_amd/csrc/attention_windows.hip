// Windowed self-attention for gfx950 (include/stabletriton_amd.h, st_attention_windows): HyperTile.  The T = gh * gw tokens of a
// self-attention site are a row-major gh x gw grid; a tiling (nh, nw) cuts it into nh * nw rectangular windows of th x tw tokens
// (th = gh / nh, tw = gw / nw, Tw = th * tw) and every window attends to itself alone.  One launch, q / k / v / out where they lie:
// no window-major copies.
//
// attnw32i_kernel runs attn32i_core (attention_core.h), the body of attn32i_kernel and attnj32i_kernel, on ONE WINDOW as if it were
// a batch entry of Tw queries and Tw keys, with two rules of its own:
//   rows   (AttRowsWin)  row i of a window is token (i / tw) * gw + i % tw from the window's first token: one divide per lane for
//                        the Q loads and one for the stores, both outside the key loop;
//   keys   (AttKeysWin)  a ring piece is 8 key rows (row lr of group p & 7).  With tw % 8 == 0 an 8-key group never leaves its grid
//                        row, so the base of group G = 8 kt + (p & 7) is wave-uniform: window row G / (tw / 8), column
//                        8 (G % (tw / 8)).  A wave keeps TWO scalar counters - the column group and the token of its first group in
//                        the next tile - stepped group by group and tile by tile without a divide (one divide at the seed); a lane
//                        adds its constant lr * ld + swizzled chunk.  K piece p and V piece p + 8 share the token.  Groups >= Tw / 8
//                        read the zero line (Tw % 8 == 0: a group is whole or absent); mask_tail stays the core's.
// Ring, counted waits, lazy maximum, MFMA order: shared code, so a window's rows carry the bits st_attention gives on the gathered
// window, and tiling (1, 1) the bits of st_attention.
//
// The grid does not depend on the tiling: with R query rows per block (256: eight self-loading waves, 128 / 96: four / three waves and
// a loader) and R | Tw for every tiling the site may use, every tiling has T / R blocks per (batch entry, head); block x serves
// window x / (Tw / R), local block x % (Tw / R).  att_xcd_decode is used as it is, on T; no block idles or exits early.  The tiling
// is a device row (n pairs, read at clamp(*step)): one scalar load per block of values no launch writes, so a captured launch follows
// in-place writes.  The entry point cannot see device values: the host wrapper (ops.attention_windows, hypertile.py) validates every
// pair it writes (nh | gh, nw | gw, tw % 8 == 0, R | Tw), the kernel trusts the row.
#include "attention_core.h"

template <typename E>
struct WinArgs {
    const E *Q, *K, *V;
    E* O;
    int T, gh, gw, H;
    int ldq, ldk, ldv, ldo;                            // token strides (the entry point checks that they fit)
    float scale_log2e;
    const int* tilings;                                // n pairs (nh, nw), or NULL: the host pair below
    const int* step;
    int n, nh, nw;
};

struct AttRowsWin {                                    // window row -> token, from the window's first token
    int tw, gw;
    __device__ __forceinline__ int operator()(int r) const {
        const int y = (unsigned)r / (unsigned)tw;
        return y * gw + (r - y * tw);
    }
};

// The windowed key rule of attn32i_core (attention_core.h: the KEYS contract).  load_tile issues sixteen DMAs and load_piece one on
// every path, and nothing else touches vector memory.
template <typename E, int NW, bool LD>
struct AttKeysWin {
    static constexpr int N = LD ? 16 : 16 / NW;
    static_assert(LD || (N <= 8 && 8 % N == 0), "a self-loading wave's pieces are all K or all V");
    const E *Kb, *Vb;                                  // the window's first token of this (batch entry, head)
    int ldk, ldv;
    int S;                                             // Tw
    int gpr;                                           // 8-key groups per window row, tw / 8
    int wrap_tok;                                      // token step from the end of a window row to the start of the next, gw - tw
    int tile_tok, tile_grp;                            // self-loading waves: token / column-group step of eight groups, before the wrap
    int wc, tok;                                       // THE TWO COUNTERS (wave-uniform): column group and token of the wave's first group of the next tile
    long off[N];                                       // lane constant per piece: lr * ld + swizzled chunk (elements)
    __device__ __forceinline__ void seed(int first, int lr, int pc) {
        const int g0 = first & 7;
        const int wr = g0 / gpr;                       // the one divide of the key rule
        wc = g0 - wr * gpr;
        tok = wr * (wrap_tok + 8 * gpr) + 8 * wc;
        const int q8 = 8 / gpr;
        tile_grp = 8 - q8 * gpr;
        tile_tok = q8 * (wrap_tok + 8 * gpr) + 8 * tile_grp;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int pce = first + i;
            const int isv = pce >> 3, row = (pce & 7) * 8 + lr;
            const int c = pc ^ (isv ? swz_v(row) : swz_k(row));
            off[i] = (long)lr * (isv ? ldv : ldk) + c * 8;
        }
    }
    __device__ __forceinline__ void load_tile(int kt, unsigned slot) {
        const E* zeros = reinterpret_cast<const E*>(g_att_zero16);
        const int ng = S >> 3;
        int c = wc, t = tok;
#pragma unroll
        for (int j = 0; j < 8; ++j) {                  // group 8 kt + j: K piece j and V piece j + 8 read the same token
            const bool in = 8 * kt + j < ng;           // wave-uniform
            att_dma16(in ? Kb + (long)t * ldk + off[j] : zeros, slot + att32_piece_off(j));
            att_dma16(in ? Vb + (long)t * ldv + off[j + 8] : zeros, slot + att32_piece_off(j + 8));
            ++c; t += 8;
            if (c == gpr) { c = 0; t += wrap_tok; }
        }
        wc = c; tok = t;                               // eight groups on: the first group of the next tile
    }
    __device__ __forceinline__ void load_piece(int kt, int i, int pce, unsigned slot, unsigned dump, bool live) {
        const E* zeros = reinterpret_cast<const E*>(g_att_zero16);
        int c = wc, t = tok;
#pragma unroll
        for (int s = 0; s < i; ++s) {                  // piece i is i groups behind the wave's first
            ++c; t += 8;
            if (c == gpr) { c = 0; t += wrap_tok; }
        }
        const int isv = pce >> 3;
        const bool in = live && 8 * kt + (pce & 7) < (S >> 3);      // wave-uniform
        const E* sp = isv ? Vb + (long)t * ldv + off[i] : Kb + (long)t * ldk + off[i];
        const unsigned dst = __builtin_amdgcn_readfirstlane(live ? slot + att32_piece_off(pce) : dump);
        att_dma16(in ? sp : zeros, dst);
        if (i == N - 1) {                              // the wave's last piece of this tile: eight groups on
            wc += tile_grp; tok += tile_tok;
            if (wc >= gpr) { wc -= gpr; tok += wrap_tok; }
        }
    }
};

template <typename E, int NW, bool LD>
__global__ __launch_bounds__((NW + (LD ? 1 : 0)) * 64) void attnw32i_kernel(const WinArgs<E> a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];      // the ring, then a 1-KiB dump for the dummy DMAs
    int head, b, xblk;
    att_xcd_decode<true>(a.T, 32 * NW, a.H, b, head, xblk);

    // the tiling: scalar loads of values no launch writes, clamped like st_attention_joint's gate
    int nh = a.nh, nw = a.nw;
    if (a.tilings) {
        int i = *a.step;
        i = i < 0 ? 0 : (i >= a.n ? a.n - 1 : i);
        nh = a.tilings[2 * i];
        nw = a.tilings[2 * i + 1];
    }
    nh = __builtin_amdgcn_readfirstlane(nh);
    nw = __builtin_amdgcn_readfirstlane(nw);
    const int gw = a.gw;
    const int th = a.gh / nh, tw = gw / nw, Tw = th * tw;
    const int bpw = Tw / (32 * NW);                    // blocks per window (the host: 32 NW | Tw)
    const int win = xblk / bpw, lblk = xblk - win * bpw;
    const int wy = win / nw, wx = win - wy * nw;
    const size_t origin = (size_t)b * a.T + (size_t)(wy * th) * gw + (size_t)wx * tw;      // the window's first token, in tokens of the whole tensor

    AttKeysWin<E, NW, LD> keys;
    keys.ldk = a.ldk; keys.ldv = a.ldv;
    keys.S = Tw;
    keys.gpr = tw >> 3;
    keys.wrap_tok = gw - tw;
    keys.Kb = a.K + origin * a.ldk + (size_t)head * ATT_D;
    keys.Vb = a.V + origin * a.ldv + (size_t)head * ATT_D;
    const long ldq = a.ldq, ldo = a.ldo;
    attn32i_core<E, NW, LD>(a.Q + origin * ldq + (size_t)head * ATT_D, ldq, Tw, lblk,
                            a.O + origin * ldo + (size_t)head * ATT_D, ldo, a.scale_log2e, lds, keys, AttRowsWin{tw, gw});
}

// Query rows per block among the forms that fit (bit 0: 256 | Tw of every tiling the site may use, bit 1: 128, bit 2: 96), by the
// reasoning of att32_form on (T, H, B) - the grid is T / R blocks per (batch entry, head) whatever the tiling:
//   256 rows (eight self-loading waves) once 256-row blocks fill the CUs (more than 128 of them);
//   else 96 rows (three waves + loader) when 128-row blocks would leave a third of the CUs without one (<= 176 blocks, and <= 256 of 96 rows);
//   else 128 rows (four waves + loader).
// Where the wanted form does not fit: the largest fitting one below it (more blocks, never fewer CUs), else the smallest above.
static inline int att_win_rows(int T, int H, int B, int fits) {
    const long hb = (long)H * B;
    int want = cdiv(T, 256) * hb > 128 ? 256 : (cdiv(T, 128) * hb <= 176 && cdiv(T, 96) * hb <= 256) ? 96 : 128;
    static const int forms[3] = {256, 128, 96};
    int below = 0, above = 0;
    for (int i = 0; i < 3; ++i) {
        if (!(fits >> i & 1)) continue;
        if (forms[i] == want) return want;
        if (forms[i] < want) below = below ? below : forms[i];
        else above = forms[i];
    }
    return below ? below : above;
}

extern "C" int st_attention_windows_rows(int T, int H, int B, int row_forms) {      // host arithmetic only: 0 = no form in the mask
    return (T > 0 && H > 0 && B > 0 && row_forms > 0 && row_forms < 8) ? att_win_rows(T, H, B, row_forms) : 0;
}

template <typename E>
static int attention_windows_launch(const WinArgs<E>& a, int B, int rows, hipStream_t st) {
    auto kfn = rows == 256 ? attnw32i_kernel<E, 8, false> : rows == 128 ? attnw32i_kernel<E, 4, true> : attnw32i_kernel<E, 3, true>;
    static unsigned long long lds_ok[3] = {0, 0, 0};          // per kernel: bit mask over device ordinals
    ensure_dynamic_lds(kfn, ATT32_RING, &lds_ok[rows == 256 ? 0 : rows == 128 ? 1 : 2]);
    const long grid = (long)(a.T / rows) * a.H * B;
    ST_REQUIRE(grid < (1L << 31), "attention_windows: too many blocks");
    hipLaunchKernelGGL(kfn, dim3((unsigned)grid), dim3(rows == 256 ? 512 : rows == 128 ? 320 : 256), ATT32_RING, st, a);
    return st_check_launch("attention_windows");
}

extern "C" int st_attention_windows(const void* q, const void* k, const void* v, void* out, int B, int gh, int gw, int H, int D,
                                    long ldq, long ldk, long ldv, long ldo, float scale, int nh, int nw,
                                    const int* tilings, const int* step, int n, int row_forms, int dtype, void* stream) {
    ST_REQUIRE(q && k && v && out, "attention_windows: null pointer");
    ST_REQUIRE(B > 0 && gh > 0 && gw > 0 && H > 0 && (long)gh * gw <= (1L << 30), "attention_windows: bad shape B=%d grid=%dx%d H=%d", B, gh, gw, H);
    ST_REQUIRE(dtype == ST_BF16 || dtype == ST_F16, "attention_windows: 16-bit types only (dtype %d); other types take the host's slow path", dtype);
    ST_REQUIRE(D == ATT_D, "attention_windows: head_dim %d not supported (only %d)", D, ATT_D);
    ST_REQUIRE(H <= 65535 && B <= 65535, "attention_windows: too many heads/batches for one launch");
    ST_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 4 == 0, "attention_windows: strides must keep 16-byte alignment");
    ST_REQUIRE((ldq | ldk | ldv | ldo) >= 0 && (ldq | ldk | ldv | ldo) < (1L << 31), "attention_windows: token strides must fit 31 bits");
    ST_REQUIRE(ldq >= (long)H * D && ldk >= (long)H * D && ldv >= (long)H * D && ldo >= (long)H * D, "attention_windows: token strides must hold a row of H*D values");
    ST_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16 == 0, "attention_windows: pointers must be 16-byte aligned");
    ST_REQUIRE((tilings == nullptr) == (step == nullptr), "attention_windows: the tiling is a table AND a step, or neither");
    ST_REQUIRE(!tilings || n > 0, "attention_windows: tiling table of %d rows", n);
    ST_REQUIRE((((uintptr_t)tilings | (uintptr_t)step) & 3) == 0, "attention_windows: misaligned table pointer");
    ST_REQUIRE(row_forms > 0 && row_forms < 8, "attention_windows: row_forms %d is no mask over (256, 128, 96)", row_forms);
    const int T = gh * gw;
    const int rows = att_win_rows(T, H, B, row_forms);
    ST_REQUIRE(T % rows == 0, "attention_windows: %d query rows per block do not divide the %d tokens", rows, T);
    if (!tilings) {
        ST_REQUIRE(nh >= 1 && nw >= 1 && gh % nh == 0 && gw % nw == 0, "attention_windows: tiling (%d, %d) does not divide the %d x %d grid", nh, nw, gh, gw);
        ST_REQUIRE((gw / nw) % 8 == 0, "attention_windows: window width %d is no multiple of 8 (the host's slow path takes it)", gw / nw);
        ST_REQUIRE(((gh / nh) * (gw / nw)) % rows == 0, "attention_windows: %d query rows per block do not divide the window's %d tokens", rows, (gh / nh) * (gw / nw));
    } else {
        nh = nw = 1;
    }
    void* out_split = nullptr;
    if (int e = st_take_split_arm("attention_windows", (long)B * T, H * D, false, &out_split)) return e;
    hipStream_t st = (hipStream_t)stream;
    const float c = scale * 1.4426950408889634f;
    if (dtype == ST_BF16) {
        const WinArgs<bf16> a{(const bf16*)q, (const bf16*)k, (const bf16*)v, (bf16*)out, T, gh, gw, H, (int)ldq, (int)ldk, (int)ldv, (int)ldo, c,
                              tilings, step, n, nh, nw};
        return attention_windows_launch<bf16>(a, B, rows, st);
    }
    const WinArgs<f16> a{(const f16*)q, (const f16*)k, (const f16*)v, (f16*)out, T, gh, gw, H, (int)ldq, (int)ldk, (int)ldv, (int)ldo, c,
                         tilings, step, n, nh, nw};
    return attention_windows_launch<f16>(a, B, rows, st);
}
