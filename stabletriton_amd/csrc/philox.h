// Counter-based Gaussian noise of the stochastic samplers: Philox4x32-10 (Salmon et al. 2011) and a 4-wide Box-Muller.
// Every value is a pure function of (seed, counter word, element): nothing is stored or advanced between launches, so a
// captured graph replays the same noise.  stabletriton_amd/rng.py restates the stream in float64 and states it in full:
//   key = (seed lo, seed hi), counter = (j >> 2, C, 0, 0) -> u0..u3;  p = ((u >> 9) + 0.5) 2^-23 (exact in fp32, in (0, 1))
//   z[4q] = r0 cos(2 pi p1), z[4q+1] = r0 sin(2 pi p1), r0 = sqrt(-2 ln p0); z[4q+2], z[4q+3] from p2, p3 the same way.
// Plain integer ops and the accurate logf / sqrtf / sincospif (the library builds without fast-math).
#pragma once
#include "common.h"

struct PhiloxKey { unsigned k0, k1; };

__device__ __forceinline__ PhiloxKey philox_key(unsigned long long seed) {
    return {(unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)};
}

// Philox4x32-10 of counter (c0, c1, 0, 0) under key
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, PhiloxKey key, unsigned (&u)[4]) {
    unsigned x0 = c0, x1 = c1, x2 = 0u, x3 = 0u, k0 = key.k0, k1 = key.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned hi0 = __umulhi(0xD2511F53u, x0), lo0 = 0xD2511F53u * x0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, x2), lo1 = 0xCD9E8D57u * x2;
        x0 = hi1 ^ x1 ^ k0; x1 = lo1; x2 = hi0 ^ x3 ^ k1; x3 = lo0;
    }
    u[0] = x0; u[1] = x1; u[2] = x2; u[3] = x3;
}

__device__ __forceinline__ float philox_uniform(unsigned u) {
    return ((float)(u >> 9) + 0.5f) * 0x1p-23f;              // (u >> 9) < 2^23: the sum and the product are exact
}

// the 4 normals of elements 4q .. 4q + 3 at counter word `ctr`
__device__ __forceinline__ void philox_normal4(PhiloxKey key, unsigned q, unsigned ctr, float* z) {
    unsigned u[4];
    philox4x32_10(q, ctr, key, u);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float r = sqrtf(-2.f * logf(philox_uniform(u[2 * h])));
        float s, c;
        sincospif(2.f * philox_uniform(u[2 * h + 1]), &s, &c);
        z[2 * h] = r * c;
        z[2 * h + 1] = r * s;
    }
}
