"""The counter-based noise generator of the stochastic samplers, restated on the host (numpy only).

The device draws its Gaussian noise with Philox4x32-10 (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3";
csrc/philox.h): every value is a pure function of (seed, counter word, element), so nothing is stored or advanced between
steps and a captured graph replays the same noise every time.  This module computes the same stream in float64, for tests
and for reproducing a loop's noise on the CPU.

The stream, for sample seed S (64 bits), counter word C (32 bits) and element offset j, taken in memory order within the
sample's dense block (for DenoiseLoop's channels_last latent, j = (h W + w) 4 + c):
    key = (S & 0xffffffff, S >> 32),  counter = (j >> 2, C, 0, 0)  ->  u0 .. u3 = philox4x32_10(counter, key)
    p_k = ((u_k >> 9) + 0.5) 2^-23                    23 bits: strictly inside (0, 1), and exact in fp32
    z[4q]     = r0 cos(2 pi p1),  z[4q + 1] = r0 sin(2 pi p1),  r0 = sqrt(-2 ln p0)       (q = j >> 2, Box-Muller)
    z[4q + 2] = r2 cos(2 pi p3),  z[4q + 3] = r2 sin(2 pi p3),  r2 = sqrt(-2 ln p2)
DenoiseLoop uses C = 0 for the initial (or img2img) noise and C = i + 1 for the noise step i adds, i the absolute schedule
index.  The stream is this project's own: it does not reproduce torch's or diffusers' noise for a given seed.
"""
from __future__ import annotations

import numpy as np

_M0, _M1 = 0xD2511F53, 0xCD9E8D57           # round multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85           # Weyl key increments
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: (..., 4) and key: (..., 2) of 32-bit words (any integer dtype, broadcast); returns (..., 4)
    uint64 holding 32-bit words.  The arithmetic runs in uint64 lanes: a 32 x 32-bit product fits exactly."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(_MASK)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(_MASK)
    c0, c1, c2, c3 = (c[..., q] for q in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    m0, m1, mask = np.uint64(_M0), np.uint64(_M1), np.uint64(_MASK)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(_W0)) & mask
            k1 = (k1 + np.uint64(_W1)) & mask
        p0, p1 = m0 * c0, m1 * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & mask
        hi1, lo1 = p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def uniform_open(u) -> np.ndarray:
    """The 23-bit uniform of each word: ((u >> 9) + 0.5) 2^-23, float64 (and exactly representable in fp32)."""
    return ((np.asarray(u, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normal(seeds, counter: int, per_sample: int) -> np.ndarray:
    """float64 (B, per_sample): the stream of each seed at counter word `counter`, in memory order (module docstring).
    per_sample must be a multiple of 4 (every Philox call gives 4 values)."""
    if per_sample <= 0 or per_sample % 4:
        raise ValueError(f"normal: per_sample {per_sample} must be a positive multiple of 4")
    if not 0 <= int(counter) <= _MASK:
        raise ValueError(f"normal: counter {counter} is not a 32-bit word")
    s = [int(seeds)] if np.ndim(seeds) == 0 and not isinstance(seeds, (list, tuple)) else [int(v) for v in seeds]
    if any(v < 0 or v >= 1 << 64 for v in s):
        raise ValueError("normal: seeds are 64-bit unsigned integers")
    key = np.array([[v & _MASK, v >> 32] for v in s], dtype=np.uint64)              # (B, 2)
    q = np.arange(per_sample // 4, dtype=np.uint64)
    ctr = np.zeros((len(q), 4), dtype=np.uint64)
    ctr[:, 0] = q
    ctr[:, 1] = int(counter)
    u = philox4x32_10(ctr[None, :, :], key[:, None, :])                             # (B, Q, 4)
    p = uniform_open(u)
    r0, r2 = np.sqrt(-2.0 * np.log(p[..., 0])), np.sqrt(-2.0 * np.log(p[..., 2]))
    t1, t3 = 2.0 * np.pi * p[..., 1], 2.0 * np.pi * p[..., 3]
    z = np.stack([r0 * np.cos(t1), r0 * np.sin(t1), r2 * np.cos(t3), r2 * np.sin(t3)], axis=-1)
    return z.reshape(len(s), per_sample)
