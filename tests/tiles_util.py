"""The tiled-denoising tests' own statement of the method (checker only; shares no code with stabletriton_amd/tiles.py), in float64.

`cut64` / `blend64` restate the two moves between a canvas and its windows window by window; `blend64` also returns what the
kernel's error bound is made of (the coverage count n and sum(w |e|) / sum(w)).  `loop64` is a float64 tiled denoise loop around the
eager float64 CPU module, built on pag_util's sampler rows and guidance and on the PAG / SEG hooks of the other test utilities;
`blend="last"` is the wrong blend the loop tests must be able to tell from the right one (the last window covering a pixel wins).
"""
import contextlib

import torch

from tests import pag_util as PU
from tests import seg_util as SU

# one rounding to the type (unit roundoff) and the fp32 accumulator's
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
U_ACC = 2.0 ** -24


def starts(L, win, stride, wrap=False):
    if wrap:
        return list(range(0, L, stride))
    s = list(range(0, L - win + 1, stride))
    return s if s[-1] == L - win else s + [L - win]


def windows_of(ys, xs):
    return [(y, x) for y in ys for x in xs]                   # t = iy * len(xs) + ix


def _cols(x0, w, W):
    return torch.tensor([(x0 + j) % W for j in range(w)])


def cut64(canvas, ys, xs, hw):
    """(rows, C, H, W) -> (rows * T, C, h, w) float64, row r * T + t."""
    h, w = hw
    W = canvas.shape[-1]
    c = canvas.double()
    out = [c[r:r + 1, :, y0:y0 + h][:, :, :, _cols(x0, w, W)] for r in range(c.shape[0]) for (y0, x0) in windows_of(ys, xs)]
    return torch.cat(out)


def blend64(windows, ys, xs, canvas_hw, weights, mode="mean"):
    """(rows * T, C, h, w) -> (canvas float64, n (H, W), sum(w |e|) / sum(w) float64).  mode "last": the last window wins."""
    H, W = canvas_hw
    wins = windows_of(ys, xs)
    T = len(wins)
    e = windows.double()
    rows, C, h, w = e.shape[0] // T, e.shape[1], e.shape[2], e.shape[3]
    wt = weights.double()
    num, mag = torch.zeros(rows, C, H, W, dtype=torch.float64), torch.zeros(rows, C, H, W, dtype=torch.float64)
    last = torch.zeros(rows, C, H, W, dtype=torch.float64)
    den, n = torch.zeros(H, W, dtype=torch.float64), torch.zeros(H, W, dtype=torch.int64)
    for r in range(rows):
        for t, (y0, x0) in enumerate(wins):
            for py in range(h):
                for px in range(w):
                    Y, X = y0 + py, (x0 + px) % W
                    v = e[r * T + t, :, py, px]
                    num[r, :, Y, X] += wt[py, px] * v
                    mag[r, :, Y, X] += wt[py, px] * v.abs()
                    last[r, :, Y, X] = v
                    if r == 0:
                        den[Y, X] += wt[py, px]
                        n[Y, X] += 1
    assert int(n.min()) >= 1, "the windows do not cover the canvas"
    return (last if mode == "last" else num / den), n, mag / den


def blend_fast64(windows, ys, xs, canvas_hw, weights, mode="mean"):
    """blend64's canvas alone, window by window (the loop's inner call: no per-pixel Python)."""
    H, W = canvas_hw
    wins = windows_of(ys, xs)
    T = len(wins)
    e = windows.double()
    rows, C, h, w = e.shape[0] // T, e.shape[1], e.shape[2], e.shape[3]
    ev = e.view(rows, T, C, h, w)
    wt = weights.double()
    num, den = torch.zeros(rows, C, H, W, dtype=torch.float64), torch.zeros(H, W, dtype=torch.float64)
    for t, (y0, x0) in enumerate(wins):
        cols = _cols(x0, w, W)
        if mode == "last":
            num[:, :, y0:y0 + h, cols] = ev[:, t]
        else:
            num[:, :, y0:y0 + h, cols] += wt * ev[:, t]
            den[y0:y0 + h, cols] += wt
    return num if mode == "last" else num / den


def blend_bound(ref, n, mag, dtype):
    """|out - ref| <= one rounding to the type at |ref| + (2 n + 4) 2^-24 sum(w |e|) / sum(w): the n-term fma chain, the (n - 1)-term
    denominator and a division good to 2 ulp."""
    return U_OUT[dtype] * ref.abs() + (2.0 * n.double() + 4.0) * U_ACC * mag


def gaussian64(h, w, sigma=0.1):
    ax = lambda m: torch.exp(-(torch.arange(m, dtype=torch.float64) - (m - 1) / 2) ** 2 / (2 * (sigma * m) ** 2))
    return ax(h)[:, None] * ax(w)[None, :]


def canvas_noise(hw, batch=1, seed=99):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((batch, 4, hw[0], hw[1]), generator=g)


def loop64(unet64, x, noise, tables, ys, xs, tile_hw, weights, g=None, phi=None, s=None, layers=("mid",), seg_sigma=None,
           wrap=False, mode="mean", pos=slice(1, 2), neg=slice(0, 1), seed=None):
    """float64 tiled loop: canvas `noise` (B, 4, H, W), conditioning rows x[k][pos] / x[k][neg] (B rows, or B * T rows: one prompt per
    window); blocks [neg | pos | pert] as the guidance asks; every block's window predictions are blended to the canvas, then
    pag_util's guidance (rescale statistics over the canvas) and sampler rows.  `s` with seg_sigma=None is PAG, with a sigma SEG."""
    del wrap                                                   # (the starts say it all: columns are taken mod W)
    n_steps = tables.n_steps
    B = noise.shape[0]
    H, W = noise.shape[-2:]
    T = len(ys) * len(xs)
    lat = noise.double() * tables.init_noise_sigma
    rows, in_scale = PU.rows64(tables), tables.in_scale()
    dsigma = tables.dsigma() if rows is None else None
    blocks = ([neg] if g is not None else []) + [pos] + ([pos] if s is not None else [])

    def per_window(t):
        t = t.double()
        if t.shape[0] == B * T:
            return t
        assert t.shape[0] == B
        return torch.cat([t[b:b + 1] for b in range(B) for _ in range(T)])

    ehs, te, ti = (torch.cat([per_window(x[k][r]) for r in blocks]) for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    chunks = len(blocks) if s is not None else 0

    def hooks():
        if not chunks:
            return contextlib.nullcontext()
        if seg_sigma is not None:
            return SU.hooked(unet64, layers, chunks, tuple(tile_hw), seg_sigma)
        return PU.hooked(unet64, layers, chunks)

    prev = None
    for i in range(n_steps):
        t = torch.tensor(float(tables.timesteps[i]), dtype=torch.float64)
        xin = cut64(lat * float(in_scale[i]), ys, xs, tile_hw)
        with torch.no_grad(), hooks():
            e_all = unet64(torch.cat([xin] * len(blocks)), t, ehs, {"text_embeds": te, "time_ids": ti})[0].double()
        parts = [blend_fast64(p, ys, xs, (H, W), weights, mode) for p in e_all.split(B * T)]
        e_neg = parts.pop(0) if g is not None else None
        e_pos = parts.pop(0)
        if s is None:
            e = e_pos if g is None else PU.guide64(e_neg, e_pos, e_pos, g, 0.0, phi)
        else:
            e = PU.guide64(e_neg, e_pos, parts.pop(0), g, float(s), phi)
        if rows is None:
            lat = lat + e * float(dsigma[i])
        else:
            sigma, a, bb, k, c = rows[i]
            d = lat - sigma * e
            new = a * lat + bb * d if (i == 0 or k == 0.0) else a * lat + bb * ((1.0 + k) * d - k * prev)
            if c != 0.0:
                new = new + c * PU.unit64(seed, i + 1, tuple(lat.shape))
            lat, prev = new, d
    return lat
