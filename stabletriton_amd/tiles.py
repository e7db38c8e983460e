"""Tiled denoising (MultiDiffusion; Mixture of Diffusers with Gaussian weights): the window grid, the blend weights, and the two
moves between a canvas and its windows.

A canvas larger than the UNet should denoise in one piece is covered by overlapping windows of the UNet's size.  Each step the UNet
predicts the noise on every window (windows are UNet batch rows), the predictions are averaged per canvas pixel under a weight map
(`blend`), the sampler updates the canvas, and the next input is cut into windows again (`gather`).  `DenoiseLoop(tile_hw=...)`
(pipeline.py) does this inside the captured loop; `gather` and `blend` are here for callers that tile outside it (a UI's tiling code
around the hooked UNet).

Window order: `t = iy * len(xs) + ix`; rows of a window batch: `r * T + t` for canvas row r.  Wrap applies to the width only: a window
that runs over the right edge continues at column 0 (360-degree panoramas).

`gaussian_weights` is Mixture of Diffusers' map as recalled (per axis exp(-(i - (n - 1) / 2)^2 / (2 (sigma n)^2)), sigma = 0.1 for the
published variance 0.01): parity with that pipeline is unpinned - no reference output has been compared.

Device tensors go to the HIP kernels (ops.tile_gather / ops.tile_blend, csrc/tiles.hip).  CPU tensors take a torch restatement with
the kernel's accumulation order (ascending t, fp32 fma chain, one division, one rounding; a pixel under one window keeps its bits).
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

MAX_STARTS = 16          # per axis: the kernels take the starts by value in their launch arguments


def tile_starts(L: int, win: int, stride: int, wrap: bool = False) -> List[int]:
    """Window starts along an axis of L cells.  Without wrap: 0, stride, ... while the window fits, plus L - win when the last of
    them does not end flush with the axis.  With wrap: 0, stride, ... below L (windows continue at cell 0)."""
    L, win, stride = int(L), int(win), int(stride)
    if win < 1 or win > L:
        raise ValueError(f"tile_starts: a window of {win} does not fit an axis of {L}")
    if stride < 1:
        raise ValueError(f"tile_starts: stride {stride} must be at least 1")
    if stride > win:
        raise ValueError(f"tile_starts: stride {stride} larger than the window {win} leaves a gap in coverage")
    if wrap:
        n = -(-L // stride)
    else:
        n = (L - win) // stride + 1 + (1 if (L - win) % stride else 0)
    if n > MAX_STARTS:                                          # (checked on the count: no list of a million starts is built first)
        raise ValueError(f"tile_starts: {n} windows on one axis; at most {MAX_STARTS}")
    if wrap:
        return list(range(0, L, stride))
    starts = list(range(0, L - win + 1, stride))
    if starts[-1] != L - win:
        starts.append(L - win)
    return starts


def _pair(v, what: str) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what}: one int or (height, width), got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


class TileGrid:
    """The windows of a canvas: `ys`, `xs`, `T = len(ys) * len(xs)`, window t = iy * len(xs) + ix.  `stride`: an int or (sy, sx),
    default half the window.  Window sides are multiples of 4 (the UNet halves its input twice); canvas sides are free."""

    def __init__(self, canvas_hw, tile_hw, stride=None, wrap_w: bool = False):
        self.canvas_hw = H, W = _pair(canvas_hw, "TileGrid: canvas_hw")
        self.tile_hw = h, w = _pair(tile_hw, "TileGrid: tile_hw")
        if h < 4 or w < 4 or h % 4 or w % 4:
            raise ValueError(f"TileGrid: window sides must be multiples of 4 (the UNet halves the latent twice), got {h} x {w}")
        if h > H or w > W:
            raise ValueError(f"TileGrid: a window of {h} x {w} is larger than the canvas {H} x {W}")
        sy, sx = (h // 2, w // 2) if stride is None else _pair(stride, "TileGrid: stride")
        self.stride = (sy, sx)
        self.wrap_w = bool(wrap_w)
        self.ys = tile_starts(H, h, sy)
        self.xs = tile_starts(W, w, sx, wrap=self.wrap_w)
        self.T = len(self.ys) * len(self.xs)

    def window(self, t: int) -> Tuple[int, int]:
        """(y, x) where window t starts."""
        return self.ys[t // len(self.xs)], self.xs[t % len(self.xs)]

    def __repr__(self):
        return f"TileGrid(canvas={self.canvas_hw}, tile={self.tile_hw}, ys={self.ys}, xs={self.xs}, wrap_w={self.wrap_w})"


def gaussian_weights(h: int, w: int, sigma: float = 0.1) -> torch.Tensor:
    """fp32 (h, w): g_h[i] * g_w[j], g_n[i] = exp(-(i - (n - 1) / 2)^2 / (2 (sigma n)^2)) (computed in float64, rounded once)."""
    if not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"gaussian_weights: sigma must be positive and finite, got {sigma}")

    def axis(n):
        i = torch.arange(n, dtype=torch.float64)
        return torch.exp(-(i - (n - 1) / 2) ** 2 / (2 * (sigma * n) ** 2))

    return (axis(int(h))[:, None] * axis(int(w))[None, :]).float()


def weight_map(weights, tile_hw) -> torch.Tensor:
    """"uniform" | "gaussian" | an (h, w) tensor -> a checked fp32 CPU map: finite and positive everywhere."""
    h, w = tile_hw
    if isinstance(weights, str):
        if weights == "uniform":
            return torch.ones((h, w), dtype=torch.float32)
        if weights == "gaussian":
            m = gaussian_weights(h, w)
        else:
            raise ValueError(f"tile weights: \"uniform\", \"gaussian\" or an (h, w) tensor, got {weights!r}")
    else:
        m = torch.as_tensor(weights).detach().to("cpu", torch.float32)
        if tuple(m.shape) != (h, w):
            raise ValueError(f"tile weights: the map must be (h, w) = {(h, w)}, got {tuple(m.shape)}")
    if not bool(torch.isfinite(m).all()) or not bool((m > 0).all()):
        raise ValueError("tile weights: the map must be finite and positive everywhere (a window's weight may underflow to 0 in fp32: "
                         "raise sigma)")
    return m.contiguous()


def _columns(x0: int, w: int, W: int) -> torch.Tensor:
    return (torch.arange(w) + x0) % W


def _check(canvas_shape, windows_shape, grid: TileGrid, what: str) -> None:
    rows, C, H, W = canvas_shape
    if (H, W) != grid.canvas_hw or tuple(windows_shape) != (rows * grid.T, C) + grid.tile_hw:
        raise ValueError(f"{what}: canvas {tuple(canvas_shape)} and windows {tuple(windows_shape)} do not fit {grid!r} "
                         f"(canvas (rows, C, H, W), windows (rows * T, C, h, w))")


def gather(canvas: torch.Tensor, grid: TileGrid, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The windows of `canvas` (rows, C, H, W) as (rows * T, C, h, w), channels_last; a bit-exact copy."""
    rows, C, H, W = canvas.shape
    h, w = grid.tile_hw
    if out is None:
        out = torch.empty((rows * grid.T, C, h, w), dtype=canvas.dtype, device=canvas.device).contiguous(memory_format=torch.channels_last)
    _check(canvas.shape, out.shape, grid, "tiles.gather")
    if canvas.device.type != "cpu":
        from . import ops
        if not canvas.is_contiguous(memory_format=torch.channels_last):
            canvas = canvas.contiguous(memory_format=torch.channels_last)
        ops.tile_gather(canvas, out, grid.ys, grid.xs, grid.wrap_w)
        return out
    view = out.view(rows, grid.T, C, h, w)
    for t in range(grid.T):
        y0, x0 = grid.window(t)
        view[:, t] = canvas[:, :, y0:y0 + h][:, :, :, _columns(x0, w, W)]
    return out


def blend(windows: torch.Tensor, grid: TileGrid, weights: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The canvas (rows, C, H, W) from its windows (rows * T, C, h, w): per pixel the weighted mean of the covering windows in
    ascending t (fp32 fma chain, one division, one rounding to the tensor's type); a pixel under one window takes its bits."""
    h, w = grid.tile_hw
    H, W = grid.canvas_hw
    rows, C = windows.shape[0] // grid.T, windows.shape[1]
    if out is None:
        out = torch.empty((rows, C, H, W), dtype=windows.dtype, device=windows.device).contiguous(memory_format=torch.channels_last)
    _check(out.shape, windows.shape, grid, "tiles.blend")
    if tuple(weights.shape) != (h, w):
        raise ValueError(f"tiles.blend: weights must be (h, w) = {(h, w)}, got {tuple(weights.shape)}")
    if windows.device.type != "cpu":
        from . import ops
        if not windows.is_contiguous(memory_format=torch.channels_last):
            windows = windows.contiguous(memory_format=torch.channels_last)
        ops.tile_blend(windows, out, weights.to(windows.device, torch.float32).contiguous(), grid.ys, grid.xs, grid.wrap_w)
        return out
    # the kernel's arithmetic: num = fma(w_t, e_t, num) in fp32 - the product of two fp32 values is exact in float64, so one float64
    # add rounded to fp32 is the fused result (but for a double rounding 2^-29 below the fp32 ulp)
    wt = weights.to(torch.float32)
    view = windows.view(rows, grid.T, C, h, w)
    num = torch.zeros((rows, C, H, W), dtype=torch.float32)
    den = torch.zeros((H, W), dtype=torch.float32)
    count = torch.zeros((H, W), dtype=torch.int32)
    first = torch.zeros((rows, C, H, W), dtype=windows.dtype)
    for t in range(grid.T):
        y0, x0 = grid.window(t)
        cols = _columns(x0, w, W)
        ys = slice(y0, y0 + h)
        e = view[:, t]
        fresh = (count[ys][:, cols] == 0)
        acc = (num[:, :, ys][:, :, :, cols].double() + wt.double() * e.double()).float()
        _put(num, ys, cols, acc)
        _put(first, ys, cols, torch.where(fresh, e, first[:, :, ys][:, :, :, cols]))
        den[ys, cols] = den[ys][:, cols] + wt
        count[ys, cols] = count[ys][:, cols] + 1
    if bool((count == 0).any()):
        raise ValueError("tiles.blend: the windows do not cover the canvas")
    out.copy_(torch.where(count == 1, first, (num / den).to(windows.dtype)))
    return out


def _put(dst: torch.Tensor, ys: slice, cols: torch.Tensor, src: torch.Tensor) -> None:
    """dst[:, :, ys, cols] = src (an indexed store: a chained `dst[...][...] = ` would write a copy)."""
    dst[:, :, ys, cols] = src
