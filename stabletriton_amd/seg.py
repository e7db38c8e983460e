"""Smoothed energy guidance (SEG; Hong, "Smoothed Energy Guidance: Guiding Diffusion Models with Reduced Energy Curvature of
Attention", 2024) inside the compiled UNet.

As with PAG (pag.py) the UNet evaluates one more block of batch rows, the "perturbed" prediction, from the positive conditioning and
the same latent, and the sampler adds `s * (e_pos - e_pert)` to the guided prediction (the same `st_pag_*` update launches).  The
perturbation has arithmetic in it: in the selected self-attention (`attn1`) sites the projected QUERIES of the perturbed rows are
Gaussian-blurred over the latent grid, at sigma = infinity replaced by their spatial mean; keys and values stay as they are.

The rule, for a site with T = h * w tokens and queries q (n, T, H * D) read as H * D planes of h x w, token t = y * w + x:
    c = ceil(6 sigma), k = c + 1 - (c mod 2), clamped to m + 1 - (m mod 2) with m = min(h, w) (k odd, k // 2 < m);
    g_i = exp(-(x_i / sigma)^2 / 2) / sum_j exp(-(x_j / sigma)^2 / 2), x_i = i - (k - 1) / 2;
    every plane becomes the separable convolution g (x) g of its reflect-padded self (pad k // 2, the edge sample not repeated);
    sigma >= 9999 (infinity): every token of a plane becomes the plane's mean instead.
The published implementation assumes a square grid; aspect buckets are why the clamp uses min(h, w).  The site's (h, w) follows from
the call's latent (lh, lw) and T: f = sqrt(lh lw / T) must be an integer that divides both sides, (h, w) = (lh / f, lw / f).

Batch layout and `chunks` as in pag.py: the perturbed rows are the LAST `B // chunks` batch entries of a UNet call.  The state module
`gm.seg` holds `chunks` and the call's latent size, both host values set for the duration of a caller's own UNet calls with
`state.using(chunks, latent_hw)`, sigma, and one DEVICE parameter row [mode, k, taps...] per token grid.  The rows are what the
kernels read: `set_sigma` recomputes them on the host and writes them in place, finite <-> infinity included, so a captured graph
follows without a new capture.  `bind(latent_hw, device)` allocates the rows of a latent size outside any capture; the leaf only
looks them up.

`attention_seg_wrapper` is the fx leaf optimizers/insert_seg.py puts in place of `attention_wrapper` at the selected sites: HIP
(ops.attention_seg, csrc/seg.hip) for device tensors, a plain torch statement for CPU tensors so that a traced CPU module can carry
the pass on its own.  With chunks == 0 it is ops.attention: the launch and the bits of a module compiled without the pass.
"""
from __future__ import annotations

import contextlib
import math
import numbers
from typing import Dict, List, Sequence, Tuple

import torch

from .pag import PerturbedRows
from .state import require_state

MEAN_SIGMA = 9999.0          # sigma at or beyond this is infinity: the plane's mean
MAX_SIDE = 128               # st_seg_blur's largest token grid side (ST_SEG_MAX_SIDE)
PARAM_WORDS = 132            # floats of a parameter row: mode, k, then the taps of at most a 128 x 128 grid (ST_SEG_PARAM_WORDS)
FACTORS = (1, 2, 4, 8)       # latent side / token grid side at the UNet's attention levels


def check_sigma(sigma) -> float:
    if isinstance(sigma, bool) or not isinstance(sigma, numbers.Real) or math.isnan(sigma) or sigma <= 0:
        raise ValueError(f"SEG: sigma must be a positive number (float('inf') for the mean), got {sigma!r}")
    return float(sigma)


def tap_count(sigma: float, h: int, w: int) -> int:
    c = int(math.ceil(6.0 * sigma))
    k = c + 1 - (c % 2)
    m = min(h, w)
    return min(k, m + 1 - (m % 2))


def taps(sigma: float, k: int) -> List[float]:
    xs = [i - (k - 1) / 2.0 for i in range(k)]
    e = [math.exp(-0.5 * (x / sigma) ** 2) for x in xs]
    total = math.fsum(e)
    return [v / total for v in e]


def param_row(sigma: float, h: int, w: int) -> List[float]:
    """The host image of a device row: [mode, k, g_0 ... g_{k-1}, 0 ...]; mode 1 (sigma = infinity) carries no taps."""
    sigma = check_sigma(sigma)
    row = [0.0] * PARAM_WORDS
    if sigma >= MEAN_SIGMA:
        row[0], row[1] = 1.0, 1.0
        return row
    k = tap_count(sigma, h, w)
    row[1] = float(k)
    row[2:2 + k] = taps(sigma, k)
    return row


def site_grid(latent_hw, tokens: int) -> Tuple[int, int]:
    """(h, w) of a site with `tokens` query rows in a call whose latent is `latent_hw`."""
    lh, lw = int(latent_hw[0]), int(latent_hw[1])
    f = math.isqrt((lh * lw) // tokens) if tokens > 0 else 0
    if f < 1 or f * f * tokens != lh * lw or lh % f or lw % f:
        raise ValueError(f"SEG: a self-attention with {tokens} tokens is no whole-number reduction of a {lh} x {lw} latent")
    return lh // f, lw // f


def blur_reference(q: torch.Tensor, grid_hw, sigma: float) -> torch.Tensor:
    """Plain torch: the blur of q (n, T, C) over the (h, w) token grid, in q's dtype."""
    h, w = grid_hw
    n, T, C = q.shape
    if sigma >= MEAN_SIGMA:
        return q.mean(dim=1, keepdim=True).expand(n, T, C).contiguous()
    k = tap_count(sigma, h, w)
    g, r = taps(sigma, k), k // 2

    def axis_matrix(length: int) -> torch.Tensor:
        m = torch.zeros((length, length), dtype=q.dtype)
        for p in range(length):
            for i in range(k):
                j = abs(p + i - r)
                j = 2 * (length - 1) - j if j >= length else j
                m[p, j] += g[i]
        return m

    planes = q.reshape(n, h, w, C)
    planes = torch.einsum("xj,nyjc->nyxc", axis_matrix(w), planes)
    planes = torch.einsum("yj,njxc->nyxc", axis_matrix(h), planes)
    return planes.reshape(n, T, C)


class SEG(PerturbedRows):
    """pag.PerturbedRows (site names, `chunks` and `latent_hw` of the current call) with sigma and the device parameter rows by
    (device, token grid)."""
    label = "SEG"

    def __init__(self, sites: Sequence[str] = (), layers: Sequence[str] = ()):
        super().__init__(sites, layers)
        self.sigma = float("inf")
        self._rows: Dict[tuple, torch.Tensor] = {}

    @contextlib.contextmanager
    def using(self, chunks: int, latent_hw=None):
        if chunks and latent_hw is None:
            raise ValueError("SEG: using(chunks, latent_hw) needs the call's latent size: the sites derive their token grids from it")
        with super().using(chunks, latent_hw):
            yield self

    # ---- device parameter rows ----
    @staticmethod
    def grids(latent_hw) -> List[Tuple[int, int]]:
        lh, lw = int(latent_hw[0]), int(latent_hw[1])
        return [(lh // f, lw // f) for f in FACTORS if lh % f == 0 and lw % f == 0 and max(lh // f, lw // f) <= MAX_SIDE]

    def _ensure(self, device: torch.device, grid: Tuple[int, int]) -> torch.Tensor:
        key = (device.type, device.index, grid)
        row = self._rows.get(key)
        if row is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"SEG: no parameter row for the {grid[0]} x {grid[1]} token grid and a stream capture is running: "
                                   "call bind(latent_hw, device) before capturing")
            row = self._rows[key] = torch.tensor(param_row(self.sigma, *grid), dtype=torch.float32, device=device)
        return row

    def bind(self, latent_hw, device) -> None:
        """Allocate (outside any capture) the parameter rows of the token grids a `latent_hw` call can have and fill them for the
        current sigma; rows that exist are left alone."""
        device = torch.device(device)
        for grid in self.grids(latent_hw):
            self._ensure(device, grid)

    def set_sigma(self, sigma: float) -> None:
        """Recompute k and the taps of every bound row on the host and write them in place (finite <-> infinity included): the
        launches of a captured graph read the rows by address."""
        self.sigma = check_sigma(sigma)
        for (_, _, grid), row in self._rows.items():
            row.copy_(torch.tensor(param_row(self.sigma, *grid), dtype=torch.float32))

    def row_for(self, tokens: int, device) -> Tuple[Tuple[int, int], torch.Tensor]:
        """((h, w), device row) of a site with `tokens` query rows in the current call."""
        if self.latent_hw is None:
            raise ValueError("SEG: the call's latent size is not set: wrap the UNet call in state.using(chunks, latent_hw)")
        grid = site_grid(self.latent_hw, tokens)
        if max(grid) > MAX_SIDE:
            raise ValueError(f"SEG: the token grid {grid[0]} x {grid[1]} is larger than {MAX_SIDE} x {MAX_SIDE}")
        return grid, self._ensure(torch.device(device), grid)

    def extra_repr(self) -> str:
        return f"sites={len(self.sites)}, chunks={self.chunks}, sigma={self.sigma}"


def blurred_attention_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, sm_scale: float, tail: int,
                                grid_hw, sigma: float) -> torch.Tensor:
    """Plain torch: the attention core on (B, T, H*D) projections whose last `tail` batch entries take blurred queries."""
    B, T, C = q.shape
    if tail > 0:
        q = torch.cat([q[:B - tail], blur_reference(q[B - tail:], grid_hw, sigma)], dim=0)
    d = C // num_heads

    def heads(t):
        return t.reshape(B, t.shape[1], num_heads, d).transpose(1, 2)

    w = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-2, -1)) * sm_scale, dim=-1)
    return torch.matmul(w, heads(v)).transpose(1, 2).reshape(B, T, C)


def attention_seg_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                          state: SEG) -> torch.Tensor:
    """fx leaf: attention_wrapper whose last B // state.chunks batch entries are perturbed (blurred queries)."""
    tail = state.tail_count(q.shape[0])
    if q.device.type == "cpu":
        grid = site_grid(state.latent_hw, q.shape[1]) if tail else None
        return blurred_attention_reference(q, k, v, num_heads, sm_scale, tail, grid, state.sigma)
    from . import ops
    if q.shape[-1] != num_heads * head_dim:
        raise ops.BackendError(f"attention_seg_wrapper: C={q.shape[-1]} != num_heads*head_dim={num_heads * head_dim}")
    if tail == 0:
        return ops.attention(q, k, v, num_heads, sm_scale)
    grid, row = state.row_for(q.shape[1], q.device)
    return ops.attention_seg(q, k, v, num_heads, sm_scale, tail, grid, row)


torch.fx.wrap("attention_seg_wrapper")


def state_of(module, what: str) -> SEG:
    """The SEG state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "seg", SEG, what, "smoothed-energy sites", 'seg_layers=("mid",)')
