"""HyperTile inside the compiled UNet: windowed self-attention (the A1111 / ComfyUI switch of that name).

The T = gh * gw tokens of a self-attention (`attn1`) site are a row-major gh x gw grid.  A tiling (nh, nw) cuts it into nh * nw
rectangular windows of th x tw tokens and every window attends to itself alone: score work drops by nh * nw, no weights, no training.
Row i of window (wy, wx) is token (wy * th + i // tw) * gw + wx * tw + i % tw.

The draw, restated from the method's description (parity with either UI's node is unpinned; their depth scaling is not built): per
axis of g tokens the candidate window sides are the `swap` smallest divisors of g that are >= min(g, tile), `tile` in tokens; per
step and site one side per axis is drawn from a host generator seeded with (seed, site index).  Steps outside
[int(start * n), int(end * n)) take the whole grid, tiling (1, 1).

What a site can run is fixed when it is first called (outside any capture), from (grid, heads, batch rows) alone, so that a captured
launch keeps its grid whatever is drawn later: the kernel (ops.attention_windows, csrc/attention_windows.hip) runs R query rows per
block, R = `rows_per_block`.  Candidates that fail the kernel's conditions are dropped from the draw: window widths that are no
multiple of 8, and then - smallest side first, heights before widths - sides until R divides th * tw of every remaining pair.  If
none but the whole grid is left, if the grid's width is no multiple of 8, if no R divides T, or if T < 256 (ordinary attention is then
on another kernel family, with other bits), THE SITE STAYS ORDINARY ATTENTION: ops.attention, the launch and the bits of a module
compiled without the pass.  A tiled site whose table holds (1, 1) everywhere also gives those bits (the same body on the same rows).

The state module `gm.hypertile` holds the per-site DEVICE tables of n_steps pairs (nh, nw) the launches read at the step counter:
`bind(n_steps)` once, `set(tile, swap, seed, start, end)` / `set(None)` write them in place, before or after a capture;
`using(latent_hw, step)` names the call's latent size and its int32 device step counter for the caller's own UNet calls.  Outside
`using` the sites are ordinary attention.  fp32 (strict mode) and head sizes other than 64 take ops.attention_windows' slow path at a
HOST tiling: every row of the site's table must then be the same pair (swap = 1, start = 0, end = 1; `set` and the site's first call
raise otherwise), and a captured graph does not follow later writes (per-step draws on the slow path are not built).  Such sites, and
CPU sites, have no block form: R = 1, so only the width and size rules drop candidates there, and the operator library is not loaded.
"""
from __future__ import annotations

import contextlib
import random
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from .seg import site_grid
from .state import require_state

ROW_FORMS = (256, 128, 96)      # query rows per block of st_attention_windows' three forms (bit i of its row_forms)
MIN_TOKENS = 256                # below it st_attention runs the 16-row kernel family


def candidates(g: int, tile: int, swap: int) -> List[int]:
    """The `swap` smallest divisors of g that are >= min(g, tile)."""
    if g < 1 or tile < 1 or swap < 1:
        raise ValueError(f"hypertile: g, tile and swap must be positive, got {g}, {tile}, {swap}")
    lo = min(g, tile)
    return [d for d in range(lo, g + 1) if g % d == 0][:swap]


def rows_per_block(T: int, H: int, B: int) -> Optional[int]:
    """R of a site: the form st_attention_windows picks (att_win_rows: CUs filled at (T, H, B)) among those that divide the whole
    grid's T; None when none does.  Host arithmetic of the operator library, no device needed."""
    fits = sum(1 << i for i, r in enumerate(ROW_FORMS) if T % r == 0)
    if not fits:
        return None
    from . import _C
    return int(_C.load().st_attention_windows_rows(T, H, B, fits))


def check_tiling(grid_hw, tiling, rows: Optional[int] = None) -> Tuple[int, int]:
    """(nh, nw) as integers, or a ValueError: nh | gh, nw | gw, and - with `rows`, the kernel's conditions - tw % 8 == 0 and rows | th * tw."""
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    nh, nw = tiling
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in (nh, nw)) or gh % nh or gw % nw:
        raise ValueError(f"hypertile: tiling {tuple(tiling)!r} does not divide the {gh} x {gw} token grid")
    if rows is not None:
        th, tw = gh // nh, gw // nw
        if tw % 8:
            raise ValueError(f"hypertile: tiling ({nh}, {nw}) of the {gh} x {gw} grid has windows {tw} tokens wide: the kernel takes multiples of 8")
        if (th * tw) % rows:
            raise ValueError(f"hypertile: tiling ({nh}, {nw}) of the {gh} x {gw} grid has windows of {th * tw} tokens: no multiple of the "
                             f"site's {rows} query rows per block")
    return nh, nw


def site_sides(grid_hw, rows: Optional[int], tile: int, swap: int):
    """(window heights, window widths) a site draws from, after the drops of the module docstring; None: ordinary attention."""
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    if rows is None or gw % 8 or (gh * gw) % rows or gh * gw < MIN_TOKENS:
        return None
    hs = candidates(gh, tile, swap)
    ws = [w for w in candidates(gw, tile, swap) if w % 8 == 0]
    while any((th * tw) % rows for th in hs or [gh] for tw in ws or [gw]):
        if hs and (not ws or hs[0] <= ws[0]):
            hs.pop(0)
        else:
            ws.pop(0)
    hs, ws = hs or [gh], ws or [gw]
    return None if hs == [gh] and ws == [gw] else (hs, ws)


def draw_table(grid_hw, sides, n_steps: int, seed: int, site: int, start: float = 0.0, end: float = 1.0) -> List[Tuple[int, int]]:
    """n_steps pairs (nh, nw): one side per axis per step inside [int(start * n), int(end * n)), (1, 1) outside; sides None: all (1, 1)."""
    if not 0.0 <= start <= end <= 1.0:
        raise ValueError(f"hypertile: 0 <= start <= end <= 1 expected, got start={start}, end={end}")
    gh, gw = int(grid_hw[0]), int(grid_hw[1])
    rng = random.Random(int(seed) * 1000003 + int(site))
    lo, hi = int(start * n_steps), int(end * n_steps)
    table = []
    for i in range(n_steps):
        if sides is None or not lo <= i < hi:
            table.append((1, 1))
        else:
            table.append((gh // rng.choice(sides[0]), gw // rng.choice(sides[1])))
    return table


def windows_gather(t: torch.Tensor, grid_hw, tiling) -> torch.Tensor:
    """(B, gh * gw, C) -> (B * nh * nw, th * tw, C), window-major."""
    gh, gw = grid_hw
    nh, nw = check_tiling(grid_hw, tiling)
    B, T, C = t.shape
    th, tw = gh // nh, gw // nw
    return t.reshape(B, nh, th, nw, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nh * nw, th * tw, C)


def windows_scatter(t: torch.Tensor, grid_hw, tiling) -> torch.Tensor:
    """The inverse of windows_gather."""
    gh, gw = grid_hw
    nh, nw = check_tiling(grid_hw, tiling)
    th, tw = gh // nh, gw // nw
    C = t.shape[-1]
    B = t.shape[0] // (nh * nw)
    return t.reshape(B, nh, nw, th, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(B, gh * gw, C)


def windows_attention_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, sm_scale: float, grid_hw,
                                tiling=(1, 1)) -> torch.Tensor:
    """Plain torch: the attention core on (B, T, H*D) projections, every window of the tiling on its own."""
    qw, kw, vw = (windows_gather(t, grid_hw, tiling) for t in (q, k, v))
    d = q.shape[-1] // num_heads

    def heads(t):
        return t.reshape(t.shape[0], t.shape[1], num_heads, d).transpose(1, 2)

    w = torch.softmax(torch.matmul(heads(qw), heads(kw).transpose(-2, -1)) * sm_scale, dim=-1)
    return windows_scatter(torch.matmul(w, heads(vw)).transpose(1, 2).reshape(qw.shape), grid_hw, tiling)


def _check_host_tiled(key, table) -> None:
    """A device site off the kernel (key: HyperTile.site) takes one pair for every step."""
    if not key[-1] and key[4] != "cpu" and len(set(table)) != 1:
        raise ValueError("hypertile: fp32 and head sizes other than 64 take the slow path at one host tiling: per-step draws there are not "
                         "built (use swap=1, start=0, end=1)")


class Site:
    """One (site index, grid, heads, rows, device) of a state: R (None: ordinary attention), the host table and its device copy."""

    def __init__(self, grid, rows, host, device):
        self.grid, self.rows, self.host = grid, rows, host
        self.table = None if rows is None else torch.tensor(host, dtype=torch.int32, device=device).reshape(-1, 2).contiguous()

    def write(self, host) -> None:
        self.host = host
        if self.table is not None:
            self.table.copy_(torch.tensor(host, dtype=torch.int32).reshape(-1, 2))


class HyperTile(nn.Module):
    """State of one compiled module whose selected self-attention sites can run windowed (module docstring)."""

    def __init__(self, sites: Sequence[str] = (), layers: Sequence[str] = ()):
        super().__init__()
        self.sites = tuple(sites)
        self.layers = tuple(layers)
        self.n_steps = 0
        self.params = None                  # (tile, swap, seed, start, end), or None: every table all (1, 1)
        self.latent_hw = None               # of the current calls (using)
        self.step = None
        self._sites: Dict[tuple, Site] = {}

    def bind(self, n_steps: int) -> None:
        """Rows per table; the tables themselves are made at a site's first call, which must not be captured."""
        if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 1:
            raise ValueError(f"hypertile: n_steps must be a positive integer, got {n_steps!r}")
        if self._sites and n_steps != self.n_steps:
            raise ValueError(f"hypertile: the state's tables hold {self.n_steps} steps; a loop of {n_steps} steps needs a module of its own")
        self.n_steps = n_steps

    def _host_table(self, index: int, grid, rows, params):
        if params is None:
            return [(1, 1)] * self.n_steps
        tile, swap, seed, start, end = params
        table = draw_table(grid, site_sides(grid, rows, tile, swap), self.n_steps, seed, index, start, end)
        for pair in table:                  # every pair written is one the kernel can trust
            check_tiling(grid, pair, rows)
        return table

    def set(self, tile: Optional[int] = 32, swap: int = 2, seed: int = 0, start: float = 0.0, end: float = 1.0) -> None:
        """Draw every site's table again and write it in place (the launches of a captured graph read the tables by address);
        `set(None)`: every row (1, 1)."""
        params = None
        if tile is not None:
            for name, v in (("tile", tile), ("swap", swap)):
                if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                    raise ValueError(f"hypertile: {name} must be a positive integer, got {v!r}")
            draw_table((1, 1), None, 1, seed, 0, start, end)      # range check of start / end
            params = (tile, swap, int(seed), float(start), float(end))
        new = {key: self._host_table(key[0], site.grid, site.rows, params) for key, site in self._sites.items() if site.rows is not None}
        for key, table in new.items():      # nothing is written unless every existing site can follow
            _check_host_tiled(key, table)
        self.params = params
        for key, table in new.items():
            self._sites[key].write(table)

    @property
    def host_tiled(self) -> bool:
        """Whether a device site of the state runs the slow path: its tiling is a HOST value, fixed in a graph when it is captured."""
        return any(site.rows is not None and not key[-1] and key[4] != "cpu" for key, site in self._sites.items())

    @contextlib.contextmanager
    def using(self, latent_hw, step: torch.Tensor):
        """The latent size and the int32 device step counter of the calls made inside the block; the previous values come back."""
        before = (self.latent_hw, self.step)
        self.latent_hw, self.step = (int(latent_hw[0]), int(latent_hw[1])), step
        try:
            yield self
        finally:
            self.latent_hw, self.step = before

    def site(self, index: int, tokens: int, heads: int, batch: int, device, kernel: bool) -> Site:
        grid = site_grid(self.latent_hw, tokens)
        key = (index, grid, heads, batch, device.type, device.index, kernel)
        site = self._sites.get(key)
        if site is None:
            if self.n_steps < 1:
                raise ValueError("hypertile: bind(n_steps) must precede the first call inside using()")
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("hypertile: a site's table is made at its first call: run one call outside the capture first")
            rows = rows_per_block(tokens, heads, batch) if kernel else 1      # the slow path and the CPU have no block form
            if rows is not None and site_sides(grid, rows, 1, 1 << 30) is None:      # no draw can ever tile it: ordinary attention for good
                rows = None
            host = self._host_table(index, grid, rows, self.params)
            if rows is not None:
                _check_host_tiled(key, host)
            site = self._sites[key] = Site(grid, rows, host, device)
        return site

    def extra_repr(self) -> str:
        return f"sites={len(self.sites)}, n_steps={self.n_steps}, params={self.params}"


def attention_hypertile_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                                state: HyperTile, index: int) -> torch.Tensor:
    """fx leaf: attention_wrapper whose token grid is cut into the windows of the site's table row at the step counter."""
    cpu = q.device.type == "cpu"
    if not cpu:
        from . import ops
        if q.shape[-1] != num_heads * head_dim:
            raise ops.BackendError(f"attention_hypertile_wrapper: C={q.shape[-1]} != num_heads*head_dim={num_heads * head_dim}")
    if state.latent_hw is None or q.shape[1] != k.shape[1]:
        return windows_attention_reference(q, k, v, num_heads, sm_scale, (1, q.shape[1])) if cpu else ops.attention(q, k, v, num_heads, sm_scale)
    kernel = not cpu and q.dtype in (torch.bfloat16, torch.float16) and head_dim == 64
    site = state.site(index, q.shape[1], num_heads, q.shape[0], q.device, kernel)
    if site.rows is None:
        return windows_attention_reference(q, k, v, num_heads, sm_scale, site.grid) if cpu else ops.attention(q, k, v, num_heads, sm_scale)
    if cpu:
        i = min(max(int(state.step.reshape(-1)[0]), 0), state.n_steps - 1)
        return windows_attention_reference(q, k, v, num_heads, sm_scale, site.grid, site.host[i])
    if kernel:
        return ops.attention_windows(q, k, v, num_heads, sm_scale, site.grid, table=(state.step, site.table), rows=site.rows)
    return ops.attention_windows(q, k, v, num_heads, sm_scale, site.grid, tiling=site.host[0])


torch.fx.wrap("attention_hypertile_wrapper")


def state_of(module, what: str) -> HyperTile:
    """The HyperTile state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "hypertile", HyperTile, what, "windowed self-attention sites", 'hypertile_layers=(".*",)')
