"""Token merging inside the compiled UNet (ToMe for Stable Diffusion, Bolya & Hoffman 2023; the A1111 "Token merging ratio", ComfyUI's
TomePatchModel, `tomesd.apply_patch`).  Restated from the method's description; parity with `tomesd` is unpinned.

A site is the `attn1` half of a transformer block, `x + to_out(attn1(norm1(x)))`, x (B, N, C) on an h x w token grid with both sides
even.  The grid is D = (h / 2)(w / 2) cells of 2 x 2 tokens; `off[c]` in 0..3 names the cell's dst token, slot (off >> 1, off & 1) - token
(2 cy + (off >> 1)) w + 2 cx + (off & 1) - and its three other tokens are the src tokens s = 3 c + k, k = 0..2, at slot k + (k >= off[c]).
S = 3 D.  Per batch row, on the pre-norm x:
    match    node_max[s] = max_j cos(src s, dst j), node_idx[s] the smallest such j;
    select   rank[s] = #{t: node_max[t] > node_max[s]} + #{t < s: node_max[t] == node_max[s]}; src s is merged iff rank[s] < r;
             where[token] = j for dst j, node_idx[s] for a merged src, D + rank[s] - r for a kept one (the argsort order, without a sort);
    merge    row m < D of the (B, N - r, C) tensor = (LN(x_dst m) + sum of LN(x_s) over the merged s with node_idx[s] = m, ascending s)
             / (1 + their number), row D + rank - r = LN(x_s) of a kept src; LN = norm1, sums in fp32;
    unmerge  out[token] = x[token] + y[where[token]], y = to_out(attention(q|k|v of the merged rows)).
r = min(S, int(N * ratio)), lowered until N - r is a multiple of ROWS = 32: the attention kernels' query block, which is also two of
the projection GEMMs' 16-row MFMA tiles, so neither launch of the shrunk site ends a batch entry on a ragged block.  `ratio` is a
compile-time value (a captured graph's shapes are static); the `off` tables are DEVICE data, one uint8 row of D per step and token grid,
shared by the batch rows and by the sites of one grid, drawn on the host from (seed, grid) and written in place: `set(seed)` /
`set(None)` (all 0, the method's use_rand=False) before or after a capture, no new capture.

The four launches are ops.tome_match / tome_select / tome_merge_norm / tome_unmerge_add (csrc/tome.hip); the projections, the attention
and to_out run on N - r rows through the launches they always had.  A site runs them for bf16 / fp16 device tensors inside
`using(latent_hw, step)`, on an even grid, with C a multiple of 64 up to MAX_C and S <= MAX_SRC (the kernels keep S words in LDS).
EVERYTHING ELSE - fp32 strict mode, CPU tensors, calls outside `using`, odd grids, sites over the caps - IS THE UNMERGED CHAIN: norm1 as a
launch of its own, the projections on N rows, a plain add; ToMe is off for that site.  That is not bit-equal to a UNet compiled
without `tome_layers`: there norm1 is folded into the q|k|v projection and the residual into to_out's epilogue.

`match_reference`, `select_reference`, `merge_reference`, `unmerge_reference` state the same maths in plain torch, in the dtype they
are given (the tests run them in float64).
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from .seg import site_grid
from .state import require_state

ROWS = 32                 # N - r is a multiple of it (module docstring)
MAX_SRC = 12288           # ops.TOME_MAX_SRC: S of the largest site the kernels take (a 128 x 128 token grid)
MAX_C = 2048              # ops.TOME_MAX_C


def check_ratio(ratio) -> float:
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= ratio <= 0.75:
        raise ValueError(f"tome: ratio must be a number in [0, 0.75] (at most the 3/4 of the tokens that are src), got {ratio!r}")
    return float(ratio)


def merged_count(tokens: int, ratio: float, rows: int = ROWS) -> int:
    """r of a site with `tokens` tokens: min(S, int(N ratio)), lowered so that N - r is a multiple of `rows` (0 when none fits)."""
    r = min(tokens // 4 * 3, int(tokens * ratio))
    r -= (rows - (tokens - r) % rows) % rows
    return max(r, 0)


def draw_offsets(grid_hw, n_steps: int, seed: Optional[int]) -> torch.Tensor:
    """The host table (n_steps, D) uint8 of a token grid: uniform in 0..3 from a generator seeded with (seed, grid); None: all 0."""
    h, w = int(grid_hw[0]), int(grid_hw[1])
    if seed is None:
        return torch.zeros((n_steps, h * w // 4), dtype=torch.uint8)
    gen = torch.Generator().manual_seed((int(seed) * 1000003 + h * 4099 + w) % (1 << 63))
    return torch.randint(0, 4, (n_steps, h * w // 4), generator=gen, dtype=torch.uint8)


def site_tokens(grid_hw, off_row: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dst tokens (D,), src tokens (S,)) of one table row, as int64 indices into the token axis."""
    h, w = int(grid_hw[0]), int(grid_hw[1])
    if h % 2 or w % 2:
        raise ValueError(f"tome: the token grid {h} x {w} must have even sides")
    wc = w // 2
    c = torch.arange(h * w // 4, device=off_row.device)
    o = off_row.to(torch.int64) & 3
    base = (2 * (c // wc)) * w + 2 * (c % wc)
    dst = base + (o >> 1) * w + (o & 1)
    k = torch.arange(3, device=off_row.device)[None, :]
    slot = k + (k >= o[:, None]).to(torch.int64)
    src = (base[:, None] + (slot >> 1) * w + (slot & 1)).reshape(-1)
    return dst, src


def match_reference(x: torch.Tensor, grid_hw, off_row: torch.Tensor):
    """node_max (B, S) in x's dtype and node_idx (B, S) int64: cosines of every src to every dst, row maximum, smallest arg-max."""
    dst, src = site_tokens(grid_hw, off_row)
    xn = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    score = xn[:, src] @ xn[:, dst].transpose(1, 2)
    node_max = score.max(dim=-1).values
    first = (score == node_max[..., None]).to(torch.int64).argmax(dim=-1)      # argmax of a 0/1 tensor: the first 1
    return node_max, first


def select_reference(node_max: torch.Tensor, node_idx: torch.Tensor, grid_hw, r: int, off_row: torch.Tensor):
    """(where (B, N), assign (B, S), kept (B, S - r)) int64, by the counting rule of the module docstring."""
    dst, src = site_tokens(grid_hw, off_row)
    B, S = node_max.shape
    D = S // 3
    t = torch.arange(S, device=node_max.device)
    node_max = torch.nan_to_num(node_max, nan=float("-inf"), posinf=float("inf"), neginf=float("-inf"))      # as the kernel ranks a NaN
    before = (node_max[:, None, :] > node_max[:, :, None]) | ((node_max[:, None, :] == node_max[:, :, None]) & (t[None, None, :] < t[None, :, None]))
    rank = before.sum(dim=-1)
    merged = rank < r
    rows = torch.where(merged, node_idx.to(torch.int64), D + rank - r)
    where = torch.empty((B, 4 * D), dtype=torch.int64, device=node_max.device)
    where[:, dst] = torch.arange(D, device=node_max.device)
    where[:, src] = rows
    assign = torch.where(merged, node_idx.to(torch.int64), torch.full_like(rank, -1))
    kept = torch.argsort(rank, dim=-1)[:, r:]
    return where, assign, kept


def merge_reference(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float, grid_hw, r: int, assign: torch.Tensor,
                    kept: torch.Tensor, off_row: torch.Tensor) -> torch.Tensor:
    """(B, N - r, C): the mean of LayerNorm(x) over every dst and what merges into it, then the LayerNorm of the kept src."""
    ln = torch.nn.functional.layer_norm(x, (x.shape[-1],), weight.to(x.dtype), bias.to(x.dtype), eps)
    return merge_rows(ln, grid_hw, r, assign, kept, off_row)


def merge_rows(ln: torch.Tensor, grid_hw, r: int, assign: torch.Tensor, kept: torch.Tensor, off_row: torch.Tensor) -> torch.Tensor:
    """The merge alone, on per-token rows (B, N, C) that are already normalised (or on anything else per token, such as a bound)."""
    dst, src = site_tokens(grid_hw, off_row)
    x = ln
    B, D = x.shape[0], dst.numel()
    ln_src = ln[:, src]
    merged = (assign >= 0)
    total = ln[:, dst].clone()
    count = torch.ones((B, D), dtype=x.dtype, device=x.device)
    index = assign.clamp_min(0)
    total.scatter_add_(1, index[..., None].expand_as(ln_src), ln_src * merged[..., None].to(x.dtype))
    count.scatter_add_(1, index, merged.to(x.dtype))
    rest = torch.gather(ln_src, 1, kept[:, :src.numel() - r, None].expand(-1, -1, x.shape[-1]))
    return torch.cat([total / count[..., None], rest], dim=1)


def unmerge_reference(x: torch.Tensor, y: torch.Tensor, where: torch.Tensor) -> torch.Tensor:
    return x + torch.gather(y, 1, where.to(torch.int64)[..., None].expand(-1, -1, y.shape[-1]))


class Plan:
    """What the three leaves of one site call pass along: r None = the unmerged chain."""
    __slots__ = ("grid", "r", "off", "step", "where", "assign", "kept")

    def __init__(self, grid=None, r=None, off=None, step=None, where=None, assign=None, kept=None):
        self.grid, self.r, self.off, self.step, self.where, self.assign, self.kept = grid, r, off, step, where, assign, kept


class ToMe(nn.Module):
    """State of one compiled module whose selected self-attention sites can merge tokens (module docstring)."""

    def __init__(self, sites: Sequence[str] = (), layers: Sequence[str] = (), ratio: float = 0.5):
        super().__init__()
        self.sites = tuple(sites)
        self.layers = tuple(layers)
        self.ratio = check_ratio(ratio)
        self.n_steps = 0
        self.seed: Optional[int] = None     # None: every offset 0
        self.latent_hw = None               # of the current calls (using)
        self.step = None
        self._tables: Dict[tuple, torch.Tensor] = {}      # (grid, device type, device index) -> uint8 (n_steps, D), never reallocated

    def bind(self, n_steps: int) -> None:
        """Rows per table; the tables themselves are made at a grid's first call, which must not be captured."""
        if isinstance(n_steps, bool) or not isinstance(n_steps, int) or n_steps < 1:
            raise ValueError(f"tome: n_steps must be a positive integer, got {n_steps!r}")
        if self._tables and n_steps != self.n_steps:
            raise ValueError(f"tome: the state's tables hold {self.n_steps} steps; a loop of {n_steps} steps needs a module of its own")
        self.n_steps = n_steps

    def set(self, seed: Optional[int] = 0) -> None:
        """Draw every grid's table again from (seed, grid) and write it in place (the launches of a captured graph read the tables by
        address); `set(None)`: every offset 0."""
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int)):
            raise ValueError(f"tome: seed must be an integer or None, got {seed!r}")
        self.seed = seed
        for key, table in self._tables.items():
            table.copy_(draw_offsets(key[0], self.n_steps, seed))

    @contextlib.contextmanager
    def using(self, latent_hw, step: torch.Tensor):
        """The latent size and the int32 device step counter of the calls made inside the block; the previous values come back."""
        before = (self.latent_hw, self.step)
        self.latent_hw, self.step = (int(latent_hw[0]), int(latent_hw[1])), step
        try:
            yield self
        finally:
            self.latent_hw, self.step = before

    def table(self, grid, device) -> torch.Tensor:
        key = (grid, device.type, device.index)
        table = self._tables.get(key)
        if table is None:
            if self.n_steps < 1:
                raise ValueError("tome: bind(n_steps) must precede the first call inside using()")
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("tome: a grid's table is made at its first call: run one call outside the capture first")
            table = self._tables[key] = draw_offsets(grid, self.n_steps, self.seed).to(device)
        return table

    def plan(self, x: torch.Tensor) -> Plan:
        """Whether a site called with x merges, and with which table: the conditions of the module docstring."""
        if self.latent_hw is None or x.device.type != "cuda" or x.dtype not in (torch.bfloat16, torch.float16) or x.dim() != 3:
            return Plan()
        N, C = x.shape[1], x.shape[2]
        try:
            grid = site_grid(self.latent_hw, N)
        except ValueError:
            return Plan()
        r = merged_count(N, self.ratio)
        if grid[0] % 2 or grid[1] % 2 or C % 64 or C > MAX_C or N // 4 * 3 > MAX_SRC or r < 1:
            return Plan()
        return Plan(grid, r, self.table(grid, x.device), self.step)

    def extra_repr(self) -> str:
        return f"sites={len(self.sites)}, ratio={self.ratio}, n_steps={self.n_steps}, seed={self.seed}"


def tome_plan_wrapper(x: torch.Tensor, state: ToMe) -> Plan:
    """fx leaf: match + select on the pre-norm x of a site (two launches), or the empty plan of the unmerged chain."""
    plan = state.plan(x)
    if plan.r is not None:
        from . import ops
        node_max, node_idx = ops.tome_match(x, plan.grid, plan.off, plan.step)
        plan.where, plan.assign, plan.kept = ops.tome_select(node_max, node_idx, plan.grid, plan.r, plan.off, plan.step)
    return plan


def tome_merge_wrapper(x: torch.Tensor, layernorm: nn.LayerNorm, plan: Plan) -> torch.Tensor:
    """fx leaf: norm1 of the site, on the merged rows (B, N - r, C); unmerged chain: norm1 as it is."""
    if plan.r is None:
        if x.device.type == "cpu":
            return torch.nn.functional.layer_norm(x, layernorm.normalized_shape, layernorm.weight, layernorm.bias, layernorm.eps)
        from . import ops
        return ops.layer_norm(x, layernorm.weight, layernorm.bias, layernorm.eps)
    from . import ops
    return ops.tome_merge_norm(x, layernorm.weight, layernorm.bias, layernorm.eps, plan.grid, plan.r, plan.assign, plan.kept, plan.off, plan.step)


def tome_unmerge_wrapper(y: torch.Tensor, x: torch.Tensor, plan: Plan, emit_stats: bool = False):
    """fx leaf: the residual add behind to_out, every token reading the row it was merged into.  `emit_stats`: also the LayerNorm
    partials of the output rows, for a following `ln_linear_wrapper`; the result is then the pair (out, stats)."""
    if plan.r is not None:
        from . import ops
        return ops.tome_unmerge_add(x, y, plan.where, emit_stats=emit_stats)
    out = x + y
    if not emit_stats:
        return out
    from . import ops
    f = out.float()
    return out, ops.RowStats(torch.stack([f.sum(-1), (f * f).sum(-1)], dim=-1).reshape(-1, 1, 2).contiguous(), 1)


for _name in ("tome_plan_wrapper", "tome_merge_wrapper", "tome_unmerge_wrapper"):
    torch.fx.wrap(_name)


def state_of(module, what: str) -> ToMe:
    """The ToMe state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "tome", ToMe, what, "token-merging self-attention sites", 'tome_layers=("down_blocks.1|up_blocks.1",)')
