"""Regional prompts inside the compiled UNet: masked multi-prompt cross-attention (ComfyUI's conditioning masks / "attention
couple", the diffusers community regional-prompting pipeline).

The caller concatenates R text contexts of `seg_len` tokens along the token axis, `encoder_hidden_states (rows, R*seg_len, cross)`.
The hoisted context module projects K / V token by token, so they come out as R key/value segments.  At every cross-attention
(`attn2`) site of a UNet compiled with `regions=R` each segment gets its own softmax and the R results are combined per query
row (= per latent cell of that level) with fp32 weights:

    out[b,t,h,:] = sum_r  w[b,r,t] * softmax_s(scale * q[b,t,h] . k[b, r*L+s, h]) v[b, r*L+s, h]          (s over segment r)

The weights live in device buffers of the state module `gm.regions`, one (rows, R, T_l) per bound row count and attention level,
read by address: `set` / `clear` are in-place writes, a captured graph stays.  "Off" - the state after `bind` and `clear` - is
weight 1 on segment 0 and 0 elsewhere: the bits of the same module compiled without the pass on segment 0's prompt.

Mask to weights (`level_weights`): masks (R, lh, lw) or (batch, R, lh, lw), non-negative and finite, at latent resolution.  Level l
is l halvings of the latent: m_l = the area mean over every 2^l x 2^l cell, w = m_l / sum_r m_l where that sum is > 0 and one-hot on
segment 0 where it is 0, flattened row-major to T_l = (lh >> l) * (lw >> l).  Rows that are not positive (the negative block
under classifier-free guidance) keep one-hot on segment 0; PAG's perturbed block takes the positive weights.

`attention_regions_wrapper` is the fx leaf optimizers/insert_regions.py puts in place of `attention_wrapper` at the attn2 sites:
HIP (ops.attention_regions, csrc/attention_regions.hip) for device tensors, `reference` - a plain torch statement of the formula -
for CPU tensors, so that a traced CPU module can carry the pass on its own.
"""
from __future__ import annotations

import re
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .state import RowBound, require_state

MAX_REGIONS = 8            # st_attention_regions: segments per launch
MAX_SEG_LEN = 255          # ... and keys per segment (the text-context kernel's range)


def _as_batched(masks: torch.Tensor, R: int, what: str) -> torch.Tensor:
    if not torch.is_tensor(masks):
        masks = torch.as_tensor(masks)
    m = masks.detach().to("cpu", torch.float32)
    if m.dim() == 3:
        m = m.unsqueeze(0)
    if m.dim() != 4 or m.shape[1] != R:
        raise ValueError(f"{what}: masks must be (R, lh, lw) or (batch, R, lh, lw) with R = {R}, got {tuple(masks.shape)}")
    if not bool(torch.isfinite(m).all()) or bool((m < 0).any()):
        raise ValueError(f"{what}: masks must be finite and non-negative")
    return m


def level_weights(masks: torch.Tensor, level: int) -> torch.Tensor:
    """(R, lh, lw) or (batch, R, lh, lw) masks -> the (batch, R, T_l) float32 weights of attention level `level` (pure, on the host)."""
    R = masks.shape[-3]
    m = _as_batched(masks, R, "level_weights")
    cell = 1 << level
    lh, lw = m.shape[-2:]
    if lh % cell or lw % cell:
        raise ValueError(f"level_weights: a {lh} x {lw} mask does not divide into {cell} x {cell} cells (level {level})")
    if level:
        m = F.avg_pool2d(m, cell)
    total = m.sum(dim=1, keepdim=True)
    first = torch.zeros_like(m)
    first[:, 0] = 1.0
    w = torch.where(total > 0, m / total.clamp(min=torch.finfo(torch.float32).tiny), first)
    return w.flatten(2).contiguous()


def off_weights(rows: int, R: int, T: int) -> torch.Tensor:
    w = torch.zeros((rows, R, T), dtype=torch.float32)
    w[:, 0] = 1.0
    return w


def row_weights(masks: torch.Tensor, level: int, rows: int, positive_rows: Sequence[int]) -> torch.Tensor:
    """(rows, R, T_l): `level_weights` on the positive rows (the j-th of them takes mask j % batch of a per-batch mask), one-hot on
    segment 0 on every other row."""
    w = level_weights(masks, level)
    batch, R, T = w.shape
    pos = [int(r) for r in positive_rows]
    if any(r < 0 or r >= rows for r in pos) or len(set(pos)) != len(pos):
        raise ValueError(f"regions: positive_rows {pos} must be distinct rows in [0, {rows})")
    if len(pos) % batch:
        raise ValueError(f"regions: {len(pos)} positive rows do not divide into a per-batch mask of {batch} entries")
    out = off_weights(rows, R, T)
    for j, r in enumerate(pos):
        out[r] = w[j % batch]
    return out


class Regions(RowBound, nn.Module):
    """State of one compiled module: R, seg_len, the attn2 site paths, the attention levels, and the weight buffers."""
    label = "regions"

    def __init__(self, R: int, seg_len: int = 77, sites: Sequence[str] = (), levels: Optional[Sequence[int]] = None):
        super().__init__()
        if isinstance(R, bool) or not isinstance(R, int) or not 1 <= R <= MAX_REGIONS:
            raise ValueError(f"regions: R must be an integer in [1, {MAX_REGIONS}], got {R!r}")
        if isinstance(seg_len, bool) or not isinstance(seg_len, int) or not 1 <= seg_len <= MAX_SEG_LEN:
            raise ValueError(f"region_tokens: an integer in [1, {MAX_SEG_LEN}] expected, got {seg_len!r}")
        self.R, self.seg_len = R, seg_len
        self.sites = tuple(sites)
        # halvings of the latent at which a site runs, from the site paths (down_blocks.i -> i, ...); None: not spelled there,
        # bind() then covers every level the latent divides into
        self.levels = None if levels is None else tuple(sorted(set(int(l) for l in levels)))
        # (rows, T_l) -> (rows, R, T_l) fp32, never reallocated.  A plain dict under a name torch does not know: NOT registered
        # buffers, so state_dict() / buffers() of the compiled module do not see them and .to(dtype) / .half() leave them fp32
        # at their addresses (captured graphs read them in place)
        self._weights: Dict[Tuple[int, int], torch.Tensor] = {}

    # ---- buffers ---------------------------------------------------------------------------------
    def bind(self, rows: int, latent_hw, device) -> None:
        """Allocate the weight buffers of a UNet batch of `rows` rows at this latent size, initialised to "off".  Outside any
        capture; a buffer that exists is kept as it is (its address is what captured graphs read), so binding twice is free."""
        rows, lh, lw, device = self._parse_bind(rows, latent_hw, device)
        for l in self._levels_for(lh, lw):
            T = (lh >> l) * (lw >> l)
            buf = self._weights.get((rows, T))
            if buf is None:
                self._refuse_capture(device, "the weight buffers")
                self._weights[(rows, T)] = off_weights(rows, self.R, T).to(device)
            elif buf.device != device:
                raise ValueError(f"regions.bind: the buffers of {rows} rows live on {buf.device}, not {device}")

    def bound_rows(self):
        return sorted({r for r, _ in self._weights})

    def weights_for(self, rows: int, T: int) -> torch.Tensor:
        buf = self._weights.get((int(rows), int(T)))
        if buf is None:
            raise ValueError(f"regions: no weight buffer for a cross-attention of {rows} rows x {T} queries (bound: "
                             f"{sorted(self._weights)}); call gm.regions.bind(rows, latent_hw, device) before the first evaluation")
        return buf

    # ---- weights ---------------------------------------------------------------------------------
    def set(self, masks: torch.Tensor, positive_rows: Sequence[int], rows: Optional[int] = None) -> None:
        """Compute the level weights of `masks` on the host and copy them into the buffers of `rows` in place (no new capture)."""
        rows = self._rows(rows, "regions.set")
        m = _as_batched(masks, self.R, "regions.set")
        lh, lw = m.shape[-2:]
        new = []
        for l in self._levels_for(lh, lw):
            T = (lh >> l) * (lw >> l)
            if (rows, T) not in self._weights:
                raise ValueError(f"regions.set: masks of {lh} x {lw} do not match the latent size bound for {rows} rows "
                                 f"(buffers: {sorted(t for r, t in self._weights if r == rows)} queries)")
            new.append((self._weights[(rows, T)], row_weights(m, l, rows, positive_rows)))
        for buf, w in new:          # (nothing is written unless every level validated)
            buf.copy_(w)

    def clear(self, rows: Optional[int] = None) -> None:
        """Back to "off": weight 1 on segment 0, 0 elsewhere (every bound row count, or that of `rows`)."""
        for (r, T), buf in self._weights.items():
            if rows is None or r == int(rows):
                buf.copy_(off_weights(r, self.R, T))

    def extra_repr(self) -> str:
        return f"R={self.R}, seg_len={self.seg_len}, sites={len(self.sites)}, levels={self.levels}, bound={sorted(self._weights)}"


_STAGE = re.compile(r"(?:^|\.)(down_blocks|up_blocks)\.(\d+)\.|(?:^|\.)(mid_block)\.")


def site_levels(sites: Sequence[str], module_names: Sequence[str]):
    """Latent halvings of every site from diffusers' stage names: down_blocks.i -> i, mid_block -> n - 1, up_blocks.j -> n - 1 - j
    with n = the number of down_blocks; None when a path does not spell its stage."""
    n = 0
    for name in module_names:
        m = re.search(r"(?:^|\.)down_blocks\.(\d+)(?:\.|$)", name)
        if m:
            n = max(n, int(m.group(1)) + 1)
    levels = set()
    for s in sites:
        m = _STAGE.search(s + ".")
        if m is None or n == 0:
            return None
        if m.group(3):
            levels.add(n - 1)
        elif m.group(1) == "down_blocks":
            levels.add(int(m.group(2)))
        else:
            levels.add(n - 1 - int(m.group(2)))
    return None if any(l < 0 for l in levels) else sorted(levels)


def reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, weights: torch.Tensor, num_heads: int, sm_scale: float,
              seg_len: int) -> torch.Tensor:
    """Plain torch: the formula of the module docstring on (B, T, H*D) / (B, R*seg_len, H*D) projections, weights (B, R, T)."""
    from .pag import identity_attention_reference
    B, T, C = q.shape
    R = weights.shape[1]
    if weights.shape != (B, R, T) or k.shape[1] != R * seg_len or v.shape != k.shape:
        raise ValueError(f"regions.reference: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}, weights {tuple(weights.shape)}, "
                         f"seg_len {seg_len}")
    wide = torch.promote_types(q.dtype, torch.float32)
    acc = None
    for r in range(R):
        seg = slice(r * seg_len, (r + 1) * seg_len)
        a = identity_attention_reference(q, k[:, seg], v[:, seg], num_heads, sm_scale, 0).to(wide)
        term = weights[:, r].to(wide).unsqueeze(-1) * a
        acc = term if acc is None else acc + term
    return acc.to(q.dtype)


def attention_regions_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                              state: Regions) -> torch.Tensor:
    """fx leaf: attention_wrapper over the R key/value segments of k / v, combined with the state's weights for this (rows, T)."""
    if k.shape[1] != state.R * state.seg_len:
        raise ValueError(f"regions: this UNet was compiled with regions={state.R}, region_tokens={state.seg_len}: the text context must "
                         f"have {state.R * state.seg_len} tokens ({state.R} prompts concatenated), got {k.shape[1]}")
    w = state.weights_for(q.shape[0], q.shape[1])
    if q.device.type == "cpu":
        return reference(q, k, v, w, num_heads, sm_scale, state.seg_len)
    from . import ops
    if q.shape[-1] != num_heads * head_dim:
        raise ops.BackendError(f"attention_regions_wrapper: C={q.shape[-1]} != num_heads*head_dim={num_heads * head_dim}")
    return ops.attention_regions(q, k, v, w, num_heads, sm_scale, state.seg_len)


torch.fx.wrap("attention_regions_wrapper")


def state_of(module, what: str) -> Regions:
    """The regions state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "regions", Regions, what, "regional cross-attention sites", "regions=R")


def positive_rows(rows: int, chunks: int):
    """Rows of a UNet batch of `chunks` equal blocks that take the masks: every block but the first, [negative | positive | ...]
    (chunks 2: guidance; 3: guidance and PAG), or every row when chunks is 1 (no negative block in the call)."""
    if isinstance(chunks, bool) or not isinstance(chunks, int) or chunks < 1:
        raise ValueError(f"regions: chunks must be a positive integer (1: every row positive; 2, 3: the first block is the negative one), got {chunks!r}")
    if rows % chunks:
        raise ValueError(f"regions: a UNet batch of {rows} rows does not divide into {chunks} chunks")
    return list(range(rows // chunks if chunks > 1 else 0, rows))
