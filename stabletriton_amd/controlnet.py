"""ControlNet (Zhang et al., "Adding Conditional Control to Text-to-Image Diffusion Models") with the compiled UNet: a second
network per step whose outputs are added to the UNet's skip connections and to the output of its middle block.

What differs from a T2I-Adapter (t2i_adapter.py): the residuals are new every step; there is one per skip tensor plus the middle
one (ten on SDXL-base, thirteen on the refiner's four levels); and a skip residual is seen by the DECODER only - the encoder layer
that also reads the skip tensor sees the unmodified value (diffusers adds `down_block_additional_residuals` to the collected skips
after the encoder has run).  So when the middle block has finished, every encoder reader of every skip tensor has run, and ONE
launch behind the middle block adds all residuals in place and rewrites the producers' GroupNorm partials
(ops.residual_add_grouped, csrc/t2i_adapter.hip); optimizers/insert_controlnet.py places that leaf and rewires the decoder's
concatenations - and through them norm1, the 1x1 shortcut and FreeU - to its outputs.

`ControlNetState` is the state of one compiled module (`gm.controlnet`): per bound row count and latent size one zeroed residual
buffer per site, an fp32 row of per-site weights, a one-entry scale table and a step counter, all read by ADDRESS by the kernel, so
`set` / `set_scale` / `set_site_weights` / `clear` are in-place writes a captured graph picks up.  A caller with per-step scales and
its own residuals (the denoise loop: the branch's outputs of this very step) lends them with `using(step, table, residuals=...)`.
Site k runs under s_k = scale * weight_k; scale 0 - the state after `bind` and `clear` - writes nothing: the bits of the module
compiled without sites.

`controlnet_sites` is the fx leaf: HIP IN PLACE for device tensors, `x + s_k * r_k` out of place in torch for CPU tensors, so that
a traced CPU module can carry the pass on its own.

`ControlNetXL` is the branch network, an eager nn.Module built from unet.py's blocks under diffusers' `ControlNetModel` key
spelling, restated from memory (diffusers is not a dependency) - parity with a published checkpoint unpinned.
`optimize_model(ControlNetXL(...), cuda_graph=False)` is the compiled branch.
"""
from __future__ import annotations

import contextlib
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

from .state import ResidualSites, comfy_control, finite_scale, require_state
from .unet import SDXL_BASE, MidStage, SinusoidalProj, Stage, TimestepMLP, UNetSpec


def scale_table(n_steps: int, scale: float = 1.0, start: float = 0.0, end: float = 1.0) -> torch.Tensor:
    """diffusers' `controlnet_conditioning_scale` / `control_guidance_start` / `control_guidance_end` as a table: `scale` for the
    steps int(n_steps * start) <= i < int(n_steps * end), 0 for the rest (n_steps fp32 values, on the host)."""
    scale, start, end = finite_scale("controlnet", scale), float(start), float(end)
    if not 0.0 <= start <= end <= 1.0:
        raise ValueError(f"controlnet: 0 <= start <= end <= 1 (the share of the steps the control acts on), got start={start!r} end={end!r}")
    lo, hi = int(n_steps * start), int(n_steps * end)
    return torch.tensor([scale if lo <= i < hi else 0.0 for i in range(n_steps)], dtype=torch.float32)


class ControlNetState(ResidualSites):
    """State of one compiled module: the sites (name, channels, latent halvings) - the skip tensors in encoder order, the middle
    block's output last - and their buffers."""
    label = "controlnet"

    def __init__(self, sites: Sequence[Tuple[str, int, int]], dtype: Optional[torch.dtype] = None):
        super().__init__(sites, dtype)
        self.host_weights = [1.0] * len(self.sites)
        self._lent = None                                  # the residuals of the caller inside `using(..., residuals=)`

    def set_site_weights(self, weights: Optional[Sequence[float]] = None) -> None:
        """One factor per site on top of the scale (the skip tensors in encoder order, the middle block's last); None: all 1.  A site
        at weight 0 is skipped.  An in-place write."""
        n = len(self.sites)
        vals = [1.0] * n if weights is None else [float(v) for v in weights]
        if len(vals) != n or any(not (v == v and abs(v) != float("inf")) for v in vals):
            raise ValueError(f"controlnet.set_site_weights: takes {n} finite values, one per site, got {vals!r}")
        for own in self._tables.values():
            own.weights.copy_(torch.tensor(vals, dtype=torch.float32))
        self.host_weights = vals

    @contextlib.contextmanager
    def using(self, step: torch.Tensor, table: torch.Tensor, residuals=None):
        """`ResidualSites.using`, and - with `residuals`, one tensor per site - the sites read those tensors INSTEAD of the state's
        buffers: no copies, a capture records their addresses."""
        with super().using(step, table):
            if residuals is not None and (not isinstance(residuals, (list, tuple)) or len(residuals) != len(self.sites)):
                raise ValueError(f"controlnet.using: residuals are {len(self.sites)} tensors, one per site (the middle block's last)")
            prev, self._lent = self._lent, None if residuals is None else list(residuals)
            try:
                yield self
            finally:
                self._lent = prev

    def residuals_for(self, xs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """The residuals the sites of a call with the activations `xs` read: the lent ones - each (rows or a divisor of rows, C_k,
        h_k, w_k) of its activation, validated here -, or the buffers bound for that size."""
        if self._lent is None:
            return [self.buffer_for(x.shape[0], k, x.shape[2], x.shape[3]) for k, x in enumerate(xs)]
        self._check_list(self._lent, "controlnet.using")
        for k, (r, x) in enumerate(zip(self._lent, xs)):
            if tuple(r.shape[1:]) != tuple(x.shape[1:]) or r.shape[0] < 1 or x.shape[0] % r.shape[0]:
                raise ValueError(f"controlnet.using: residual {k} (site {self.sites[k]}) is {tuple(r.shape)}; the activation there is "
                                 f"{tuple(x.shape)}")
        return self._lent


def controlnet_sites(mid: torch.Tensor, skips, state: ControlNetState, src_stats=None):
    """fx leaf behind the middle block: site k of `skips + [mid]` becomes x_k + s_k * r_k, s_k = table[*step] * weight_k of
    `state.current`.  Returns the flat tuple (values of the n sites, then statistics of the n sites or None): device tensors are
    written IN PLACE by one launch (the decoder's readers were rewired to this node; the encoder's readers ran before it) that also
    rewrites the GroupNorm partials `src_stats[k]` the producer of x_k emitted; CPU tensors are computed out of place in torch."""
    xs = list(skips) + [mid]
    n = len(xs)
    src_stats = [None] * n if src_stats is None else list(src_stats)
    rs = state.residuals_for(xs)
    step, table, weights = state.current(mid.device)
    if mid.device.type == "cpu":
        s = state.cpu_scale(step, table)
        out = []
        for x, r, w in zip(xs, rs, state.host_weights):
            sk = s * w
            out.append(x if sk == 0.0 else x + sk * r.to(x.dtype).repeat(x.shape[0] // r.shape[0], 1, 1, 1))
        return tuple(out) + (None,) * n
    for k, (x, r) in enumerate(zip(xs, rs)):
        if r.dtype != x.dtype or r.device != x.device:
            raise ValueError(f"controlnet: the residual of site {state.sites[k]} is {r.dtype} on {r.device}, the activation is "
                             f"{x.dtype} on {x.device}: bind(rows, latent_hw, device, dtype) with the UNet's own")
    from . import ops
    return tuple(xs) + tuple(ops.residual_add_grouped(xs, rs, table, step, src_stats, weights))


torch.fx.wrap("controlnet_sites")


def state_of(module, what: str) -> ControlNetState:
    """The ControlNet state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "controlnet", ControlNetState, what, "ControlNet sites", "controlnet=True")


def check_combination(controlnet, t2i_adapter, fp8) -> None:
    if controlnet and t2i_adapter:
        raise ValueError("controlnet=True cannot be combined with t2i_adapter=True: a T2I-Adapter site writes the skip tensors in the "
                         "encoder, a ControlNet site behind the middle block; one compiled module carries one of the two")
    if controlnet and fp8:
        raise ValueError("controlnet=True cannot be combined with fp8=True: the fp8 plan's e4m3 copies of a site's input would miss "
                         "the residual")


def comfy_residuals(state: ControlNetState, control: dict):
    """ComfyUI's `control` dict -> one entry per site (a tensor or None), or None when it carries nothing.  `control["output"]`
    holds the skip residuals: ComfyUI pops from the END while the decoder consumes its skips last-first, so entry i is skip i in
    encoder order; `control["middle"]` takes its last entry.  A non-empty `control["input"]` (T2I-Adapter residuals) raises."""
    inputs, output, middle = comfy_control(control, "output / middle", "a ControlNet")
    if any(e is not None for e in inputs):
        raise NotImplementedError('control["input"] (T2I-Adapter residuals inside the encoder) is not supported by a UNet compiled with '
                                  "controlnet=True: only ControlNet residuals (output / middle) are")
    n = len(state.sites)
    if output and len(output) != n - 1:      # (ComfyUI pops from the end: a shorter list would belong to the LAST skips; none is guessed)
        raise NotImplementedError(f'control["output"] carries {len(output)} residuals; this UNet has {n - 1} skip tensors and takes one '
                                  "entry (or None) for each")
    out = output + [None] * (n - 1 - len(output)) + [middle]
    return None if all(e is None for e in out) else out


# ---- the branch network (eager; optimize_model compiles it) --------------------------------------------------------------------
class ControlNetConditioningEmbedding(nn.Module):
    """Control image (B, 3, 8 lh, 8 lw) -> (B, widths[0], lh, lw): conv_in 3 -> 16, blocks 16 -> 16 -> 32 -> 32 -> 96 -> 96 -> 256 with
    stride 2 on every second one, conv_out 256 -> widths[0]; 3x3 convolutions with SiLU between."""

    def __init__(self, out_channels: int, in_channels: int = 3, block_out_channels: Sequence[int] = (16, 32, 96, 256)):
        super().__init__()
        c = tuple(block_out_channels)
        self.conv_in = nn.Conv2d(in_channels, c[0], 3, padding=1)
        blocks = []
        for i in range(len(c) - 1):
            blocks.append(nn.Conv2d(c[i], c[i], 3, padding=1))
            blocks.append(nn.Conv2d(c[i], c[i + 1], 3, padding=1, stride=2))
        self.blocks = nn.ModuleList(blocks)
        self.conv_out = nn.Conv2d(c[-1], out_channels, 3, padding=1)
        self.act = nn.SiLU()

    def forward(self, image):
        x = self.act(self.conv_in(image))
        for block in self.blocks:
            x = self.act(block(x))
        return self.conv_out(x)


class ControlNetXL(nn.Module):
    """The ControlNet of an SDXL-family UNet: the UNet's encoder and middle block (unet.py's own blocks; `widths` and
    `resnets_per_level` are the UNet's, `depths` may differ), the control image's embedding added behind conv_in, and one 1x1
    "zero convolution" per skip tensor and for the middle block.  State-dict keys as diffusers' `ControlNetModel` spells them:
    conv_in, time_embedding, add_embedding, down_blocks, mid_block, controlnet_cond_embedding.{conv_in, blocks.0..5, conv_out},
    controlnet_down_blocks.{k}, controlnet_mid_block.  Restated from memory of the diffusers layout - parity with a published
    checkpoint unpinned: no published checkpoint or diffusers run has been compared.

    forward(sample, timesteps, encoder_hidden_states, added_cond_kwargs, cond_embed) -> (list of skip residuals, mid residual)
    with x = conv_in(sample) + cond_embed; `embed_condition(image)` gives cond_embed, once per control image, off the hot path."""

    def __init__(self, spec: UNetSpec = SDXL_BASE):
        super().__init__()
        self.spec = spec
        w, n = spec.widths, len(spec.widths)
        self.conv_in = nn.Conv2d(spec.in_channels, w[0], 3, padding=1)
        self.time_proj = SinusoidalProj(spec.time_proj_dim)
        self.time_embedding = TimestepMLP(spec.time_proj_dim, spec.temb_dim)
        self.add_time_proj = SinusoidalProj(spec.add_time_proj_dim)
        self.add_embedding = TimestepMLP(spec.add_in_dim, spec.temb_dim)
        self.controlnet_cond_embedding = ControlNetConditioningEmbedding(w[0])
        skip_ch, downs, c_prev = [w[0]], [], w[0]
        for lvl in range(n):
            io = [(c_prev if j == 0 else w[lvl], w[lvl]) for j in range(spec.resnets_per_level)]
            downs.append(Stage(io, spec, spec.depths[lvl], down=lvl < n - 1))
            skip_ch += [w[lvl]] * spec.resnets_per_level + ([w[lvl]] if lvl < n - 1 else [])
            c_prev = w[lvl]
        self.down_blocks = nn.ModuleList(downs)
        self.mid_block = MidStage(w[-1], spec, spec.depths[-1] if spec.mid_depth is None else spec.mid_depth)
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(c, c, 1) for c in skip_ch])
        self.controlnet_mid_block = nn.Conv2d(w[-1], w[-1], 1)

    def embed_condition(self, image: torch.Tensor) -> torch.Tensor:
        if image.dim() != 4 or image.shape[-2] % 8 or image.shape[-1] % 8:
            raise ValueError(f"ControlNetXL: a (B, 3, H, W) control image with H and W multiples of 8 (8 x the latent) expected, got "
                             f"{tuple(image.shape)}")
        with torch.no_grad():
            return self.controlnet_cond_embedding(image)

    def forward(self, sample, timesteps, encoder_hidden_states, added_cond_kwargs, cond_embed):
        text_embeds = added_cond_kwargs.get("text_embeds")
        time_ids = added_cond_kwargs.get("time_ids")
        tid = self.add_time_proj(time_ids.flatten()).reshape((text_embeds.shape[0], -1))
        add = torch.concat([text_embeds, tid], dim=-1)
        timesteps = timesteps.expand(sample.shape[0])
        emb = self.time_embedding(self.time_proj(timesteps).to(dtype=sample.dtype))
        emb = emb + self.add_embedding(add.to(emb.dtype))
        x = self.conv_in(sample) + cond_embed
        skips = [x]
        for blk in self.down_blocks:
            x = blk.encode(x, emb, encoder_hidden_states, skips)
        x = self.mid_block(x, emb, encoder_hidden_states)
        down = [conv(s) for conv, s in zip(self.controlnet_down_blocks, skips)]
        return down, self.controlnet_mid_block(x)
