"""T2I-Adapter (Mou et al., "T2I-Adapter: Learning Adapters to Dig out More Controllable Ability for Text-to-Image Diffusion
Models") inside the compiled UNet: structural control (canny, depth, pose, sketch, lineart) as residual sites.

The adapter network runs ONCE per control image and gives one feature map per site; they are constant over the trajectory.  Per
denoise step the UNet adds `s * f_k` to its activation at four places (diffusers' `down_intrablock_additional_residuals` rule for
SDXL; ComfyUI's `control["input"]` / `["middle"]` entries of a T2I adapter land on the same places):

  site A   the output of `down_blocks.0.downsamplers.0`                        (320 channels, latent / 2)
  site B   the output of `down_blocks.1` after its last attention, before its downsampler      (640, latent / 2)
  site C   likewise for the last down block                                   (1280, latent / 4)
  site M   the output of `mid_block`                                          (1280, latent / 4)

Every reader of the value sees the sum: the skip connections carry the residual too, as in diffusers (whose `+=` writes into the
tensors already collected as skips).  optimizers/insert_t2i_adapter.py places the sites.

`T2IAdapterState` is the state of one compiled module (`gm.t2i_adapter`), after regions.Regions: static feature buffers per bound
row count and site size, and an fp32 scale table, all read by ADDRESS by the kernel (csrc/t2i_adapter.hip), so `set` / `set_scale` /
`clear` are in-place writes a captured graph picks up.  The scale of a step is `table[*step]`; a caller with per-step scales (the
denoise loop) hands its own table and step counter to the sites with `using(step, table)` around its UNet calls.  Scale 0 - the
state after `bind` and `clear` - is an early exit of the kernel that writes nothing: the bits of the module compiled without sites.

`t2i_site` is the fx leaf: HIP (ops.residual_add) IN PLACE for device tensors, `x + s * f` out of place in torch for CPU tensors, so
that a traced CPU module can carry the pass on its own.

`FullAdapterXL` is the adapter network itself, an eager nn.Module that is not on the hot path: the published TencentARC / diffusers
`full_adapter_xl` layout restated from memory (diffusers is not a dependency) - parity unpinned, as for SDXL_REFINER in unet.py.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import nn

from .state import ResidualSites, comfy_control, finite_scale, require_state


def scale_table(n_steps: int, scale: float = 1.0, factor: float = 1.0) -> torch.Tensor:
    """diffusers' `adapter_conditioning_scale` / `adapter_conditioning_factor` as a table: `scale` for the steps
    i < int(n_steps * factor), 0 for the rest (n_steps fp32 values, on the host)."""
    scale, factor = finite_scale("t2i_adapter", scale), float(factor)
    if not 0.0 <= factor <= 1.0:
        raise ValueError(f"t2i_adapter: factor must lie in [0, 1] (the share of the steps the adapter acts on), got {factor!r}")
    on = int(n_steps * factor)
    return torch.tensor([scale if i < on else 0.0 for i in range(n_steps)], dtype=torch.float32)


class T2IAdapterState(ResidualSites):
    """State of one compiled module: the sites (name, channels, latent halvings, ComfyUI input-block index) and their buffers."""
    label = "t2i_adapter"
    words = ("feature", "feature maps", "rows or 1")

    def __init__(self, sites: Sequence[Tuple[str, int, int, Optional[int]]], dtype: Optional[torch.dtype] = None):
        super().__init__(sites, dtype)
        self.input_blocks = tuple(s[3] for s in sites)     # index among ComfyUI's input blocks; None: the middle block

    def bind(self, rows: int, latent_hw, device, dtype: Optional[torch.dtype] = None, feature_rows: Optional[int] = None) -> None:
        """`ResidualSites.bind` with the buffers' rows under this state's name: the features are constant over the row blocks of a
        guided call, which share one copy of `feature_rows` = batch rows."""
        super().bind(rows, latent_hw, device, dtype, feature_rows)

    features_for = ResidualSites.buffer_for


def t2i_site(x: torch.Tensor, state: T2IAdapterState, k: int, src_stats=None, emit_colstats: bool = False):
    """fx leaf: x + s * f_k at site k, s = table[*step] of `state.current`.  Device tensors: IN PLACE on x (every reader of the value
    was rewired to this node), and the GroupNorm partials `src_stats` x's producer emitted are rewritten for the new values;
    with emit_colstats the result is the pair (x, statistics or None).  CPU tensors: out of place in torch."""
    rows, _, h, w = x.shape
    f = state.features_for(rows, k, h, w)
    step, table, _ = state.current(x.device)
    if x.device.type == "cpu":
        s = state.cpu_scale(step, table)
        out = x if s == 0.0 else x + s * f.to(x.dtype).repeat(rows // f.shape[0], 1, 1, 1)
        return (out, None) if emit_colstats else out
    if f.dtype != x.dtype or f.device != x.device:
        raise ValueError(f"t2i_adapter: the feature buffers of site {state.sites[k]} are {f.dtype} on {f.device}, the activation is "
                         f"{x.dtype} on {x.device}: bind(rows, latent_hw, device, dtype) with the UNet's own")
    from . import ops
    st = ops.residual_add(x, f, table, step, src_stats)
    return (x, st) if emit_colstats else x


torch.fx.wrap("t2i_site")


def state_of(module, what: str) -> T2IAdapterState:
    """The T2I-Adapter state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "t2i_adapter", T2IAdapterState, what, "T2I-Adapter sites", "t2i_adapter=True")


def check_combination(t2i_adapter, fp8) -> None:
    if t2i_adapter and fp8:
        raise ValueError("t2i_adapter=True cannot be combined with fp8=True: the fp8 plan's e4m3 copies of a site's input would miss "
                         "the residual")


def comfy_features(state: T2IAdapterState, control: dict):
    """ComfyUI's `control` dict -> one entry per site (a tensor or None).  `control["input"]` is consumed from the END, one entry per
    input block (ComfyUI's apply_control pops), `control["middle"]` likewise for the middle block; None entries are skipped.
    Non-None entries anywhere but on the sites, and a non-empty `control["output"]` (ControlNet's decoder residuals), raise."""
    inputs, output, middle = comfy_control(control, "input / middle", "a T2I adapter")
    if output:
        raise NotImplementedError('control["output"] (ControlNet residuals on the decoder\'s skip connections) is not supported by the '
                                  "compiled UNet: only T2I-Adapter residuals (input / middle) are")
    out = [None] * len(state.sites)
    for j, entry in enumerate(reversed(inputs)):            # entry j from the end goes to input block j
        if entry is None:
            continue
        if j not in state.input_blocks:
            raise NotImplementedError(f'control["input"] carries a residual for input block {j}; the compiled UNet has T2I-Adapter sites '
                                      f"at the input blocks {[b for b in state.input_blocks if b is not None]} only (ControlNet is not supported)")
        out[state.input_blocks.index(j)] = entry
    if middle is not None:
        if None not in state.input_blocks:
            raise NotImplementedError("this UNet has no site behind its middle block")
        out[state.input_blocks.index(None)] = middle
    return out


# ---- the adapter network (eager, once per control image) ------------------------------------------------------------------------
class AdapterResnetBlock(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.block1 = nn.Conv2d(channels, channels, 3, padding=1)
        self.act = nn.ReLU()
        self.block2 = nn.Conv2d(channels, channels, 1)

    def forward(self, x):
        return self.block2(self.act(self.block1(x))) + x


class AdapterBlock(nn.Module):
    def __init__(self, c_in: int, c_out: int, num_res_blocks: int, down: bool = False):
        super().__init__()
        self.downsample = nn.AvgPool2d(2, stride=2, ceil_mode=True) if down else None
        self.in_conv = nn.Conv2d(c_in, c_out, 1) if c_in != c_out else None
        self.resnets = nn.Sequential(*[AdapterResnetBlock(c_out) for _ in range(num_res_blocks)])

    def forward(self, x):
        if self.downsample is not None:
            x = self.downsample(x)
        if self.in_conv is not None:
            x = self.in_conv(x)
        return self.resnets(x)


class FullAdapterXL(nn.Module):
    """The `full_adapter_xl` network of the published SDXL T2I-Adapters: PixelUnshuffle(16) -> conv_in 3x3 -> four blocks of two
    resnets (block1 3x3 -> ReLU -> block2 1x1, plus skip); block 1 opens with a 1x1 in_conv, block 2 with
    AvgPool2d(2, ceil_mode=True) and an in_conv.  A control image (B, 3, 8 lh, 8 lw) gives the four feature maps of the sites at
    latent lh x lw.  State-dict keys: conv_in, body.{i}.in_conv, body.{i}.resnets.{j}.block1 / .block2 (the published files spell them
    under `adapter.`; `load_adapter_state_dict` takes both).  Restated from memory of the TencentARC / diffusers layout - parity
    unpinned: no published checkpoint or diffusers run has been compared."""

    def __init__(self, channels: Sequence[int] = (320, 640, 1280, 1280), in_channels: int = 3, num_res_blocks: int = 2,
                 downscale_factor: int = 16):
        super().__init__()
        if len(channels) != 4:
            raise ValueError(f"FullAdapterXL: four block widths expected, got {tuple(channels)}")
        self.channels = tuple(int(c) for c in channels)
        self.downscale_factor = downscale_factor
        self.unshuffle = nn.PixelUnshuffle(downscale_factor)
        self.conv_in = nn.Conv2d(in_channels * downscale_factor ** 2, self.channels[0], 3, padding=1)
        c = self.channels
        self.body = nn.ModuleList([AdapterBlock(c[0], c[0], num_res_blocks), AdapterBlock(c[0], c[1], num_res_blocks),
                                   AdapterBlock(c[1], c[2], num_res_blocks, down=True), AdapterBlock(c[2], c[3], num_res_blocks)])

    def forward(self, image: torch.Tensor):
        if image.dim() != 4 or image.shape[-2] % self.downscale_factor or image.shape[-1] % self.downscale_factor:
            raise ValueError(f"FullAdapterXL: a (B, C, H, W) image with H and W multiples of {self.downscale_factor} expected, got "
                             f"{tuple(image.shape)}")
        x = self.conv_in(self.unshuffle(image))
        features = []
        for block in self.body:
            x = block(x)
            features.append(x)
        return features

    def load_adapter_state_dict(self, state_dict, strict: bool = True):
        """load_state_dict that also takes the published spelling with a leading `adapter.` on every key."""
        sd = {(k[len("adapter."):] if k.startswith("adapter.") else k): v for k, v in state_dict.items()}
        return self.load_state_dict(sd, strict=strict)
