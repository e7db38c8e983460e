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

import contextlib
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from .state import RowBound, latent_size, require_state


def scale_table(n_steps: int, scale: float = 1.0, factor: float = 1.0) -> torch.Tensor:
    """diffusers' `adapter_conditioning_scale` / `adapter_conditioning_factor` as a table: `scale` for the steps
    i < int(n_steps * factor), 0 for the rest (n_steps fp32 values, on the host)."""
    scale, factor = float(scale), float(factor)
    if not (scale == scale and abs(scale) != float("inf")):
        raise ValueError(f"t2i_adapter: scale must be finite, got {scale!r}")
    if not 0.0 <= factor <= 1.0:
        raise ValueError(f"t2i_adapter: factor must lie in [0, 1] (the share of the steps the adapter acts on), got {factor!r}")
    on = int(n_steps * factor)
    return torch.tensor([scale if i < on else 0.0 for i in range(n_steps)], dtype=torch.float32)


class T2IAdapterState(RowBound, nn.Module):
    """State of one compiled module: the sites (name, channels, latent halvings, ComfyUI input-block index) and their buffers."""
    label = "t2i_adapter"

    def __init__(self, sites: Sequence[Tuple[str, int, int, Optional[int]]], dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.sites = tuple(s[0] for s in sites)
        self.channels = tuple(int(s[1]) for s in sites)
        self.levels = tuple(int(s[2]) for s in sites)
        self.input_blocks = tuple(s[3] for s in sites)     # index among ComfyUI's input blocks; None: the middle block
        self.dtype = dtype                                 # the dtype `bind` allocates in when it is not told another
        # (rows, site, h, w) -> (feature rows, C, h, w) channels_last, never reallocated.  Plain dicts under names torch does not
        # know, as in regions.Regions: not registered buffers, so .to(dtype) / state_dict() leave them alone at their addresses
        self._features: Dict[Tuple[int, int, int, int], torch.Tensor] = {}
        self._tables: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}      # device -> (scale table of one entry, step 0)
        self._use = None                                   # (step, table) of the caller inside `using`
        self.host_scale = 0.0                              # the state's own scale as a Python float (the CPU route computes with it)

    # ---- geometry --------------------------------------------------------------------------------
    def site_shapes(self, latent_hw):
        """(C, h, w) of every site's feature map at this latent size: each halving is the UNet's stride-2 convolution, ceil(n / 2)
        (the adapter's AvgPool2d(ceil_mode=True) and PixelUnshuffle of a multiple of 16 pixels give the same sizes)."""
        lh, lw = latent_size(latent_hw)
        out = []
        for c, l in zip(self.channels, self.levels):
            h, w = lh, lw
            for _ in range(l):
                h, w = (h + 1) // 2, (w + 1) // 2
            out.append((c, h, w))
        return out

    # ---- buffers ---------------------------------------------------------------------------------
    def bind(self, rows: int, latent_hw, device, dtype: Optional[torch.dtype] = None, feature_rows: Optional[int] = None) -> None:
        """Allocate the zeroed feature buffers of a UNet batch of `rows` rows at this latent size, and the scale table (0 = off).
        `feature_rows` (a divisor of rows; default rows): how many feature rows the buffers hold - the row blocks [negative |
        positive | perturbed] of a guided call share one copy of `batch` rows.  Outside any capture; a buffer that exists is kept
        (its address is what captured graphs read), so binding twice is free."""
        rows = int(rows)
        f_rows = rows if feature_rows is None else int(feature_rows)
        lh, lw = latent_size(latent_hw)
        if rows < 1 or lh < 1 or lw < 1 or f_rows < 1 or rows % f_rows:      # (not _parse_bind: this text names feature_rows too)
            raise ValueError(f"t2i_adapter.bind: rows {rows}, latent {lh} x {lw}, feature_rows {f_rows} (a divisor of rows)")
        device = torch.device(device)
        dtype = dtype or self.dtype or torch.float32
        if device not in self._tables:
            self._refuse_capture(device)
            self._tables[device] = (torch.full((1,), self.host_scale, dtype=torch.float32, device=device),
                                    torch.zeros(1, dtype=torch.int32, device=device))
        for k, (c, h, w) in enumerate(self.site_shapes((lh, lw))):
            buf = self._features.get((rows, k, h, w))
            if buf is None:
                self._refuse_capture(device)
                self._features[(rows, k, h, w)] = torch.zeros((f_rows, c, h, w), dtype=dtype, device=device).contiguous(
                    memory_format=torch.channels_last)
            elif buf.device != device or buf.dtype != dtype or buf.shape[0] != f_rows:
                raise ValueError(f"t2i_adapter.bind: the buffers of {rows} rows at site {self.sites[k]} are {tuple(buf.shape)} {buf.dtype} on "
                                 f"{buf.device}; asked for {f_rows} feature rows of {dtype} on {device}")

    def bound_rows(self):
        return sorted({key[0] for key in self._features})

    def features_for(self, rows: int, k: int, h: int, w: int) -> torch.Tensor:
        buf = self._features.get((int(rows), int(k), int(h), int(w)))
        if buf is None:
            raise ValueError(f"t2i_adapter: no feature buffer for site {self.sites[k]} at {rows} rows x {h} x {w} (bound: "
                             f"{sorted(self._features)}); call gm.t2i_adapter.bind(rows, latent_hw, device) before the first evaluation")
        return buf

    def _own(self, device=None):
        if not self._tables:
            raise ValueError("t2i_adapter: nothing is bound; call bind(rows, latent_hw, device) first")
        if device is None:
            if len(self._tables) != 1:
                raise ValueError(f"t2i_adapter: bound on {sorted(str(d) for d in self._tables)}: one state serves one device")
            return next(iter(self._tables.values()))
        return self._tables[torch.device(device)]

    # ---- values ----------------------------------------------------------------------------------
    def check_features(self, features, rows: int, what: str):
        """The (buffer, tensor) pairs `set` would write, validated; nothing is written."""
        n = len(self.sites)
        if not isinstance(features, (list, tuple)) or len(features) != n:
            got = len(features) if isinstance(features, (list, tuple)) else type(features).__name__
            raise ValueError(f"{what}: takes {n} feature maps, one per site {self.sites}, got {got}")
        pairs = []
        for k, f in enumerate(features):
            if not torch.is_tensor(f) or f.dim() != 4 or f.shape[1] != self.channels[k]:
                shape = tuple(f.shape) if torch.is_tensor(f) else type(f).__name__
                raise ValueError(f"{what}: feature {k} (site {self.sites[k]}) must be (rows or 1, {self.channels[k]}, h, w), got {shape}")
            buf = self._features.get((rows, k, int(f.shape[2]), int(f.shape[3])))
            if buf is None:
                sizes = sorted(key[2:] for key in self._features if key[0] == rows and key[1] == k)
                raise ValueError(f"{what}: feature {k} (site {self.sites[k]}) is {tuple(f.shape[2:])}; the buffers bound for {rows} rows "
                                 f"have the sizes {sizes} there (the adapter image is 8 x the latent size)")
            if f.shape[0] not in (1, buf.shape[0]):
                raise ValueError(f"{what}: feature {k} (site {self.sites[k]}) has {f.shape[0]} rows; the buffers hold {buf.shape[0]} "
                                 "(or 1 for every row)")
            pairs.append((buf, f))
        return pairs

    def set(self, features, scale: Optional[float] = 1.0, rows: Optional[int] = None) -> None:
        """Copy one feature map per site into the buffers of `rows` in place, and (scale not None) set the state's own scale."""
        rows = self._rows(rows, "t2i_adapter.set")
        pairs = self.check_features(features, rows, "t2i_adapter.set")
        for buf, f in pairs:          # (nothing is written unless every site validated)
            buf.copy_(f.detach().to(buf.dtype).expand(buf.shape))
        if scale is not None:
            self.set_scale(scale)

    def set_scale(self, scale: float) -> None:
        """The state's own scale (what the sites read outside `using`): an in-place write on every bound device."""
        scale_table(1, scale)            # (validates)
        for table, _ in self._tables.values():
            table.fill_(float(scale))
        self.host_scale = float(scale)

    def clear(self) -> None:
        """Back to "off": scale 0 (the feature buffers keep their contents; nobody reads them)."""
        for table, _ in self._tables.values():
            table.zero_()
        self.host_scale = 0.0

    @contextlib.contextmanager
    def using(self, step: torch.Tensor, table: torch.Tensor):
        """Around the caller's own UNet calls: the sites read `table[*step]` (an fp32 device table, an int32 device counter, both by
        address) instead of the state's own scale."""
        if step.dtype != torch.int32 or step.numel() != 1 or table.dtype != torch.float32 or table.dim() != 1:
            raise ValueError("t2i_adapter.using: step is an int32 tensor of one entry, table a 1-D fp32 tensor")
        prev, self._use = self._use, (step, table)
        try:
            yield self
        finally:
            self._use = prev

    def current(self, device):
        """(step, table) the sites of a call on `device` read."""
        if self._use is not None:
            return self._use
        table, step = self._own(device)
        return step, table

    def extra_repr(self) -> str:
        return f"sites={self.sites}, channels={self.channels}, levels={self.levels}, bound={sorted(self._features)}"


def t2i_site(x: torch.Tensor, state: T2IAdapterState, k: int, src_stats=None, emit_colstats: bool = False):
    """fx leaf: x + s * f_k at site k, s = table[*step] of `state.current`.  Device tensors: IN PLACE on x (every reader of the value
    was rewired to this node), and the GroupNorm partials `src_stats` x's producer emitted are rewritten for the new values;
    with emit_colstats the result is the pair (x, statistics or None).  CPU tensors: out of place in torch."""
    rows, _, h, w = x.shape
    f = state.features_for(rows, k, h, w)
    step, table = state.current(x.device)
    if x.device.type == "cpu":
        i = min(max(int(step.reshape(-1)[0]), 0), table.numel() - 1)      # the kernel's clamp: a step past the table reads its last entry
        s = state.host_scale if state._use is None else float(table[i])
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
    if not isinstance(control, dict):
        raise NotImplementedError(f"control must be a dict of lists (input / middle), got {type(control).__name__}")
    extra = sorted(k for k in control if k not in ("input", "middle", "output"))
    if extra:
        raise NotImplementedError(f"control entries {extra} are not supported by the compiled UNet (input / middle of a T2I adapter are)")
    if control.get("output"):
        raise NotImplementedError('control["output"] (ControlNet residuals on the decoder\'s skip connections) is not supported by the '
                                  "compiled UNet: only T2I-Adapter residuals (input / middle) are")
    out = [None] * len(state.sites)
    inputs = list(control.get("input") or [])
    for j, entry in enumerate(reversed(inputs)):            # entry j from the end goes to input block j
        if entry is None:
            continue
        if j not in state.input_blocks:
            raise NotImplementedError(f'control["input"] carries a residual for input block {j}; the compiled UNet has T2I-Adapter sites '
                                      f"at the input blocks {[b for b in state.input_blocks if b is not None]} only (ControlNet is not supported)")
        out[state.input_blocks.index(j)] = entry
    middle = list(control.get("middle") or [])
    if any(e is not None for e in middle[:-1]):
        raise NotImplementedError('control["middle"] carries more than one residual; the middle block takes the last entry')
    if middle and middle[-1] is not None:
        if None not in state.input_blocks:
            raise NotImplementedError("this UNet has no site behind its middle block")
        out[state.input_blocks.index(None)] = middle[-1]
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
