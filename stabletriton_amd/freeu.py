"""FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") inside the compiled UNet.

At the decoder concatenations of the first two decoder stages the running activation `h` gets half of its channels
rescaled and the skip tensor `r` gets its lowest spatial frequencies damped, before `cat([h, r], 1)`:

  r' = fourier_filter(r, threshold=1, scale=s)      X = fftshift(fftn(r)); X[H/2-1 : H/2+1, W/2-1 : W/2+1] *= s; real part back
  version 1 (diffusers `enable_freeu`)   h'[:, :C/2] = b * h[:, :C/2]
  version 2 (ComfyUI `FreeU_V2`)         h'[:, :C/2] = h[:, :C/2] * ((b - 1) * mu_hat + 1),  mu = mean over ALL channels,
                                         mu_hat = (mu - min) / (max - min) per sample over the H x W map

Stage 0 of the decoder (`up_blocks.0`) uses (b1, s1), stage 1 (b2, s2): diffusers' `resolution_idx` rule.  On SDXL-base
those are the six sites ComfyUI's channel rule (1280 / 640) selects too; for other topologies ComfyUI's rule can differ
from the stage rule used here, which is out of scope.

Where a sample's mean map is constant (max == min) the original divides by zero; here mu_hat = 0 there (the factor is 1).

`FreeU` is the parameter state of one compiled module (`gm.freeu`): an fp32 device row (b1, s1, b2, s2, version) the
kernels read by address, so `set` / `disable` are in-place writes a captured graph picks up.  It starts neutral
(b = s = 1: both tensors pass through bit for bit, still through the two launches).  `reference` is the plain torch
statement with torch.fft; `freeu_wrapper` is the fx leaf: HIP (ops.freeu, csrc/freeu.hip) for device tensors, `reference`
for CPU tensors so that a traced CPU module can carry the pass on its own.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .state import require_state

NEUTRAL = (1.0, 1.0, 1.0, 1.0, 1.0)       # (b1, s1, b2, s2, version)


def _check_sizes(h: int, w: int) -> None:
    if h < 2 or w < 2:
        raise ValueError(f"FreeU: a {h} x {w} map has no low-frequency box (the published filter's slice is empty for a side of 1)")


def lowpass_reference(x: torch.Tensor, scale: float) -> torch.Tensor:
    """diffusers' fourier_filter(x, threshold=1, scale) on the last two dimensions, in x's own precision (complex of it)."""
    H, W = x.shape[-2:]
    _check_sizes(H, W)
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(H, W, dtype=x.dtype, device=x.device)
    mask[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


def lowpass_closed_form(x: torch.Tensor, scale: float) -> torch.Tensor:
    """The same filter as seven moments per plane and a rank-7 update (what csrc/freeu.hip computes), in x's precision."""
    H, W = x.shape[-2:]
    _check_sizes(H, W)
    t = (2.0 * math.pi / H) * torch.arange(H, dtype=x.dtype, device=x.device)[:, None]
    p = (2.0 * math.pi / W) * torch.arange(W, dtype=x.dtype, device=x.device)[None, :]
    one = torch.ones(H, W, dtype=x.dtype, device=x.device)
    basis = torch.stack([one, torch.cos(t) * one, torch.sin(t) * one, torch.cos(p) * one, torch.sin(p) * one,
                         torch.cos(t + p), torch.sin(t + p)])                       # (7, H, W)
    m = torch.einsum("...hw,khw->...k", x, basis)
    return x + ((scale - 1.0) / (H * W)) * torch.einsum("...k,khw->...hw", m, basis)


def backbone_reference(h: torch.Tensor, b: float, version: int) -> torch.Tensor:
    half = h.shape[1] // 2
    out = h.clone()
    if version == 1:
        out[:, :half] = h[:, :half] * b
        return out
    mu = h.mean(dim=1, keepdim=True)
    lo = mu.amin(dim=(2, 3), keepdim=True)
    hi = mu.amax(dim=(2, 3), keepdim=True)
    span = hi - lo
    hat = torch.where(span > 0, (mu - lo) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(mu))
    out[:, :half] = h[:, :half] * ((b - 1.0) * hat + 1.0)
    return out


def reference(h: torch.Tensor, skip: torch.Tensor, b: float, s: float, version: int = 1):
    """(h', skip') of one site, plain torch with torch.fft; any float dtype (16-bit inputs are computed in fp32 and
    rounded once), CPU or device."""
    if version not in (1, 2):
        raise ValueError(f"FreeU: version {version!r} (1: diffusers, 2: ComfyUI FreeU_V2)")
    _check_sizes(*h.shape[-2:])
    wide = h.dtype if h.dtype in (torch.float32, torch.float64) else torch.float32
    hh, rr = h.to(wide), skip.to(wide)
    h2 = hh if b == 1.0 else backbone_reference(hh, float(b), version)
    r2 = rr if s == 1.0 else lowpass_reference(rr, float(s))
    return h2.to(h.dtype), r2.to(skip.dtype)


class FreeU(nn.Module):
    """Parameter state of one compiled module; `params` is what the kernels read."""

    def __init__(self, device=None):
        super().__init__()
        self.register_buffer("params", torch.tensor(NEUTRAL, dtype=torch.float32, device=device), persistent=False)
        self.host = NEUTRAL                      # the same row as Python floats (the CPU route computes with these)

    @staticmethod
    def validate(s1, s2, b1, b2, version=1):
        vals = {}
        for name, v in (("s1", s1), ("s2", s2), ("b1", b1), ("b2", b2)):
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"FreeU: {name} must be a number, got {v!r}") from None
            if not math.isfinite(f) or f <= 0.0:
                raise ValueError(f"FreeU: {name} = {v!r} must be finite and positive")
            vals[name] = f
        if isinstance(version, bool) or version not in (1, 2):
            raise ValueError(f"FreeU: version {version!r} (1: diffusers enable_freeu, 2: ComfyUI FreeU_V2)")
        return (vals["b1"], vals["s1"], vals["b2"], vals["s2"], float(int(version)))

    def set(self, s1: float, s2: float, b1: float, b2: float, version: int = 1) -> None:
        """diffusers' argument order.  An in-place write of the device row: captured graphs keep reading it."""
        row = self.validate(s1, s2, b1, b2, version)
        self.params.copy_(torch.tensor(row, dtype=torch.float32))
        self.host = row

    def disable(self) -> None:
        self.params.copy_(torch.tensor(NEUTRAL, dtype=torch.float32))
        self.host = NEUTRAL

    @property
    def enabled(self) -> bool:
        return self.host[:4] != NEUTRAL[:4]

    def extra_repr(self) -> str:
        b1, s1, b2, s2, v = self.host
        return f"s1={s1}, s2={s2}, b1={b1}, b2={b2}, version={int(v)}"


def freeu_wrapper(h: torch.Tensor, skip: torch.Tensor, state: FreeU, slot: int):
    """fx leaf: (h', skip', stats of h', stats of skip') of decoder site `slot` (0: b1, s1; 1: b2, s2)."""
    if h.device.type == "cpu":
        b, s = state.host[2 * slot], state.host[2 * slot + 1]
        h2, r2 = reference(h, skip, b, s, int(state.host[4]))
        return h2, r2, None, None
    from . import ops
    return ops.freeu(h, skip, state.params, slot)


torch.fx.wrap("freeu_wrapper")


def state_of(module, what: str) -> FreeU:
    """The FreeU state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "freeu", FreeU, what, "FreeU sites", "freeu=True")
