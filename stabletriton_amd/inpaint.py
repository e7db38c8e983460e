"""Masked inpainting: keep part of a latent fixed while the rest is denoised.  The mask, the threshold table of the differential
mode, and the one blend that runs behind every sampler step.

After step i the sampler has moved the whole latent to noise level sigma[i + 1].  The blend then puts the pixels to keep back onto
the known image at that same noise level,

    known  = init + sigma[i + 1] * noise            (noise: the trajectory's own unit start noise)
    latent = known + w * (latent - known)           (w = 1: untouched; w = 0: known, exactly)

and writes the next UNet input (latent * in_scale[i + 1]) for every row block of the UNet batch.  sigma[n] = 0, so behind the last
step a kept pixel is `init` bit for bit.  Mask values: 1 = repaint, 0 = keep, at latent resolution.

Three forms of w:
  binary mask   w = mask in {0, 1}: diffusers' StableDiffusionXLInpaintPipeline post-step blend for a four-channel UNet
                ((1 - mask) * init_latents_proper + mask * latents), with `init_latents_proper` the init latent re-noised by
                `scheduler.add_noise` with the trajectory's start noise to the next timestep.
  soft mask     w = mask in [0, 1]: the same line with a fractional mask.
  differential  w = (mask > thr[i]): Differential Diffusion (Levin and Fried), restated from memory: `mask` is a change map, a
                pixel of value m stays frozen after step i while m <= thr[i], and with `differential_thresholds`
                (thr[i] = 1 - (i + 1) / n) it is free for roughly the last m * n steps; m == 0 is kept to the end.

The blend runs behind the step, on the fp32 latent, so the sampler's update, the guidance and rescale arithmetic and the
stochastic samplers' noise are what they are without a mask.  The DPM-Solver++ history (the previous step's prediction of the clean
latent) is left alone, as diffusers leaves its `model_outputs`.  Parity with either published pipeline is unpinned - no reference
output has been compared.

`DenoiseLoop(inpaint=True)` / `set_inpaint` (pipeline.py) run the blend inside the captured loop; `blend` is here for callers with
their own loop (a UI's inpainting around the hooked UNet).  Device tensors go to the HIP kernel (ops.inpaint_blend,
csrc/inpaint.hip); CPU tensors take a torch restatement of the same arithmetic (fp32 fused multiply-adds, one rounding to the input's
type).
"""
from __future__ import annotations

from typing import Optional

import torch


def prepare_mask(mask, batch: int, latent_hw) -> torch.Tensor:
    """A checked fp32 CPU mask (1 | B, lh, lw) from (lh, lw), (1 | B, lh, lw) or (1 | B, 1, lh, lw); values finite and in [0, 1],
    1 = repaint, 0 = keep.  The mask is taken AT LATENT RESOLUTION and never resampled: a mask drawn at pixel resolution is the
    caller's to reduce (how - nearest, area, a dilation first - changes the seam, and is the caller's choice)."""
    lh, lw = int(latent_hw[0]), int(latent_hw[1])
    m = torch.as_tensor(mask).detach().to("cpu", torch.float32)
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3 or m.shape[0] not in (1, int(batch)) or tuple(m.shape[1:]) != (lh, lw):
        raise ValueError(f"inpaint mask: takes ({lh}, {lw}), (1 | {batch}, {lh}, {lw}) or (1 | {batch}, 1, {lh}, {lw}) at latent resolution "
                         f"(masks are not resampled), got {tuple(torch.as_tensor(mask).shape)}")
    if not bool(torch.isfinite(m).all()):
        raise ValueError("inpaint mask: values must be finite")
    if bool((m < 0).any()) or bool((m > 1).any()):
        raise ValueError("inpaint mask: values must lie in [0, 1] (1 = repaint, 0 = keep)")
    return m.contiguous()


def differential_thresholds(n_steps: int) -> torch.Tensor:
    """fp32 thr[i] = 1 - (i + 1) / n_steps (computed in float64, rounded once): the last entry is 0, so only m == 0 is kept to the
    end."""
    n = int(n_steps)
    if n < 1:
        raise ValueError(f"differential_thresholds: n_steps must be at least 1, got {n_steps}")
    i = torch.arange(1, n + 1, dtype=torch.float64)
    return (1.0 - i / n).float()


def _fma(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fp32 fma(a, b, c): the product of two fp32 values is exact in float64, so one float64 add rounded to fp32 is the fused result
    (but for a double rounding 2^-29 below the fp32 ulp)."""
    return (a.double() * b.double() + c.double()).float()


def blend(latent: torch.Tensor, x_step: torch.Tensor, init: torch.Tensor, noise: torch.Tensor, mask: torch.Tensor,
          sigma_next: torch.Tensor, in_scale: torch.Tensor, step, thr: Optional[torch.Tensor] = None) -> None:
    """The blend behind sampler step `step`, IN PLACE on `latent` (B, C, H, W) fp32 and `x_step` (blocks * B, C, H, W), the next
    UNet input of every row block; `init`, `noise` (B, C, H, W) fp32; `mask` fp32 (1 | B, H, W) (prepare_mask); `sigma_next`
    (tables.sigmas[1:]), `in_scale` and `thr` fp32 tables of n_steps values; `step` an int32 tensor of one entry (or, on the CPU, an
    int).  With `thr` the mask is a change map and w = (mask > thr[step]); a NaN entry of `thr` means "no threshold at this step".
    Pixels at w == 1 are not written.  Device tensors: one HIP launch, all tensors dense channels_last."""
    if latent.device.type != "cpu":
        from . import ops
        ops.inpaint_blend(latent, x_step, init, noise, mask, sigma_next, in_scale, step, thr)
        return
    B = latent.shape[0]
    n = sigma_next.numel()
    if x_step.shape[0] < B or x_step.shape[0] % B or tuple(x_step.shape[1:]) != tuple(latent.shape[1:]):
        raise ValueError(f"inpaint.blend: x_step must be (blocks * {B}, ...) of the latent's shape {tuple(latent.shape)}, got {tuple(x_step.shape)}")
    if mask.dim() != 3 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != tuple(latent.shape[2:]):
        raise ValueError(f"inpaint.blend: mask must be (1 | {B}, H, W) = {tuple(latent.shape[2:])}, got {tuple(mask.shape)}")
    i = min(max(int(step.item()) if torch.is_tensor(step) else int(step), 0), n - 1)
    s = sigma_next[i].float()
    sc = in_scale[min(i + 1, n - 1)].float()
    m = mask.float()
    t = None if thr is None else thr[i].float()
    w = m if (t is None or bool(torch.isnan(t))) else (m > t).float()
    w = torch.where(w < 1, w.clamp_min(0.0), torch.ones_like(w))[:, None]        # (1 | B, 1, H, W); NaN compares false: repaint
    known = _fma(s.expand_as(noise), noise.float(), init.float())
    soft = _fma(w.expand_as(known), latent - known, known)
    v = torch.where(w == 0, known, soft)
    keep = (w == 1).expand_as(latent)
    latent.copy_(torch.where(keep, latent, v))
    out = (v * sc).to(x_step.dtype)
    for r in range(x_step.shape[0] // B):
        rows = x_step[r * B:(r + 1) * B]
        rows.copy_(torch.where(keep, rows, out))
