"""The FreeU tests' own statement of the method (checker only; shares no code with stabletriton_amd/freeu.py).

`fourier_filter` is the published filter (diffusers `fourier_filter(x, threshold=1, scale)`), `backbone` the two
backbone rules, `hooked` the independent eager route: forward_pre_hooks on `up_blocks[i].resnets[j]` (i = 0, 1) that
split the concatenated input at the running activation's width, apply the formulas and concatenate again.
"""
import contextlib

import torch

SDXL_VALUES = dict(s1=0.9, s2=0.2, b1=1.3, b2=1.4)      # the values the FreeU authors give for SDXL


def fourier_filter(x: torch.Tensor, scale: float) -> torch.Tensor:
    H, W = x.shape[-2:]
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    f[..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] *= scale
    return torch.fft.ifftn(torch.fft.ifftshift(f, dim=(-2, -1)), dim=(-2, -1)).real


def backbone(h: torch.Tensor, b: float, version: int) -> torch.Tensor:
    half = h.shape[1] // 2
    if version == 1:
        return torch.cat([h[:, :half] * b, h[:, half:]], dim=1)
    mu = h.mean(1, keepdim=True)
    n = mu.shape[0]
    lo = mu.view(n, -1).min(dim=1).values.view(n, 1, 1, 1)
    hi = mu.view(n, -1).max(dim=1).values.view(n, 1, 1, 1)
    hat = torch.zeros_like(mu)
    ok = (hi > lo).expand_as(mu)
    hat[ok] = ((mu - lo) / (hi - lo))[ok]                  # (a constant map divides by zero in the original: 0 here, as documented)
    return torch.cat([h[:, :half] * ((b - 1.0) * hat + 1.0), h[:, half:]], dim=1)


def site(h, skip, b, s, version):
    """(h', skip') in float64 whatever comes in."""
    return backbone(h.double(), b, version), fourier_filter(skip.double(), s)


def running_widths(unet):
    """{(stage, resnet): channels of the running activation entering that decoder resnet} for stages 0 and 1."""
    w = unet.spec.widths
    n = len(w)
    out = {}
    for i in (0, 1):
        lvl = n - 1 - i
        for j in range(len(unet.up_blocks[i].resnets)):
            out[(i, j)] = (w[-1] if i == 0 else w[lvl + 1]) if j == 0 else w[lvl]
    return out


@contextlib.contextmanager
def hooked(unet, s1, s2, b1, b2, version=1):
    """The eager `unet` (stabletriton_amd.unet.UNet2DConditionModel, any float dtype) with FreeU applied by hooks."""
    handles = []
    for (i, j), ch in running_widths(unet).items():
        b, s = (b1, s1) if i == 0 else (b2, s2)

        def pre(module, args, ch=ch, b=b, s=s):
            x, temb = args
            h2, r2 = site(x[:, :ch], x[:, ch:], b, s, version)
            return torch.cat([h2, r2], dim=1).to(x.dtype), temb

        handles.append(unet.up_blocks[i].resnets[j].register_forward_pre_hook(pre))
    try:
        yield unet
    finally:
        for h in handles:
            h.remove()
