"""The SDXL VAE decoder as a plain eager nn.Module for `optimize_model`, and `decode`, the step from a denoised latent to an image.

`DenoiseLoop.denoise` ends at a latent; `decode(optimize_model(DecoderXL()...), latent)` turns it into the image on this
project's kernels: the 3x3 convolutions with their fused GroupNorm+SiLU producers, residual epilogues and the nearest-2x gather
(csrc/gemm_conv_*.hip), and the middle block's self-attention - ONE head of 512 channels over every latent cell - on
csrc/attention_d512.hip.  The encoder, tiled decoding and TAESD are not built.

The eager ops are written in the canonical forms the rewrite passes look for (unet.py): attention as
view -> transpose -> matmul * scale -> softmax -> matmul -> transpose -> contiguous -> view, GroupNorm -> SiLU -> conv as module
calls, the upsample as interpolate(nearest, 2x) -> conv.
"""
from __future__ import annotations

import copy
from typing import Sequence

import torch
from torch import nn
import torch.nn.functional as F

from .unet import Upsample

SCALING_FACTOR = 0.13025          # the published SDXL VAE's latent scale


class VaeResBlock(nn.Module):
    """unet.ResBlock without a time embedding (the VAE has none): GN-SiLU-conv3x3, GN-SiLU-conv3x3, + skip."""

    def __init__(self, c_in: int, c_out: int, groups: int):
        super().__init__()
        self.norm1 = nn.GroupNorm(groups, c_in, eps=1e-6)
        self.conv1 = nn.Conv2d(c_in, c_out, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, c_out, eps=1e-6)
        self.dropout = nn.Dropout(0.0)
        self.conv2 = nn.Conv2d(c_out, c_out, 3, padding=1)
        self.nonlinearity = nn.SiLU()
        self.conv_shortcut = nn.Conv2d(c_in, c_out, 1) if c_in != c_out else None

    def forward(self, x):
        h = self.conv1(self.nonlinearity(self.norm1(x)))
        h = self.conv2(self.dropout(self.nonlinearity(self.norm2(h))))
        if self.conv_shortcut is not None:
            x = self.conv_shortcut(x)
        return x + h


class VaeAttention(nn.Module):
    """The middle block's self-attention over the latent cells: GroupNorm, q / k / v / out projections with bias, one head as wide
    as the block, residual."""

    def __init__(self, dim: int, groups: int):
        super().__init__()
        self.num_heads = 1
        self.head_dim = dim
        self.scale = dim ** -0.5
        self.group_norm = nn.GroupNorm(groups, dim, eps=1e-6)
        self.to_q = nn.Linear(dim, dim)
        self.to_k = nn.Linear(dim, dim)
        self.to_v = nn.Linear(dim, dim)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])

    def forward(self, x):
        b, c, h, w = x.shape
        y = self.group_norm(x).permute(0, 2, 3, 1).reshape(b, h * w, c)
        q = self.to_q(y)
        k = self.to_k(y)
        v = self.to_v(y)
        n, t, d = q.size()                            # (read by the attention pattern alone: none of its values may leave the match)
        q = q.view(q.size(0), q.size(1), self.num_heads, self.head_dim).transpose(1, 2)
        k = k.view(k.size(0), k.size(1), self.num_heads, self.head_dim).transpose(1, 2)
        v = v.view(v.size(0), v.size(1), self.num_heads, self.head_dim).transpose(1, 2)
        a = torch.softmax(torch.matmul(q, k.transpose(-2, -1)) * self.scale, dim=-1)
        o = torch.matmul(a, v).transpose(1, 2).contiguous().view(n, t, d)
        o = self.to_out[1](self.to_out[0](o))
        o = o.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous()
        return o + x


class VaeMidBlock(nn.Module):
    def __init__(self, c: int, groups: int):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResBlock(c, c, groups), VaeResBlock(c, c, groups)])
        self.attentions = nn.ModuleList([VaeAttention(c, groups)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class VaeUpBlock(nn.Module):
    def __init__(self, c_in: int, c_out: int, layers: int, groups: int, up: bool):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResBlock(c_in if i == 0 else c_out, c_out, groups) for i in range(layers)])
        self.upsamplers = nn.ModuleList([Upsample(c_out)]) if up else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        if self.upsamplers is not None:
            x = self.upsamplers[0](x)
        return x


class _Decoder(nn.Module):
    def __init__(self, latent_channels: int, out_channels: int, widths: Sequence[int], layers: int, groups: int):
        super().__init__()
        rev = tuple(reversed(widths))
        self.conv_in = nn.Conv2d(latent_channels, rev[0], 3, padding=1)
        self.mid_block = VaeMidBlock(rev[0], groups)
        self.up_blocks = nn.ModuleList([VaeUpBlock(rev[max(i - 1, 0)], c, layers, groups, up=i < len(rev) - 1)
                                        for i, c in enumerate(rev)])
        self.conv_norm_out = nn.GroupNorm(groups, rev[-1], eps=1e-6)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(rev[-1], out_channels, 3, padding=1)

    def forward(self, z):
        x = self.mid_block(self.conv_in(z))
        for blk in self.up_blocks:
            x = blk(x)
        return self.conv_out(self.conv_act(self.conv_norm_out(x)))


class DecoderXL(nn.Module):
    """The decoder half of the SDXL `AutoencoderKL`: post_quant_conv (1x1, 4 -> 4), decoder.conv_in (4 -> 512), the middle block
    (resnet, one-head 512-channel self-attention, resnet), four up blocks of three resnets (512, 512, 256, 128 channels, a nearest-2x
    `Upsample` behind the first three), conv_norm_out, SiLU, conv_out (128 -> 3).  GroupNorm 32 groups, eps 1e-6.  State-dict keys
    as diffusers spells them (`post_quant_conv.weight`, `decoder.mid_block.attentions.0.to_q.weight`,
    `decoder.up_blocks.2.upsamplers.0.conv.bias`, ...); `load_state_dict` also takes a whole AutoencoderKL state dict and leaves the
    encoder's keys aside.  Restated from memory of the diffusers layout - parity with a published checkpoint unpinned: no
    published checkpoint or diffusers run has been compared.

    forward(z) -> (B, 3, 8h, 8w) for an ALREADY UNSCALED latent z (`decode` divides by the scaling factor).  bfloat16 is the
    intended 16-bit dtype: the published fp16 weights overflow in the decoder's last blocks.

    `optimize_model(DecoderXL().to("cuda", torch.bfloat16), cuda_graph=False)` compiles it; no flag: the module type says what it
    is.  Load the weights BEFORE compiling: the compiled module carries conv_out with a zero fourth filter (the convolution kernels
    want Cout % 4 == 0), a copy of the weights at that moment.  post_quant_conv (16 multiply-adds a latent cell, fits neither
    convolution kernel) stays a torch call, and in fp32 (the strict mode) so does the attention core."""

    def __init__(self, latent_channels: int = 4, out_channels: int = 3, widths: Sequence[int] = (128, 256, 512, 512),
                 layers_per_block: int = 3, groups: int = 32):
        super().__init__()
        self.out_channels = out_channels
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1)
        self.decoder = _Decoder(latent_channels, out_channels, widths, layers_per_block, groups)

    def forward(self, z):
        z = F.conv2d(z, self.post_quant_conv.weight, self.post_quant_conv.bias)      # (a function call: replace_conv leaves it to torch)
        return self.decoder(z)[:, :self.out_channels]

    def load_state_dict(self, state_dict, strict: bool = True, **kwargs):
        own = {k: v for k, v in state_dict.items() if not k.startswith(("encoder.", "quant_conv."))}
        return super().load_state_dict(own, strict=strict, **kwargs)

    def kernel_form(self) -> "DecoderXL":
        """A shallow copy that shares every parameter but conv_out, which gets zero filters up to a multiple of 4 output channels;
        forward slices them away again.  What `replace_backend` traces."""
        conv = self.decoder.conv_out
        pad = -conv.out_channels % 4
        if pad == 0:
            return self
        wide = nn.Conv2d(conv.in_channels, conv.out_channels + pad, 3, padding=1).to(conv.weight.device, conv.weight.dtype)
        with torch.no_grad():
            wide.weight.zero_()
            wide.bias.zero_()
            wide.weight[:conv.out_channels].copy_(conv.weight)
            wide.bias[:conv.out_channels].copy_(conv.bias)
        if conv.weight.is_contiguous(memory_format=torch.channels_last) and not conv.weight.is_contiguous():
            wide = wide.to(memory_format=torch.channels_last)
        wide.requires_grad_(conv.weight.requires_grad)
        new, dec = copy.copy(self), copy.copy(self.decoder)
        new._modules, dec._modules = dict(self._modules), dict(self.decoder._modules)
        dec.conv_out = wide
        new.decoder = dec
        return new


def decode(compiled, latent: torch.Tensor, scaling_factor: float = SCALING_FACTOR) -> torch.Tensor:
    """(B, 4, h, w) latent as the denoise loop leaves it -> (B, 3, 8h, 8w) image in roughly [-1, 1], through a `DecoderXL` (compiled
    by `optimize_model`, or eager)."""
    if latent.dim() != 4:
        raise ValueError(f"decode: a (B, C, h, w) latent expected, got {tuple(latent.shape)}")
    p = next(compiled.parameters())
    with torch.no_grad():
        return compiled((latent / scaling_factor).to(p.dtype))
