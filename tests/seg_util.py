"""The SEG tests' own statement of the method (checker only; shares no code with stabletriton_amd/seg.py), in float64.

Rules 1-7 of smoothed energy guidance as this project states them: the tap count and its clamp on min(h, w), the normalised Gaussian
taps, the separable convolution of every reflect-padded channel plane (torch's own F.pad(mode="reflect") and conv2d), the spatial
mean at sigma >= 9999, the site's token grid from the call's latent size.  `hooked` is the independent eager route: forward hooks on
the selected `attn1` modules of the eager UNet2DConditionModel that recompute the tail rows of the module's output with blurred
queries; `loop64` is a float64 denoise loop around a (hooked, float64, CPU) module built on pag_util's sampler rows and guidance.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

from tests import pag_util as PU

INF = float("inf")


def tap_count(sigma, h, w):
    c = math.ceil(6 * sigma)
    k = c + 1 - (c % 2)
    m = min(h, w)
    return min(k, m + 1 - (m % 2))


def taps64(sigma, k):
    x = torch.arange(k, dtype=torch.float64) - (k - 1) / 2
    e = torch.exp(-0.5 * (x / sigma) ** 2)
    return e / e.sum()


def reflect_index(j, n):
    """Where sample j of an axis of n samples, j in [-(n - 1), 2 (n - 1)], is found after reflection (the edge not repeated)."""
    if j < 0:
        return -j
    return 2 * (n - 1) - j if j >= n else j


def grid_of(latent_hw, tokens):
    lh, lw = latent_hw
    f = math.sqrt(lh * lw / tokens)
    if f != int(f) or lh % int(f) or lw % int(f):
        raise ValueError(f"{tokens} tokens are no whole-number reduction of a {lh} x {lw} latent")
    f = int(f)
    return lh // f, lw // f


def blur64(q, grid_hw, sigma):
    """q (n, T, C), any float dtype -> the blurred queries in float64."""
    h, w = grid_hw
    n, T, C = q.shape
    assert T == h * w
    x = q.double()
    if sigma >= 9999:
        return x.mean(dim=1, keepdim=True).expand(n, T, C).clone()
    k = tap_count(sigma, h, w)
    g = taps64(sigma, k)
    planes = x.view(n, h, w, C).permute(0, 3, 1, 2).reshape(n * C, 1, h, w)
    planes = F.pad(planes, (k // 2, k // 2, k // 2, k // 2), mode="reflect")
    planes = F.conv2d(planes, g.view(1, 1, 1, k))
    planes = F.conv2d(planes, g.view(1, 1, k, 1))
    return planes.view(n, C, h, w).permute(0, 2, 3, 1).reshape(n, T, C)


def blur_bound(q, grid_hw, sigma, rounding):
    """Elementwise bound on |kernel - blur64| from the arithmetic: the output's rounding (rel, abs) plus the worst case of a
    sequential fp32 sum per pass, (k + 8) 2^-24 sum |g_i| |x_i|, carried through the second pass; mean mode (T + 8) 2^-24 mean |x|."""
    h, w = grid_hw
    n, T, C = q.shape
    ulp = 2.0 ** -24
    rel, absolute = rounding
    want = blur64(q, grid_hw, sigma)
    mag = blur64(q.double().abs(), grid_hw, sigma)                 # sum |g| |x| of both passes: the blur of |x|
    if sigma >= 9999:
        return rel * want.abs() + absolute + (T + 8) * ulp * mag
    k = tap_count(sigma, h, w)
    return rel * want.abs() + absolute + 2 * (k + 8) * ulp * mag


def attention64(q, k, v, heads, scale):
    B, T, C = q.shape
    d = C // heads
    sp = lambda t: t.double().view(B, -1, heads, d).transpose(1, 2)
    p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * scale, dim=-1)
    return (p @ sp(v)).transpose(1, 2).reshape(B, T, C)


@contextlib.contextmanager
def hooked(unet, layers, chunks, latent_hw, sigma):
    """The eager `unet` whose selected self-attentions recompute the last B // chunks batch rows with blurred queries."""
    handles = []
    mods = dict(unet.named_modules())

    def hook(mod, args, out):
        x = args[0]
        b = x.shape[0]
        assert b % chunks == 0
        n = b // chunks
        xt = x[b - n:]
        grid = grid_of(latent_hw, xt.shape[1])
        q = blur64(mod.to_q(xt), grid, sigma).to(xt.dtype)
        o = attention64(q, mod.to_k(xt), mod.to_v(xt), mod.num_heads, mod.scale).to(xt.dtype)
        out = out.clone()
        out[b - n:] = mod.to_out[0](o)
        return out

    if chunks:
        for name in PU.selected(unet, layers):
            handles.append(mods[name].register_forward_hook(hook))
    try:
        yield unet
    finally:
        for h in handles:
            h.remove()


def loop64(unet64, x, tables, s, sigma, latent_hw, g=None, phi=None, seed=None, layers=("mid",), pos=slice(1, 2), neg=slice(0, 1)):
    """float64 SEG loop around the eager float64 CPU module `unet64`: pag_util.loop64 with the blurred-query hooks; rows
    [neg | pos | pert] (g given) or [pos | pert]; `s` a float or one value per step.  Returns (final latent, |e_pos - e_pert| max
    at step 0)."""
    n = tables.n_steps
    b = x["latent"][pos].shape[0]
    lat = x["latent"][:b].double() * tables.init_noise_sigma
    rows, in_scale = PU.rows64(tables), tables.in_scale()
    dsigma = tables.dsigma() if rows is None else None
    blocks = ([neg] if g is not None else []) + [pos, pos]
    ehs, te, ti = (torch.cat([x[k][r] for r in blocks]).double() for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    prev, gap0 = None, None
    for i in range(n):
        t = torch.tensor(float(tables.timesteps[i]), dtype=torch.float64)
        xin = torch.cat([lat] * len(blocks)) * float(in_scale[i])
        with torch.no_grad(), hooked(unet64, layers, len(blocks), latent_hw, sigma):
            e_all = unet64(xin, t, ehs, {"text_embeds": te, "time_ids": ti})[0].double()
        parts = list(e_all.split(b))
        e_neg = parts.pop(0) if g is not None else None
        e_pos, e_pert = parts
        si = float(s[i]) if hasattr(s, "__len__") else float(s)
        e = PU.guide64(e_neg, e_pos, e_pert, g, si, phi)
        if i == 0:
            gap0 = float((e_pos - e_pert).abs().max())
        if rows is None:
            lat = lat + e * float(dsigma[i])
        else:
            sig, a, bb, k, c = rows[i]
            d = lat - sig * e
            new = a * lat + bb * d if (i == 0 or k == 0.0) else a * lat + bb * ((1.0 + k) * d - k * prev)
            if c != 0.0:
                new = new + c * PU.unit64(seed, i + 1, tuple(lat.shape))
            lat, prev = new, d
    return lat, gap0
