"""The inpainting tests' own statement of the method (checker only; shares no code with stabletriton_amd/inpaint.py), in float64.

`weight64` / `blend64` restate the blend behind one sampler step and return what the kernel's error bounds are made of.  `loop64` is
a float64 inpainting loop around the eager float64 CPU module, built on pag_util's sampler rows and guidance; with `tiles` it composes
its own canvas loop from tiles_util's two moves (cut the next input into windows, blend the windows' predictions).  `wrong=True` is the
wrong blend the loop tests must be able to tell from the right one: the known region re-noised at sigma[i] instead of sigma[i + 1].
"""
import math

import torch

from tests import pag_util as PU
from tests import tiles_util as TU

# significand bits and the smallest normal exponent (value = f * 2^e, f in [0.5, 1)) of the types next_in comes in
P_BITS = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}
E_MIN = {torch.float32: -125, torch.bfloat16: -125, torch.float16: -13}


def ulp(x64, dtype):
    """The spacing of `dtype` at |x| (float64 tensor): 2^(e - p) for |x| = f 2^e, f in [0.5, 1); the subnormal spacing below."""
    _, e = torch.frexp(x64.abs())
    e = e.clamp_min(E_MIN[dtype]).double()
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - P_BITS[dtype])


def init_latent(hw, batch=1, seed=7):
    """The image to keep: a seeded latent of about the spread a VAE-encoded image has."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((batch, 4, hw[0], hw[1]), generator=g) * 0.8


def half_mask(hw):
    """Binary (1, H, W): the left half is kept (0), the right half repainted (1)."""
    m = torch.ones((1, hw[0], hw[1]))
    m[:, :, :hw[1] // 2] = 0.0
    return m


def level_mask(hw, levels):
    """(1, H, W): vertical bands of equal width, one per level (the last band takes the remainder)."""
    m = torch.empty((1, hw[0], hw[1]))
    band = hw[1] // len(levels)
    for k, v in enumerate(levels):
        m[:, :, k * band:(hw[1] if k == len(levels) - 1 else (k + 1) * band)] = float(v)
    return m


def latent_bound(mag64):
    """|latent - blend64| <= 2^-22 (|init| + |s noise| + |latent_in|): the fp32 roundings of known = fma(s, noise, init), of
    latent - known and of the second fma, each at most 2^-24 of a value no larger than that magnitude."""
    return 2.0 ** -22 * mag64


def next_bound(next64, mag64, sc, dtype):
    """|next_in - v sc| <= one ulp of the type at the float64 value (the fp32 product's rounding and the one to the type) plus the
    latent's bound carried through the scale."""
    return ulp(next64, dtype) + latent_bound(mag64) * abs(float(sc))


def weight64(mask, thr_i=None):
    """(1 | B, H, W) -> float64 (1 | B, 1, H, W): the mask itself, or (mask > thr_i); NaN and >= 1 repaint (1), negative keeps (0)."""
    m = mask.double()
    w = m if thr_i is None else (m > float(thr_i)).double()
    w = torch.where(w < 1, w.clamp_min(0.0), torch.ones_like(w))
    return w[:, None]


def blend64(latent, init, noise, mask, s, sc, thr_i=None):
    """One blend in float64 from the stored values: (v, v * sc, w, magnitude) with v the latent behind the blend (the input where
    w == 1), w (1 | B, 1, H, W) and magnitude = |init| + |s noise| + |latent_in|, what the fp32 roundings scale with."""
    lat, a, z = latent.double(), init.double(), noise.double()
    w = weight64(mask, thr_i)
    known = a + float(s) * z
    v = torch.where(w == 1, lat, torch.where(w == 0, known, known + w * (lat - known)))
    return v, v * float(sc), w, a.abs() + (float(s) * z).abs() + lat.abs()


def loop64(unet64, x, noise, tables, init, mask, g=None, phi=None, thr=None, wrong=False, tiles=None, seed=None, start=0,
           pos=slice(1, 2), neg=slice(0, 1)):
    """float64 inpainting loop: `noise` (B, 4, H, W) unit start noise, conditioning rows x[k][pos] / x[k][neg], blocks [neg | pos]
    under guidance g; pag_util's guidance (with rescale phi) and sampler rows; behind every step the blend with known =
    init + sigma[i + 1] noise (`wrong`: sigma[i]).  `thr`: n thresholds (differential mode).  `tiles` = (ys, xs, (h, w), weights64):
    the UNet sees the windows of the canvas, their predictions are blended per canvas pixel, the mask lives on the canvas.  `start`:
    the img2img start step (the trajectory starts from init + sigma[start] noise)."""
    n = tables.n_steps
    B = noise.shape[0]
    H, W = noise.shape[-2:]
    sig = [float(v) for v in tables.sigmas]
    z, a = noise.double(), init.double().expand(B, -1, -1, -1)
    lat = z * tables.init_noise_sigma if start == 0 else a + z * sig[start]
    rows, in_scale = PU.rows64(tables), tables.in_scale()
    dsigma = tables.dsigma() if rows is None else None
    blocks = ([neg] if g is not None else []) + [pos]
    T = len(tiles[0]) * len(tiles[1]) if tiles is not None else 1

    def per_window(t):
        t = t.double()
        return t if T == 1 else torch.cat([t[b:b + 1] for b in range(B) for _ in range(T)])

    ehs, te, ti = (torch.cat([per_window(x[k][r]) for r in blocks]) for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    prev = None
    for i in range(start, n):
        t = torch.tensor(float(tables.timesteps[i]), dtype=torch.float64)
        xin = lat * float(in_scale[i])
        if tiles is not None:
            xin = TU.cut64(xin, tiles[0], tiles[1], tiles[2])
        with torch.no_grad():
            e_all = unet64(torch.cat([xin] * len(blocks)), t, ehs, {"text_embeds": te, "time_ids": ti})[0].double()
        parts = list(e_all.split(B * T))
        if tiles is not None:
            parts = [TU.blend_fast64(p, tiles[0], tiles[1], (H, W), tiles[3]) for p in parts]
        e_neg = parts.pop(0) if g is not None else None
        e_pos = parts.pop(0)
        e = e_pos if g is None else PU.guide64(e_neg, e_pos, e_pos, g, 0.0, phi)
        if rows is None:
            lat = lat + e * float(dsigma[i])
        else:
            sigma, ca, cb, k, c = rows[i]
            d = lat - sigma * e
            new = ca * lat + cb * d if (i == start or k == 0.0) else ca * lat + cb * ((1.0 + k) * d - k * prev)
            if c != 0.0:
                new = new + c * PU.unit64(seed, i + 1, tuple(lat.shape))
            lat, prev = new, d
        w = weight64(mask, None if thr is None else thr[i])
        known = a + (sig[i] if wrong else sig[i + 1]) * z
        lat = torch.where(w == 1, lat, torch.where(w == 0, known, known + w * (lat - known)))
    return lat


# ------------------------------------------------------------------------------------------------ one blend: cases and the check
# (shared by the CPU route's test and the kernel's: tests/test_inpaint_host.py, tests/test_inpaint_gpu.py)
N_STEPS = 4
SIGMA_NEXT = torch.tensor([7.5, 2.25, 0.6, 0.0])
IN_SCALE = torch.tensor([0.07, 0.13, 0.4, 0.85])
# (H, W), blocks, mask rows, channels (batch 2 throughout): 70 pixels in one workgroup, 514 in three with a partial last one
SHAPES = {"5x7_b1_m1": ((5, 7), 1, 1, 4), "5x7_b2_mB": ((5, 7), 2, 2, 4), "5x7_b3_m1": ((5, 7), 3, 1, 4), "257x1_b2_m1": ((257, 1), 2, 1, 4),
          "257x1_b1_mB": ((257, 1), 1, 2, 4), "257x1_b3_mB": ((257, 1), 3, 2, 4), "5x7_b2_mB_c8": ((5, 7), 2, 2, 8)}


def blend_case(hw, blocks, mask_rows, C, kind, dtype, seed=21):
    """(latent, next_in, init, noise, mask, thr) of one blend, batch 2: fp32 values, next_in NaN (what is not written stays NaN)."""
    B = 2
    g = torch.Generator().manual_seed(seed)
    cl = torch.channels_last
    lat, init, noise = ((torch.randn((B, C) + hw, generator=g) * s).contiguous(memory_format=cl) for s in (6.0, 0.8, 1.0))
    n = hw[0] * hw[1]
    u = torch.rand((mask_rows, n), generator=g)
    if kind == "ones":
        m = torch.ones(mask_rows, n)
    elif kind == "zeros":
        m = torch.zeros(mask_rows, n)
    elif kind == "binary":
        m = (u > 0.5).float()
    elif kind == "soft":
        m = torch.where(u < 0.2, torch.zeros_like(u), torch.where(u > 0.8, torch.ones_like(u), u))
    else:                                                      # "levels": a three-level change map for the threshold mode
        m = torch.where(u < 0.33, torch.zeros_like(u), torch.where(u > 0.66, torch.ones_like(u), torch.full_like(u, 0.5)))
    thr = torch.tensor([0.75, 0.5, 0.25, 0.0]) if kind == "levels" else None
    nxt = torch.full((blocks * B, C) + hw, math.nan, dtype=dtype).contiguous(memory_format=cl)
    return lat, nxt, init, noise, m.view((mask_rows,) + hw).contiguous(), thr


def check_blend(got_lat, got_next, case, step, dtype, what):
    """Every property of one blend against blend64: nothing written at w == 1, exact at w == 0 with s == 0, the rest inside the
    format-derived bounds, all row blocks equal.  `got_next` started as NaN everywhere.  Returns the worst fractions of the bounds."""
    lat, _, init, noise, mask, thr = case
    B = lat.shape[0]
    i = step
    s, sc = float(SIGMA_NEXT[i]), float(IN_SCALE[min(i + 1, N_STEPS - 1)])
    v, nx, w, mag = blend64(lat, init, noise, mask, s, sc, None if thr is None else float(thr[i]))
    full = lambda t: t.expand_as(v)
    repaint, keep = full(w == 1), full(w == 0)
    gl, gn = got_lat.double().cpu(), got_next.cpu()
    assert torch.equal(got_lat.cpu()[repaint], lat[repaint]), f"{what}: latent written where w == 1"
    blocks = gn.shape[0] // B
    for r in range(blocks):
        rows = gn[r * B:(r + 1) * B]
        assert bool(torch.isnan(rows[repaint]).all()), f"{what}: next_in written where w == 1 (row block {r})"
        assert bool(torch.isfinite(rows[~repaint]).all()), f"{what}: a next_in element was never stored (row block {r})"
        assert torch.equal(rows[~repaint], gn[:B][~repaint]), f"{what}: row block {r} differs from row block 0"
    if s == 0.0:
        assert torch.equal(got_lat.cpu()[keep], init[keep]), f"{what}: w == 0 at sigma 0 must give init bit for bit"
    fl = fn = 0.0
    if bool((~repaint).any()):
        fl = float(((gl - v).abs() / latent_bound(mag).clamp_min(1e-300))[~repaint].max())
        fn = float(((gn[:B].double() - nx).abs() / next_bound(nx, mag, sc, dtype).clamp_min(1e-300))[~repaint].max())
    assert fl <= 1.0 and fn <= 1.0, f"{what}: latent {fl:.3g} x its bound, next_in {fn:.3g} x its bound"
    return fl, fn
