"""The PAG tests' own statement of the method (checker only; shares no code with stabletriton_amd/pag.py).

`hooked` is the independent eager route: forward hooks on the selected `attn1` modules of the eager UNet2DConditionModel that
overwrite the tail rows of the module's output with `to_out[0](to_v(x_tail))` - what identity attention gives (diffusers'
PAGCFGIdentitySelfAttnProcessor2_0).  `guide64` is the float64 guidance of diffusers' PAGMixin (+ rescale_noise_cfg), `loop64` a
float64 denoise loop around a (hooked, float64, CPU) module for the three samplers of the project.
"""
import contextlib
import math
import re

import torch

from stabletriton_amd import rng


def selected(unet, layers):
    """Names of the attn1 modules whose path any of `layers` (regular expressions) is found in; "mid" finds mid_block."""
    names = [n for n, _ in unet.named_modules() if n.endswith(".attn1")]
    return [n for n in names if any(re.search(p, n) for p in layers)]


@contextlib.contextmanager
def hooked(unet, layers, chunks):
    """The eager `unet` whose selected self-attentions return to_out(to_v(x)) for the last B // chunks batch rows."""
    handles = []
    mods = dict(unet.named_modules())

    def hook(mod, args, out):
        x = args[0]
        b = x.shape[0]
        assert b % chunks == 0
        n = b // chunks
        out = out.clone()
        out[b - n:] = mod.to_out[0](mod.to_v(x[b - n:]))
        return out

    if chunks:
        for name in selected(unet, layers):
            handles.append(mods[name].register_forward_hook(hook))
    try:
        yield unet
    finally:
        for h in handles:
            h.remove()


def three_rows(hw, seed, **kw):
    """UNet inputs of one [negative | positive | perturbed] evaluation from synth.denoise_inputs(2, hw, seed): row 0 is the
    negative prompt, row 1 the prompt (also the perturbed row's), row 0's latent in all three rows."""
    from stabletriton_amd import synth
    x = synth.denoise_inputs(2, hw, seed, **kw)
    out = {k: x[k][[0, 1, 1]].clone() for k in ("encoder_hidden_states", "text_embeds", "time_ids")}
    out["latent"] = x["latent"][[0, 0, 0]].clone()
    return out


def guide64(e_neg, e_pos, e_pert, g, s, phi=None):
    """float64: e = e_neg + g (e_pos - e_neg) + s (e_pos - e_pert), or e_pos + s (e_pos - e_pert) when e_neg is None; then
    diffusers' rescale_noise_cfg of the total (std over C, H, W with correction 1) when phi is given."""
    ep, ex = e_pos.double(), e_pert.double()
    if e_neg is None:
        assert phi is None
        return ep + s * (ep - ex)
    en = e_neg.double()
    e = en + g * (ep - en) + s * (ep - ex)
    if phi is not None:
        r = ep.std(dim=(1, 2, 3), keepdim=True) / e.std(dim=(1, 2, 3), keepdim=True)
        e = phi * (e * r) + (1.0 - phi) * e
    return e


def guide_magnitude(e_neg, e_pos, e_pert, g, s, phi=None):
    """What the fp32 terms of guide64's e are made of: the existing two-way bound extended by |s| (|e_pos| + |e_pert|)."""
    ep, ex = e_pos.double(), e_pert.double()
    extra = abs(s) * (ep.abs() + ex.abs())
    if e_neg is None:
        return ep.abs() + extra
    en = e_neg.double()
    mag = en.abs() + abs(g) * (ep.abs() + en.abs()) + extra
    if phi is not None:
        e = guide64(e_neg, e_pos, e_pert, g, s)
        r = ep.std(dim=(1, 2, 3), keepdim=True) / e.std(dim=(1, 2, 3), keepdim=True)
        mag = mag * (abs(phi) * r + abs(1.0 - phi))
    return mag


# ---- float64 sampler rows from the stored sigmas (the formulas of scheduler.py's docstring, restated) ------------------------
def rows64(tables):
    """[sigma, a, b, k, c] per step: Euler tables give None (the Euler update needs only dsigma)."""
    name = type(tables).__name__
    if name == "EulerTables":
        return None
    s = [float(v) for v in tables.sigmas]
    eta = getattr(tables, "eta", 0.0) if name == "SDETables" else 0.0
    s_noise = getattr(tables, "s_noise", 1.0)
    rows = []
    for i in range(len(s) - 1):
        sc, sn = s[i], s[i + 1]
        if sn == 0.0:
            rows.append((sc, 0.0, 1.0, 0.0, 0.0))
            continue
        if name == "SDETables" and tables.sampler == "euler_ancestral":
            up = min(sn, eta * math.sqrt(sn ** 2 * (sc ** 2 - sn ** 2) / sc ** 2))
            down = math.sqrt(sn ** 2 - up ** 2)
            rows.append((sc, down / sc, 1.0 - down / sc, 0.0, s_noise * up))
            continue
        h = math.log(sc) - math.log(sn)
        k = 0.0 if i == 0 else 1.0 / (2.0 * ((math.log(s[i - 1]) - math.log(sc)) / h))
        if name == "SDETables":
            rows.append((sc, sn / sc * math.exp(-eta * h), -math.expm1(-(1.0 + eta) * h), k,
                         s_noise * sn * math.sqrt(-math.expm1(-2.0 * eta * h))))
        else:
            rows.append((sc, sn / sc, -math.expm1(-h), k, 0.0))
    return rows


def unit64(seed, counter, shape):
    """rng.py's float64 stream laid out as a channels_last latent: j = (h W + w) C + c."""
    b, c, h, w = shape
    z = rng.normal([seed + i for i in range(b)], counter, c * h * w)
    return torch.from_numpy(z).view(b, h, w, c).permute(0, 3, 1, 2)


def loop64(unet64, x, tables, s, g=None, phi=None, seed=None, layers=("mid",), pos=slice(1, 2), neg=slice(0, 1)):
    """float64 PAG loop around the eager float64 CPU module `unet64`: rows [neg | pos | pert] (g given) or [pos | pert]; the
    perturbed rows carry the positive conditioning and the same latent; `s` a float or one value per step (s = None: no
    perturbed rows at all, plain CFG / unguided).  Returns (final latent, |e_pos - e_pert| max at step 0)."""
    n = tables.n_steps
    b = x["latent"][pos].shape[0]
    lat = x["latent"][:b].double() * tables.init_noise_sigma
    rows, in_scale = rows64(tables), tables.in_scale()
    dsigma = tables.dsigma() if rows is None else None
    blocks = ([neg] if g is not None else []) + [pos] + ([pos] if s is not None else [])
    ehs, te, ti = (torch.cat([x[k][r] for r in blocks]).double() for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    chunks = len(blocks) if s is not None else 0
    prev, gap0 = None, None
    for i in range(n):
        t = torch.tensor(float(tables.timesteps[i]), dtype=torch.float64)
        xin = torch.cat([lat] * len(blocks)) * float(in_scale[i])
        with torch.no_grad(), hooked(unet64, layers, chunks):
            e_all = unet64(xin, t, ehs, {"text_embeds": te, "time_ids": ti})[0].double()
        parts = list(e_all.split(b))
        e_neg = parts.pop(0) if g is not None else None
        e_pos = parts.pop(0)
        if s is None:
            e = e_pos if g is None else guide64(e_neg, e_pos, e_pos, g, 0.0, phi)
        else:
            e_pert = parts.pop(0)
            si = float(s[i]) if hasattr(s, "__len__") else float(s)
            e = guide64(e_neg, e_pos, e_pert, g, si, phi)
            if i == 0:
                gap0 = float((e_pos - e_pert).abs().max())
        if rows is None:
            lat = lat + e * float(dsigma[i])
        else:
            sigma, a, bb, k, c = rows[i]
            d = lat - sigma * e
            if i == 0 or k == 0.0:
                new = a * lat + bb * d
            else:
                new = a * lat + bb * ((1.0 + k) * d - k * prev)
            if c != 0.0:
                new = new + c * unit64(seed, i + 1, tuple(lat.shape))
            lat, prev = new, d
    return lat, gap0
