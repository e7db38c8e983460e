"""The reference-only tests' own statement of the method (checker only; shares no code with stabletriton_amd/reference.py).

`hooked` is the independent eager route: forward hooks on the selected `attn1` modules of the eager UNet2DConditionModel that
recompute the leading rows' output as `attn1(x, context=cat([x, x[ref_of_row]], 1))` - the module's own cross-attention path over
its own tokens followed by its reference row's.  `loop64` is tests/pag_util.py's float64 denoise loop with a reference block in place
of the perturbed one: rows [neg | pos | ref] (g given) or [pos | ref], the reference rows carrying the positive conditioning and, at
step i, (ref_init + sigma[i] * ref_noise) * in_scale[i]; their prediction is dropped.
"""
import contextlib

import torch

from tests import pag_util as PU


def ref_of_row(b: int, batch: int, chunks: int) -> int:
    """The reference row of leading row b in a call of `batch` rows: lead + b % (batch // chunks)."""
    n = batch // chunks
    return batch - n + b % n


@contextlib.contextmanager
def hooked(unet, layers, chunks):
    """The eager `unet` whose selected self-attentions let every row but the last B // chunks also attend to its reference row."""
    handles = []
    mods = dict(unet.named_modules())

    def hook(mod, args, out):
        x = args[0]
        b = x.shape[0]
        assert b % chunks == 0
        lead = b - b // chunks
        if lead == 0:
            return out
        rows = torch.tensor([ref_of_row(r, b, chunks) for r in range(lead)])
        out = out.clone()
        out[:lead] = type(mod).forward(mod, x[:lead], context=torch.cat([x[:lead], x[rows]], dim=1))
        return out

    if chunks:
        for name in PU.selected(unet, layers):
            handles.append(mods[name].register_forward_hook(hook))
    try:
        yield unet
    finally:
        for h in handles:
            h.remove()


def loop64(unet64, x, tables, ref_init, ref_noise, g=None, phi=None, seed=None, layers=(".*",), pos=slice(1, 2), neg=slice(0, 1),
           on=None):
    """float64 loop around the eager float64 CPU module `unet64`; `ref_init` None: no reference rows at all (plain CFG / unguided);
    `on`: one flag per step (None: every step) - a step whose flag is off runs the unhooked module on the same rows."""
    n = tables.n_steps
    b = x["latent"][pos].shape[0]
    lat = x["latent"][:b].double() * tables.init_noise_sigma
    rows, in_scale = PU.rows64(tables), tables.in_scale()
    dsigma = tables.dsigma() if rows is None else None
    blocks = ([neg] if g is not None else []) + [pos] + ([pos] if ref_init is not None else [])
    ehs, te, ti = (torch.cat([x[k][r] for r in blocks]).double() for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    prev = None
    for i in range(n):
        t = torch.tensor(float(tables.timesteps[i]), dtype=torch.float64)
        lead = len(blocks) - (1 if ref_init is not None else 0)
        xin = [lat * float(in_scale[i])] * lead
        chunks = 0
        if ref_init is not None:
            xin.append((ref_init.double() + float(tables.sigmas[i]) * ref_noise.double()).expand_as(lat) * float(in_scale[i]))
            chunks = len(blocks) if (on is None or on[i]) else 0
        with torch.no_grad(), hooked(unet64, layers, chunks):
            e_all = unet64(torch.cat(xin), t, ehs, {"text_embeds": te, "time_ids": ti})[0].double()
        parts = list(e_all.split(b))
        e_neg = parts.pop(0) if g is not None else None
        e_pos = parts.pop(0)
        e = e_pos if g is None else PU.guide64(e_neg, e_pos, e_pos, g, 0.0, phi)
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
                new = new + c * PU.unit64(seed, i + 1, tuple(lat.shape))
            lat, prev = new, d
    return lat
