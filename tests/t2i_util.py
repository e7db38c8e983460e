"""The T2I-Adapter tests' own statement of the method (checker only; shares no code with stabletriton_amd/t2i_adapter.py).

`hooked` is the reference of every test: the EAGER UNet2DConditionModel with PyTorch forward hooks that add s * f to the outputs of
down_blocks[0].downsamplers[0], down_blocks[1].attentions[-1], down_blocks[-1].attentions[-1] and mid_block.  Never the compiled
module.  The hooks are removed in a `finally` (the SDXL eager module is shared by the whole session)."""
import contextlib

import torch

from stabletriton_amd import synth


def site_modules(unet):
    return [unet.down_blocks[0].downsamplers[0], unet.down_blocks[1].attentions[-1], unet.down_blocks[-1].attentions[-1], unet.mid_block]


def site_shapes(spec, latent_hw):
    """(C, h, w) per site, written out for a three-level network: A and B at half the latent, C and M at a quarter (the stride-2
    convolutions round up)."""
    lh, lw = (latent_hw, latent_hw) if isinstance(latent_hw, int) else latent_hw
    h1, w1 = (lh + 1) // 2, (lw + 1) // 2
    h2, w2 = (h1 + 1) // 2, (w1 + 1) // 2
    w = spec.widths
    return [(w[0], h1, w1), (w[1], h1, w1), (w[-1], h2, w2), (w[-1], h2, w2)]


def features(spec, latent_hw, rows=1, seed=7):
    """Synthetic feature maps of magnitude ~1, fp32, deterministic."""
    return [synth.normal(f"t2i.feature.{k}.{rows}.{c}x{h}x{w}", (rows, c, h, w), seed + k)
            for k, (c, h, w) in enumerate(site_shapes(spec, latent_hw))]


@contextlib.contextmanager
def hooked(unet, feats, scale):
    """`unet` with out + scale * f at the four places; feats of 1 or B rows are repeated over the row blocks of a guided batch.
    scale None: nothing is hooked."""
    handles = []
    try:
        if scale is not None:
            for mod, f in zip(site_modules(unet), feats):
                def add(module, args, out, f=f):
                    ff = f.to(device=out.device, dtype=out.dtype)
                    return out + scale * ff.repeat(out.shape[0] // ff.shape[0], 1, 1, 1)
                handles.append(mod.register_forward_hook(add))
        yield unet
    finally:
        for h in handles:
            h.remove()
