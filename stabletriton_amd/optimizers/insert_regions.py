"""Regional cross-attention sites (addition; regions.py): `attention_wrapper` -> `attention_regions_wrapper` at every
cross-attention.

Runs where insert_pag runs, directly after fuse_attention, while the projections are still call_module nodes whose targets spell
the module path: a site is an `attention_wrapper` whose query is the output of a module `<path>.attn2.to_q` (the classes of the
modules are never looked at, and a prefix in front of the block names - the ComfyUI entry wraps the network as `unet.` - does not
matter).  Self-attention (`attn1`) is never a site.

Only the leaf changes, so the K / V projections of the text context are hoisted and fused as without the pass (R prompts
concatenated along the token axis come out as R key/value segments), and the query projection still folds its LayerNorm.
`fuse_query_projection_into_attention` no longer matches these sites: they run as `ln_linear_wrapper` plus the regional leaf, one
launch more per site than the fused form.
"""
from __future__ import annotations

from torch import fx

from ..regions import Regions, attention_regions_wrapper, site_levels
from .attention_sites import attention_sites, replace_sites


def insert_regions(gm: fx.GraphModule, R: int, seg_len: int = 77) -> int:
    """Rewrite every cross-attention site and install the state as `gm.regions` (unbound; "off" once bound); returns the number of
    sites."""
    chosen = attention_sites(gm, "attn2")
    sites = [p for _, p in chosen]
    state = Regions(R, seg_len, sites, site_levels(sites, [name for name, _ in gm.named_modules()]))      # (validates R, seg_len)
    if not chosen:
        raise ValueError("regions: this UNet has no cross-attention (attn2) site")
    return replace_sites(gm, chosen, "regions", state, attention_regions_wrapper)
