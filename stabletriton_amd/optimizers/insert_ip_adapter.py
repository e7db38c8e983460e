"""IP-Adapter cross-attention sites (addition; ip_adapter.py): `attention_wrapper` -> `attention_ip_wrapper` at every
cross-attention.

Runs where insert_regions runs, directly after fuse_attention, while the projections are still call_module nodes whose targets
spell the module path, and selects sites the same way: an `attention_wrapper` whose query is the output of a module
`<path>.attn2.to_q` (the classes of the modules are never looked at, a prefix in front of the block names does not matter).
Self-attention (`attn1`) is never a site.  Every site gets its index into the state's tables as a constant argument; the widths
(C_site, cross_dim) are read off the site's `to_k` weight.

Only the leaf changes, so the K / V projections of the text context are hoisted and fused as without the pass, and the query
projection still folds its LayerNorm.  The cost: `fuse_query_projection_into_attention` no longer matches these sites - they run
as `ln_linear_wrapper` plus the segmented leaf, one launch more per site than the fused form, as with regions - and every image
segment that is on adds one 64-key tile pass to the site's launch.
"""
from __future__ import annotations

from torch import fx

from ..ip_adapter import IPAdapter, attention_ip_wrapper, parse_token_counts
from ..regions import site_levels
from .attention_sites import attention_sites, replace_sites


def insert_ip_adapter(gm: fx.GraphModule, ip_adapter) -> int:
    """Rewrite every cross-attention site and install the state as `gm.ip_adapter` (unbound; every slot "off"); returns the number
    of sites."""
    tokens = parse_token_counts(ip_adapter)
    chosen = attention_sites(gm, "attn2")
    if not chosen:
        raise ValueError("ip_adapter: this UNet has no cross-attention (attn2) site")
    sites = [p for _, p in chosen]
    keys = [gm.get_submodule(p + ".to_k").weight for p in sites]
    dims = [(int(w.shape[0]), int(w.shape[1])) for w in keys]
    state = IPAdapter(tokens, sites, dims, site_levels(sites, [name for name, _ in gm.named_modules()]), like=keys[0])
    return replace_sites(gm, chosen, "ip_adapter", state, attention_ip_wrapper, lambda i: (i,))
