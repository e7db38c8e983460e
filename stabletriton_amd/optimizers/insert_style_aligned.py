"""StyleAligned sites (addition; style_aligned.py): `attention_wrapper` -> `attention_style_wrapper` at the selected
self-attentions.

Runs directly after fuse_attention, as insert_reference does and by the same rules: a candidate is an `attention_wrapper` whose
query is the output of a module `<path>.attn1.to_q`; `<path>.attn1` is matched against `style_aligned_layers`, every entry a regular
expression `re.search`ed against that path, so ".*" selects every self-attention (what the published method does).  An entry that
selects no self-attention raises ValueError; cross-attention (`attn2`) is never a candidate.

Only the leaf changes: q, k and v stay the three projections of one input, so the later passes (the fused q|k|v projection,
LayerNorm folding, the fp8 plan) fire on these sites exactly as without the pass; the leaf then renormalises the q and k columns of
that fused buffer in place and reads the style row's keys and values from it, with no copy.  The state records every site's
channel width (its query projection's), which sizes the AdaIN scratch.
"""
from __future__ import annotations

from typing import Sequence

from torch import fx

from ..style_aligned import StyleAligned, attention_style_wrapper
from .attention_sites import attention_sites, replace_sites, select_by_layers


def insert_style_aligned(gm: fx.GraphModule, style_aligned_layers: Sequence[str]) -> int:
    """Rewrite the selected sites and install the state as `gm.style_aligned` (per 0: ordinary attention); returns the number of sites."""
    chosen, layers = select_by_layers(attention_sites(gm, "attn1"), style_aligned_layers, "style_aligned_layers")
    widths = [gm.get_submodule(str(n.args[0].target)).out_features for n, _ in chosen]
    return replace_sites(gm, chosen, "style_aligned", StyleAligned([p for _, p in chosen], layers, widths), attention_style_wrapper)
