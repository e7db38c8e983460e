"""HyperTile sites (addition; hypertile.py): `attention_wrapper` -> `attention_hypertile_wrapper` at the selected self-attentions.

Runs directly after fuse_attention, as insert_reference does and by the same rules: a candidate is an `attention_wrapper` whose query
is the output of a module `<path>.attn1.to_q`; `<path>.attn1` is matched against `hypertile_layers`, every entry a regular expression
`re.search`ed against that path, so ".*" selects every self-attention and "down_blocks.1" the first attention level's.  An entry that
selects no self-attention raises ValueError; cross-attention (`attn2`) is never a candidate.

Only the leaf changes: q, k and v stay the three projections of one input, so the later passes (the fused q|k|v projection, LayerNorm
folding, the strict split images, the fp8 plan) fire on these sites exactly as without the pass; the kernel reads the windows from the
q, k and v columns of that fused buffer where they lie.  Every leaf carries its site index: the per-site tables of the state.
"""
from __future__ import annotations

from typing import Sequence

from torch import fx

from ..hypertile import HyperTile, attention_hypertile_wrapper
from .attention_sites import attention_sites, replace_sites, select_by_layers


def insert_hypertile(gm: fx.GraphModule, hypertile_layers: Sequence[str]) -> int:
    """Rewrite the selected sites and install the state as `gm.hypertile` (outside `using`: ordinary attention); returns the number of sites."""
    chosen, hypertile_layers = select_by_layers(attention_sites(gm, "attn1"), hypertile_layers, "hypertile_layers")
    return replace_sites(gm, chosen, "hypertile", HyperTile([p for _, p in chosen], hypertile_layers), attention_hypertile_wrapper,
                         extra=lambda i: (i,))
