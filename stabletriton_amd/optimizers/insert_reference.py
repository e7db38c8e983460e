"""Reference-only sites (addition; reference.py): `attention_wrapper` -> `attention_reference_wrapper` at the selected
self-attentions.

Runs directly after fuse_attention, as insert_pag does and by the same rules: a candidate is an `attention_wrapper` whose query is
the output of a module `<path>.attn1.to_q`; `<path>.attn1` is matched against `reference_layers`, every entry a regular expression
`re.search`ed against that path, so ".*" selects every self-attention (what the reference-only methods do) and "up_blocks" the
decoder's.  An entry that selects no self-attention raises ValueError; cross-attention (`attn2`) is never a candidate.

Only the leaf changes: q, k and v stay the three projections of one input, so the later passes (the fused q|k|v projection,
LayerNorm folding, the strict split images, the fp8 plan) fire on these sites exactly as without the pass; the leaf then takes the
reference rows' keys and values as batch slices of the k and v columns of that fused buffer, with no copy.
"""
from __future__ import annotations

from typing import Sequence

from torch import fx

from ..reference import ReferenceRows, attention_reference_wrapper
from .attention_sites import attention_sites, replace_sites, select_by_layers


def insert_reference(gm: fx.GraphModule, reference_layers: Sequence[str]) -> int:
    """Rewrite the selected sites and install the state as `gm.reference` (chunks 0: ordinary attention); returns the number of sites."""
    chosen, reference_layers = select_by_layers(attention_sites(gm, "attn1"), reference_layers, "reference_layers")
    return replace_sites(gm, chosen, "reference", ReferenceRows([p for _, p in chosen], reference_layers), attention_reference_wrapper)
