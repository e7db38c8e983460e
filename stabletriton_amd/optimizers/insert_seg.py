"""Smoothed-energy sites (addition; seg.py): `attention_wrapper` -> `attention_seg_wrapper` at the selected self-attentions.

insert_pag's site rule: the pass runs directly after fuse_attention, while the projections are still call_module nodes whose targets
spell the module path; a candidate is an `attention_wrapper` whose query is the output of a module `<path>.attn1.to_q`, and
`<path>.attn1` is matched against `seg_layers`, every entry a regular expression `re.search`ed against that path ("mid" selects
every attn1 under `mid_block`).  An entry that selects no self-attention raises ValueError; cross-attention is never a candidate.

Only the leaf changes: q, k and v stay the three projections of one input, so the later passes (the fused q|k|v projection,
LayerNorm folding, the strict split images, the fp8 plan) fire on these sites exactly as without the pass.  A site carries one
leaf, and SEG and PAG both claim the perturbed row block: `seg_layers` together with `pag_layers` is refused by the callers
(optimization.replace_backend).
"""
from __future__ import annotations

from typing import Sequence

from torch import fx

from ..seg import SEG, attention_seg_wrapper
from .attention_sites import attention_sites, replace_sites, select_by_layers


def insert_seg(gm: fx.GraphModule, seg_layers: Sequence[str]) -> int:
    """Rewrite the selected sites and install the state as `gm.seg` (chunks 0: ordinary attention); returns the number of sites."""
    chosen, seg_layers = select_by_layers(attention_sites(gm, "attn1"), seg_layers, "seg_layers")
    return replace_sites(gm, chosen, "seg", SEG([p for _, p in chosen], seg_layers), attention_seg_wrapper)
