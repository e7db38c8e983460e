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

import re
from typing import Sequence

from torch import fx

from ..seg import SEG, attention_seg_wrapper
from .insert_pag import _attn1_path
from .wrappers import attention_wrapper


def insert_seg(gm: fx.GraphModule, seg_layers: Sequence[str]) -> int:
    """Rewrite the selected sites and install the state as `gm.seg` (chunks 0: ordinary attention); returns the number of sites."""
    if isinstance(seg_layers, str):
        seg_layers = (seg_layers,)
    seg_layers = tuple(seg_layers)
    if not seg_layers or not all(isinstance(p, str) and p for p in seg_layers):
        raise ValueError(f"seg_layers: a non-empty sequence of regular expressions (e.g. (\"mid\",)) expected, got {seg_layers!r}")
    patterns = [re.compile(p) for p in seg_layers]
    candidates = [(n, path) for n in gm.graph.nodes
                  if n.op == "call_function" and n.target is attention_wrapper and not n.kwargs
                  for path in (_attn1_path(n),) if path is not None]
    hit = [False] * len(patterns)
    chosen = []
    for n, path in candidates:
        found = [i for i, p in enumerate(patterns) if p.search(path)]
        for i in found:
            hit[i] = True
        if found:
            chosen.append((n, path))
    missed = [seg_layers[i] for i, h in enumerate(hit) if not h]
    if missed:
        raise ValueError(f"seg_layers: {missed} match no self-attention (attn1) of this UNet; its self-attentions are "
                         f"{[p for _, p in candidates][:4]}{' ...' if len(candidates) > 4 else ''}")
    gm.add_submodule("seg", SEG([p for _, p in chosen], seg_layers))
    for n, _ in chosen:
        with gm.graph.inserting_before(n):
            state = gm.graph.get_attr("seg")
            new = gm.graph.call_function(attention_seg_wrapper, tuple(n.args) + (state,))
        n.replace_all_uses_with(new)
        gm.graph.erase_node(n)
    gm.graph.lint()
    gm.recompile()
    return len(chosen)
