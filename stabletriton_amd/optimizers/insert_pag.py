"""Perturbed-attention sites (addition; pag.py): `attention_wrapper` -> `attention_pag_wrapper` at the selected self-attentions.

Runs directly after fuse_attention, while the projections are still call_module nodes whose targets spell the module path: a
candidate is an `attention_wrapper` whose query is the output of a module `<path>.attn1.to_q` (self-attention; the classes of the
modules are never looked at, and a prefix in front of the block names - the ComfyUI entry wraps the network as `unet.` - does not
matter).  `<path>.attn1` is matched against `pag_layers`: every entry is a regular expression, `re.search`ed against that path
(the rule of current diffusers' `pag_applied_layers`), so "mid" selects every attn1 under `mid_block`, "down_blocks.2" the third
encoder stage, "blocks.(0|1)" both sides' first two stages.  An entry that selects no self-attention raises ValueError;
cross-attention (`attn2`) is never a candidate.

Only the leaf changes: q, k and v stay the three projections of one input, so the later passes (the fused q|k|v projection,
LayerNorm folding, the strict split images, the fp8 plan) fire on these sites exactly as without the pass.
"""
from __future__ import annotations

import re
from typing import Sequence

from torch import fx

from ..pag import PAG, attention_pag_wrapper
from .wrappers import attention_wrapper

_SELF_QUERY = re.compile(r"^(.*(?:^|\.)attn1)\.to_q$")


def _attn1_path(att: fx.Node):
    """Module path of the self-attention whose to_q feeds `att`'s query, else None."""
    q = att.args[0]
    if not (isinstance(q, fx.Node) and q.op == "call_module"):
        return None
    m = _SELF_QUERY.match(str(q.target))
    return m.group(1) if m else None


def insert_pag(gm: fx.GraphModule, pag_layers: Sequence[str]) -> int:
    """Rewrite the selected sites and install the state as `gm.pag` (chunks 0: ordinary attention); returns the number of sites."""
    if isinstance(pag_layers, str):
        pag_layers = (pag_layers,)
    pag_layers = tuple(pag_layers)
    if not pag_layers or not all(isinstance(p, str) and p for p in pag_layers):
        raise ValueError(f"pag_layers: a non-empty sequence of regular expressions (e.g. (\"mid\",)) expected, got {pag_layers!r}")
    patterns = [re.compile(p) for p in pag_layers]
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
    missed = [pag_layers[i] for i, h in enumerate(hit) if not h]
    if missed:
        raise ValueError(f"pag_layers: {missed} match no self-attention (attn1) of this UNet; its self-attentions are "
                         f"{[p for _, p in candidates][:4]}{' ...' if len(candidates) > 4 else ''}")
    gm.add_submodule("pag", PAG([p for _, p in chosen], pag_layers))
    for n, _ in chosen:
        with gm.graph.inserting_before(n):
            state = gm.graph.get_attr("pag")
            new = gm.graph.call_function(attention_pag_wrapper, tuple(n.args) + (state,))
        n.replace_all_uses_with(new)
        gm.graph.erase_node(n)
    gm.graph.lint()
    gm.recompile()
    return len(chosen)
