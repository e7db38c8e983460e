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

from typing import Sequence

from torch import fx

from ..pag import PAG, attention_pag_wrapper
from .attention_sites import attention_sites, replace_sites, select_by_layers


def insert_pag(gm: fx.GraphModule, pag_layers: Sequence[str]) -> int:
    """Rewrite the selected sites and install the state as `gm.pag` (chunks 0: ordinary attention); returns the number of sites."""
    chosen, pag_layers = select_by_layers(attention_sites(gm, "attn1"), pag_layers, "pag_layers")
    return replace_sites(gm, chosen, "pag", PAG([p for _, p in chosen], pag_layers), attention_pag_wrapper)
