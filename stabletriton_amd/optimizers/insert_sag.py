"""The self-attention guidance site (addition; sag.py): `attention_wrapper` -> `attention_sag_wrapper` at ONE self-attention.

insert_pag's site rule: the pass runs directly after fuse_attention, while the projections are still call_module nodes whose targets
spell the module path; a candidate is an `attention_wrapper` whose query is the output of a module `<path>.attn1.to_q`.  `sag_layer`
is True - the first `attn1` of the middle block, ComfyUI's site - or one regular expression `re.search`ed against `<path>.attn1` that
must select exactly one candidate: the guidance thresholds one attention map.  Zero or several matches raise ValueError;
cross-attention is never a candidate.

Only the leaf changes: q, k and v stay the three projections of one input, so the later passes (the fused q|k|v projection, LayerNorm
folding, the strict split images) fire on the site exactly as without the pass, and the leaf reads q and k where that projection
leaves them.
"""
from __future__ import annotations

from torch import fx

from ..sag import DEFAULT_SITE, SAG, attention_sag_wrapper
from .attention_sites import attention_sites, replace_sites, select_by_layers


def insert_sag(gm: fx.GraphModule, sag_layer=True) -> int:
    """Rewrite the site and install the state as `gm.sag` (rows 0: ordinary attention); returns the number of sites, 1."""
    if sag_layer is True:
        sag_layer = DEFAULT_SITE
    if not isinstance(sag_layer, str) or not sag_layer:
        raise ValueError(f"sag_layer: True (the middle block's first self-attention) or one regular expression expected, got {sag_layer!r}")
    chosen, _ = select_by_layers(attention_sites(gm, "attn1"), (sag_layer,), "sag_layer")
    if len(chosen) != 1:
        raise ValueError(f"sag_layer: {sag_layer!r} selects {len(chosen)} self-attentions ({[p for _, p in chosen][:4]}"
                         f"{' ...' if len(chosen) > 4 else ''}); self-attention guidance reads exactly one")
    return replace_sites(gm, chosen, "sag", SAG(chosen[0][1], sag_layer), attention_sag_wrapper)
