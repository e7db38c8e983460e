"""Token-merging sites (addition; tome.py): the first half of the selected transformer blocks runs on N - r merged tokens.

Runs directly after fuse_attention, ahead of the other site passes (none of which may be combined with it) and by their rules: a
candidate is an `attention_wrapper` whose query is the output of a module `<path>.attn1.to_q`; `<path>.attn1` is matched against `tome_layers`, every entry a regular expression
`re.search`ed against that path.  An entry that selects no self-attention raises ValueError; cross-attention is never a candidate.

Unlike those passes this one changes more than the leaf.  The site is `x + to_out(attention(to_q(n), to_k(n), to_v(n)))`, n = norm1(x):
    plan = tome_plan_wrapper(x, state)                    match + select on the pre-norm x
    n    = tome_merge_wrapper(x, norm1, plan)             in place of the norm1 call: (B, N - r, C)
    ...  to_q / to_k / to_v / attention_wrapper / to_out  untouched, now on N - r rows
    out  = tome_unmerge_wrapper(to_out(...), x, plan)     in place of the add
so the later passes still fuse q|k|v into one GEMM (three projections of one node), while neither the LayerNorm fold (norm1 is no
`layer_norm_wrapper` any more) nor a residual fusion (there is no add) fires on the site; norm2's fold takes its row partials from the
unmerge leaf (fuse_layernorm_into_linear knows it as a producer).  A site whose graph is not that chain raises: nothing is skipped
silently.
"""
from __future__ import annotations

import operator
from typing import Sequence

import torch
from torch import fx, nn

from ..tome import ToMe, tome_merge_wrapper, tome_plan_wrapper, tome_unmerge_wrapper
from .attention_sites import attention_sites, select_by_layers


def _module_call(gm: fx.GraphModule, n, cls) -> bool:
    return isinstance(n, fx.Node) and n.op == "call_module" and isinstance(gm.get_submodule(n.target), cls)


def insert_tome(gm: fx.GraphModule, tome_layers: Sequence[str], ratio: float = 0.5) -> int:
    """Rewrite the selected sites and install the state as `gm.tome` (outside `using`: the unmerged chain); returns the number of sites."""
    chosen, tome_layers = select_by_layers(attention_sites(gm, "attn1"), tome_layers, "tome_layers")
    gm.add_submodule("tome", ToMe([p for _, p in chosen], tome_layers, ratio))
    for att, path in chosen:
        q, k, v = att.args[:3]
        ln = q.args[0]
        ok = (_module_call(gm, ln, nn.LayerNorm) and all(_module_call(gm, p, nn.Linear) and p.args[0] is ln for p in (q, k, v))
              and set(ln.users) == {q, k, v} and len(att.users) == 1)
        out = next(iter(att.users)) if ok else None
        ok = ok and _module_call(gm, out, nn.Linear) and len(out.users) == 1
        add = next(iter(out.users)) if ok else None
        x = ln.args[0] if ok else None
        ok = ok and add.op == "call_function" and add.target in (operator.add, torch.add) and len(add.args) == 2 and not add.kwargs \
            and set(add.args) == {out, x}
        if not ok:
            raise ValueError(f"tome_layers: the self-attention {path} is not the chain x + to_out(attention(q|k|v of norm1(x))): the site "
                             "cannot be rewritten")
        with gm.graph.inserting_before(ln):
            state = gm.graph.get_attr("tome")
            plan = gm.graph.call_function(tome_plan_wrapper, (x, state))
            merged = gm.graph.call_function(tome_merge_wrapper, (x, gm.graph.get_attr(ln.target), plan))
        ln.replace_all_uses_with(merged)
        gm.graph.erase_node(ln)
        with gm.graph.inserting_before(add):
            new = gm.graph.call_function(tome_unmerge_wrapper, (out, x, plan))
        add.replace_all_uses_with(new)
        gm.graph.erase_node(add)
    gm.graph.lint()
    gm.recompile()
    return len(chosen)
