"""What the site passes on `attention_wrapper` share (insert_pag, insert_seg, insert_regions, insert_ip_adapter): finding the self- or
cross-attention sites by the module path of their query projection, selecting some by regular expressions, and putting another leaf
with the feature's state in their place."""
from __future__ import annotations

import re
from typing import Callable, List, Sequence, Tuple

from torch import fx, nn

from .wrappers import attention_wrapper


def attention_sites(gm: fx.GraphModule, kind: str) -> List[Tuple[fx.Node, str]]:
    """(node, `<path>.<kind>`) of every `attention_wrapper` whose query is the output of a module `<path>.<kind>.to_q`;
    kind "attn1": the self-attentions, "attn2": the cross-attentions."""
    query = re.compile(rf"^(.*(?:^|\.){kind})\.to_q$")
    out = []
    for n in gm.graph.nodes:
        if n.op == "call_function" and n.target is attention_wrapper and not n.kwargs:
            q = n.args[0]
            m = query.match(str(q.target)) if isinstance(q, fx.Node) and q.op == "call_module" else None
            if m:
                out.append((n, m.group(1)))
    return out


def select_by_layers(candidates: Sequence[Tuple[fx.Node, str]], layers, flag_name: str):
    """-> (the candidates whose path some entry of `layers` `re.search`es, layers as a tuple); every entry must select one."""
    if isinstance(layers, str):
        layers = (layers,)
    layers = tuple(layers)
    if not layers or not all(isinstance(p, str) and p for p in layers):
        raise ValueError(f"{flag_name}: a non-empty sequence of regular expressions (e.g. (\"mid\",)) expected, got {layers!r}")
    patterns = [re.compile(p) for p in layers]
    hit = [False] * len(patterns)
    chosen = []
    for n, path in candidates:
        found = [i for i, p in enumerate(patterns) if p.search(path)]
        for i in found:
            hit[i] = True
        if found:
            chosen.append((n, path))
    missed = [layers[i] for i, h in enumerate(hit) if not h]
    if missed:
        raise ValueError(f"{flag_name}: {missed} match no self-attention (attn1) of this UNet; its self-attentions are "
                         f"{[p for _, p in candidates][:4]}{' ...' if len(candidates) > 4 else ''}")
    return chosen, layers


def replace_sites(gm: fx.GraphModule, chosen: Sequence[Tuple[fx.Node, str]], attr: str, state: nn.Module, leaf: Callable,
                  extra: Callable = lambda i: ()) -> int:
    """Install `state` as `gm.<attr>` and put `leaf(*args, state, *extra(i))` in place of the i-th chosen node; returns their number."""
    gm.add_submodule(attr, state)
    for i, (n, _) in enumerate(chosen):
        with gm.graph.inserting_before(n):
            new = gm.graph.call_function(leaf, tuple(n.args) + (gm.graph.get_attr(attr),) + tuple(extra(i)))
        n.replace_all_uses_with(new)
        gm.graph.erase_node(n)
    gm.graph.lint()
    gm.recompile()
    return len(chosen)
