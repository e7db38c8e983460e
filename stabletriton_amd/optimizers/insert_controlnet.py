"""ControlNet residual sites (addition; controlnet.py): one `controlnet_sites(mid, skips, state)` leaf behind the middle block, read
by the decoder only.

Runs first, on the freshly traced graph, while the call_module nodes still spell the module paths (a prefix in front of
`down_blocks`, as the ComfyUI entry's `unet.`, does not matter; module classes are never looked at).  The skip values are, in
encoder order, the output of `conv_in`, per down block each resnet's output (behind its attention where the level has one) and
each downsampler's output: the module paths give their names, channel counts and levels, and the SECOND part of each decoder
concatenation - read last-first - gives the values themselves.  The middle site is the first part of the first decoder
concatenation.

Only the decoder's concatenations are rewired to the leaf - and through them norm1, the 1x1 shortcut and FreeU's sites, which
insert_freeu places afterwards.  The encoder's readers of a skip tensor keep the original node: diffusers adds a ControlNet's
residuals to the collected skips after the encoder has run, and on the device the leaf writes in place only once every one of
those readers has been launched.  fuse_groupnorm_stats takes an output of the leaf as a producer and hands the leaf the inner
producer's partials, which the kernel rewrites.
"""
from __future__ import annotations

import operator
import re

import torch
from torch import fx

from ..controlnet import ControlNetState, controlnet_sites

_CONV_IN = re.compile(r"(?:^|\.)conv_in$")
_DOWN_RES = re.compile(r"(?:^|\.)down_blocks\.(\d+)\.resnets\.(\d+)\.conv2$")
_DOWN_ATT = re.compile(r"(?:^|\.)down_blocks\.(\d+)\.attentions\.(\d+)\.proj_out$")
_DOWN_CONV = re.compile(r"(?:^|\.)down_blocks\.(\d+)\.downsamplers\.0\.conv$")
_UP_RES = re.compile(r"(?:^|\.)up_blocks\.\d+\.resnets\.\d+\.")


def decoder_cats(gm: fx.GraphModule):
    """The decoder's skip concatenations in graph order: two tensors along the channels, read by an up block's resnet only."""
    cats = []
    for n in gm.graph.nodes:
        if not (n.op == "call_function" and n.target in (torch.cat, torch.concat)):
            continue
        parts = n.args[0] if n.args else n.kwargs.get("tensors")
        dim = n.kwargs.get("dim", n.args[1] if len(n.args) > 1 else 0)
        if dim != 1 or not isinstance(parts, (list, tuple)) or len(parts) != 2 or not all(isinstance(p, fx.Node) for p in parts):
            continue
        if n.users and all(u.op == "call_module" and _UP_RES.search(str(u.target)) for u in n.users):
            cats.append(n)
    return cats


def find_sites(gm: fx.GraphModule):
    """([(name, channels, latent halvings)] in site order - the skips in encoder order, the middle block last -, the decoder's
    concatenations in graph order)."""
    mods = dict(gm.named_modules())
    conv_in = next((name for name in mods if _CONV_IN.search(name)), None)
    res, att, down = {}, set(), {}
    for name, mod in mods.items():
        m = _DOWN_RES.search(name)
        if m:
            res[(int(m.group(1)), int(m.group(2)))] = int(mod.out_channels)
        m = _DOWN_ATT.search(name)
        if m:
            att.add((int(m.group(1)), int(m.group(2))))
        m = _DOWN_CONV.search(name)
        if m:
            down[int(m.group(1))] = int(mod.out_channels)
    if conv_in is None or not res:
        raise ValueError("controlnet: the traced module does not spell diffusers' conv_in / down_blocks paths; the sites cannot be placed")
    sites = [("conv_in", int(mods[conv_in].out_channels), 0)]
    for i in range(max(b for b, _ in res) + 1):
        for j in sorted(r for b, r in res if b == i):
            what = "attentions" if (i, j) in att else "resnets"
            sites.append((f"down_blocks.{i}.{what}.{j}", res[(i, j)], i))
        if i in down:
            sites.append((f"down_blocks.{i}.downsamplers.0", down[i], i + 1))
    cats = decoder_cats(gm)
    if len(cats) != len(sites):
        raise ValueError(f"controlnet: the encoder emits {len(sites)} skip tensors but the decoder has {len(cats)} skip concatenations; "
                         "the sites cannot be placed")
    sites.append(("mid_block", sites[-1][1], sites[-1][2]))
    return sites, cats


def insert_controlnet(gm: fx.GraphModule) -> int:
    """Place the leaf and install the state (scale 0 = off, nothing bound) as `gm.controlnet`; returns the number of sites."""
    sites, cats = find_sites(gm)
    part = lambda cat, i: (cat.args[0] if cat.args else cat.kwargs["tensors"])[i]
    mid = part(cats[0], 0)
    skips = [part(cat, 1) for cat in reversed(cats)]            # the decoder pops: its first concatenation reads the last skip
    if len(set(skips)) != len(skips) or mid in skips:
        raise ValueError("controlnet: a skip tensor is read by two decoder concatenations; the sites cannot be placed")
    order = {n: i for i, n in enumerate(gm.graph.nodes)}
    if any(order[s] > order[mid] for s in skips):
        raise ValueError("controlnet: a skip tensor is produced behind the middle block; the sites cannot be placed")
    p = next(gm.parameters(), None)
    gm.add_submodule("controlnet", ControlNetState(sites, dtype=p.dtype if p is not None else None))
    n = len(sites)
    with gm.graph.inserting_after(mid):
        state = gm.graph.get_attr("controlnet")
    with gm.graph.inserting_after(state):
        leaf = gm.graph.call_function(controlnet_sites, (mid, skips, state))
    at, outs = leaf, []
    for k in range(n):
        with gm.graph.inserting_after(at):
            at = gm.graph.call_function(operator.getitem, (leaf, k))
        outs.append(at)
    for j, cat in enumerate(cats):                              # ONLY the decoder's readers: the encoder's keep the original nodes
        new = [outs[n - 1] if j == 0 else part(cat, 0), outs[n - 2 - j]]
        if cat.args:
            cat.args = (new,) + tuple(cat.args[1:])
        else:
            cat.kwargs = {**cat.kwargs, "tensors": new}
    gm.graph.lint()
    gm.recompile()
    return n
