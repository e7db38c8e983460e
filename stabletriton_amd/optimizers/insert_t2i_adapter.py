"""T2I-Adapter residual sites (addition; t2i_adapter.py): `v` -> `t2i_site(v, state, k)` at one place per down block and behind the
middle block.

Runs first, on the freshly traced graph, while the call_module nodes still spell the module paths (a prefix in front of
`down_blocks`, as the ComfyUI entry's `unet.`, does not matter; module classes are never looked at).  diffusers' rule for
`down_intrablock_additional_residuals`:

  site A      the output of `down_blocks.0.downsamplers.0.conv`;
  sites B, C  block i >= 1: its output after the last attention and before its downsampler - in the graph the value that feeds
              `down_blocks.i.downsamplers.0.conv`, or `mid_block.resnets.0.norm1` for the last block;
  site M      the `mid_block` output: the first half of the first decoder concatenation.

EVERY user of the value behind a site is rewired to the site - the skip connection, the next resnet's norm and its shortcut:
diffusers' skip tensors carry the residual too, and the device kernel adds in place.  fuse_groupnorm_stats then takes the site as
the producer of its output and hands it the inner producer's partials (`src_stats`), which the kernel rewrites: fuse_skip_cat
still removes the concatenations and no GroupNorm falls back to a statistics pass.
"""
from __future__ import annotations

import re

from torch import fx

from ..t2i_adapter import T2IAdapterState, t2i_site
from .insert_controlnet import decoder_cats

_DOWN_CONV = re.compile(r"(?:^|\.)down_blocks\.(\d+)\.downsamplers\.0\.conv$")
_DOWN_RES = re.compile(r"(?:^|\.)down_blocks\.(\d+)\.resnets\.(\d+)\.")
_MID_IN = re.compile(r"(?:^|\.)mid_block\.resnets\.0\.norm1$")


def find_sites(gm: fx.GraphModule):
    """[(name, value node, channels, latent halvings, ComfyUI input-block index or None)] in site order."""
    mods = dict(gm.named_modules())
    down_convs, mid_in, n_res = {}, None, {}
    for n in gm.graph.nodes:
        if n.op != "call_module":
            continue
        m = _DOWN_CONV.search(str(n.target))
        if m:
            down_convs[int(m.group(1))] = n
        elif _MID_IN.search(str(n.target)) and mid_in is None:
            mid_in = n
    for name in mods:
        m = _DOWN_RES.search(name + ".")
        if m:
            i = int(m.group(1))
            n_res[i] = max(n_res.get(i, 0), int(m.group(2)) + 1)
    blocks = max(n_res) + 1 if n_res else 0
    if blocks < 2 or 0 not in down_convs or mid_in is None:
        raise ValueError("t2i_adapter: the traced module does not spell diffusers' down_blocks / mid_block paths; the sites cannot be placed")
    # ComfyUI's input blocks: conv_in, then per down block its resnets (+ attention) one by one and its downsampler
    base, at = {}, 1
    for i in range(blocks):
        base[i] = at
        at += n_res.get(i, 0) + (1 if i in down_convs else 0)
    sites = []
    conv0 = down_convs[0]
    sites.append(("down_blocks.0.downsamplers.0", conv0, mods[conv0.target].out_channels, 1, base[0] + n_res[0]))
    for i in range(1, blocks):
        reader = down_convs.get(i) if i < blocks - 1 else mid_in
        if reader is None or not isinstance(reader.args[0], fx.Node):
            raise ValueError(f"t2i_adapter: down_blocks.{i} has no downsampler / middle-block reader to place its site at")
        mod = mods[reader.target]
        ch = mod.in_channels if hasattr(mod, "in_channels") else mod.num_channels
        sites.append((f"down_blocks.{i}", reader.args[0], int(ch), i, base[i] + n_res[i] - 1))
    cat = next(iter(decoder_cats(gm)), None)             # the decoder's skip concatenations in graph order: the first reads the middle block
    if cat is None:
        raise ValueError("t2i_adapter: no decoder concatenation behind the middle block; the middle site cannot be placed")
    mid = cat.args[0][0] if cat.args else cat.kwargs["tensors"][0]
    sites.append(("mid_block", mid, sites[-1][2], blocks - 1, None))
    return sites


def insert_t2i_adapter(gm: fx.GraphModule) -> int:
    """Place the sites and install the state (scale 0 = off, nothing bound) as `gm.t2i_adapter`; returns the number of sites."""
    found = find_sites(gm)
    p = next(gm.parameters(), None)
    gm.add_submodule("t2i_adapter", T2IAdapterState([(name, ch, lvl, blk) for name, _, ch, lvl, blk in found],
                                                    dtype=p.dtype if p is not None else None))
    for k, (_, value, _, _, _) in enumerate(found):
        with gm.graph.inserting_after(value):
            state = gm.graph.get_attr("t2i_adapter")
        with gm.graph.inserting_after(state):
            site = gm.graph.call_function(t2i_site, (value, state, k))
        value.replace_all_uses_with(site, delete_user_cb=lambda u, site=site: u is not site)
    gm.graph.lint()
    gm.recompile()
    return len(found)
