"""FreeU sites (addition; freeu.py): `cat([h, r], 1)` -> `cat([h', r'], 1)` at the decoder's first two stages.

Runs first, on the freshly traced graph, while the readers of every concatenation are still call_module nodes whose
targets spell the module path: a site is a two-tensor channel concatenation all of whose module readers live under
`up_blocks.<i>.resnets.<j>` for one stage index i in {0, 1} (diffusers' `resolution_idx` rule; the reference's
unet_pt.py:349-357 uses the same names).  The classes of the modules are never looked at, and a prefix in front of
`up_blocks` (the ComfyUI entry wraps the network as `unet.`) does not matter.  Stage 0 reads (b1, s1), stage 1 (b2, s2).

The node returns (h', r', statistics of h', statistics of r'): fuse_groupnorm_stats takes the last two as the
producers' partials, so fuse_skip_cat still removes the concatenation and no site falls back to a statistics pass.
"""
from __future__ import annotations

import operator
import re

import torch
from torch import fx

from ..freeu import FreeU, freeu_wrapper

_READER = re.compile(r"(?:^|\.)up_blocks\.(\d+)\.resnets\.\d+\.")


def _stage_of(cat: fx.Node):
    """Decoder stage index when every module reader of `cat` belongs to resnets of one stage, else None."""
    stages = set()
    for u in cat.users:
        if u.op != "call_module":
            return None
        m = _READER.search(str(u.target))
        if m is None:
            return None
        stages.add(int(m.group(1)))
    return stages.pop() if len(stages) == 1 else None


def insert_freeu(gm: fx.GraphModule, device=None) -> int:
    """Rewrite the sites and install the (neutral) parameter state as `gm.freeu`; returns the number of sites."""
    if device is None:
        p = next(gm.parameters(), None)
        device = p.device if p is not None else None
    gm.add_submodule("freeu", FreeU(device))
    count = 0
    for n in list(gm.graph.nodes):
        if not (n.op == "call_function" and n.target in (torch.cat, torch.concat)):
            continue
        parts = n.args[0] if n.args else n.kwargs.get("tensors")
        dim = n.kwargs.get("dim", n.args[1] if len(n.args) > 1 else 0)
        if dim != 1 or not isinstance(parts, (list, tuple)) or len(parts) != 2:
            continue
        stage = _stage_of(n)
        if stage not in (0, 1):
            continue
        with gm.graph.inserting_before(n):
            state = gm.graph.get_attr("freeu")
            site = gm.graph.call_function(freeu_wrapper, (parts[0], parts[1], state, stage))
            h2 = gm.graph.call_function(operator.getitem, (site, 0))
            r2 = gm.graph.call_function(operator.getitem, (site, 1))
        n.args = ([h2, r2],) + tuple(n.args[1:])
        count += 1
    gm.graph.lint()
    gm.recompile()
    return count
