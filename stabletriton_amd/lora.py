"""LoRA adapters, merged into the weights in place.

A step of the compiled UNet is launch-bound, so an adapter never runs as a side branch here: it is merged into the
`nn.Linear` weights the kernels already read, and a merged weight adds no launch.  Every merge REBUILDS the weight from a
snapshot of its base,

    W = round_to_dtype( fp32(Base) + sum_j scale_j * (Up_j @ Down_j) ),        Up_j = (alpha_j / rank_j) * up_j, folded at load

in one grouped launch over all adapted modules (`ops.lora_merge`, csrc/lora.hip).  Rebuilding instead of adding and
subtracting is what makes `unload` restore the base bit for bit, scale 0 equal the base, and a scale change free of drift in
16-bit models.  The weights keep their addresses, so captured graphs stay valid; the owner re-derives what was computed
from them (fused q|k|v, LayerNorm-folded projections, split images, the fp8 plan's e4m3 weights: `refresh_derived`).

`parse_lora_state_dict` reads the three spellings in the wild (PEFT / current diffusers, older diffusers, kohya);
`LoraSet` owns the state of one module; `attach(compiled)` returns the set of an `optimize_model` result.
`DenoiseLoop.load_lora` and the hooks' `load_lora` are thin wrappers over it.

Scope: `nn.Linear` targets only (attention projections, feed-forward, proj_in / proj_out, and the time-path Linears when an
adapter names them).  Convolution adapters (LoCon / LyCORIS), DoRA and text-encoder adapters are reported, not applied.
"""
from __future__ import annotations

import re
from collections import OrderedDict
from typing import Callable, Dict, Iterable, List, Mapping, Optional, Tuple

import torch
from torch import nn

MAX_ADAPTERS = 8        # capacity of a LoraSet: the device scale table has this many slots and never moves
MAX_RANK = 128          # largest rank of one adapter on one module

_TEXT_ENCODER = re.compile(r"^(lora_te\d*_|text_encoder(_\d+)?\.|te\d*\.|lora_prior_te)")
_PEFT = re.compile(r"^(?P<path>.+)\.lora_(?P<ab>[AB])(?:\.[^.]+)?\.weight$")
_OLD_PROC = re.compile(r"^(?P<attn>.+?)\.(?:processor\.)?(?P<proj>to_q|to_k|to_v|to_out)_lora\.(?P<du>down|up)\.weight$")
_OLD_LAYER = re.compile(r"^(?P<path>.+)\.lora(?:_layer)?\.(?P<du>down|up)\.weight$")
_KOHYA = re.compile(r"^(?P<stem>lora_unet_[^.]+)\.(?P<what>lora_down\.weight|lora_up\.weight|alpha)$")


def is_text_encoder_key(key: str) -> bool:
    return _TEXT_ENCODER.match(key) is not None


def _place(key: str, flat: Mapping[str, str], names) -> Optional[Tuple[str, str]]:
    """(module name, 'down' | 'up' | 'alpha') for one state-dict key, or None when the key names no target."""
    m = _KOHYA.match(key)
    if m:
        name = flat.get(m["stem"][len("lora_unet_"):])
        what = {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha"}[m["what"]]
        return (name, what) if name is not None else None
    if key.startswith("unet."):
        key = key[len("unet."):]
    m = _PEFT.match(key)
    if m:
        return (m["path"], "down" if m["ab"] == "A" else "up") if m["path"] in names else None
    m = _OLD_PROC.match(key)
    if m:
        path = f"{m['attn']}.{m['proj']}" + (".0" if m["proj"] == "to_out" else "")
        return (path, m["du"]) if path in names else None
    m = _OLD_LAYER.match(key)
    if m:
        return (m["path"], m["du"]) if m["path"] in names else None
    if key.endswith(".alpha") and key[:-len(".alpha")] in names:
        return key[:-len(".alpha")], "alpha"
    return None


def parse_lora_state_dict(sd: Mapping[str, torch.Tensor], module_names: Iterable[str]):
    """Place a LoRA state dict on the modules named by `module_names` (the model's own `nn.Linear` names).

    Returns `(placed, unplaced)`: `placed[name] = (down (r, K), up (N, r), alpha)`, `unplaced` the keys that name no target
    (convolutions, other networks, text encoders - `is_text_encoder_key` tells the latter apart).  Spellings:
      PEFT / diffusers      <path>.lora_A.weight, <path>.lora_B.weight  [, <path>.alpha]
      older diffusers       <attn>.to_q_lora.down.weight / .up.weight, with or without `.processor`; <path>.lora.down.weight
      kohya                 lora_unet_<path with underscores>.lora_down.weight / .lora_up.weight / .alpha
    An optional `unet.` prefix is dropped.  kohya's underscores are resolved against the module names themselves
    (`name.replace(".", "_")`), never by guessing where the dots were.  `alpha` defaults to the rank."""
    names = set(module_names)
    flat: Dict[str, str] = {}
    for n in names:
        f = n.replace(".", "_")
        if f in flat:
            raise ValueError(f"modules {flat[f]!r} and {n!r} have the same kohya name {f!r}")
        flat[f] = n
    parts: Dict[str, Dict[str, torch.Tensor]] = {}
    unplaced: List[str] = []
    for key, val in sd.items():
        hit = None if is_text_encoder_key(key) else _place(key, flat, names)
        if hit is None:
            unplaced.append(key)
            continue
        name, what = hit
        slot = parts.setdefault(name, {})
        if what in slot:
            raise ValueError(f"{name}: the state dict holds two {what} entries (the second is {key!r})")
        slot[what] = val
    placed = {}
    for name, p in parts.items():
        if "down" not in p or "up" not in p:
            raise ValueError(f"{name}: incomplete adapter, found only {sorted(p)}")
        down, up = p["down"], p["up"]
        if down.dim() == 4 and tuple(down.shape[2:]) == (1, 1) and up.dim() == 4 and tuple(up.shape[2:]) == (1, 1):
            down, up = down[:, :, 0, 0], up[:, :, 0, 0]          # a Linear that another exporter wrote as a 1x1 convolution
        alpha = float(p["alpha"]) if "alpha" in p else float(down.shape[0])
        placed[name] = (down, up, alpha)
    return placed, unplaced


def check_shapes(name: str, weight_shape, down: torch.Tensor, up: torch.Tensor) -> int:
    """up is (N, r), down is (r, K), r at most MAX_RANK; returns r."""
    n, k = weight_shape
    if down.dim() != 2 or up.dim() != 2:
        raise ValueError(f"{name}: LoRA factors must be 2-D, got down {tuple(down.shape)} and up {tuple(up.shape)}")
    r = down.shape[0]
    if r < 1 or r > MAX_RANK:
        raise ValueError(f"{name}: rank {r} is outside 1 .. {MAX_RANK}")
    if tuple(down.shape) != (r, k) or tuple(up.shape) != (n, r):
        raise ValueError(f"{name}: a ({n}, {k}) weight takes down ({r}, {k}) and up ({n}, {r}); got down {tuple(down.shape)} "
                         f"and up {tuple(up.shape)}")
    return r


def target_linears(module: nn.Module) -> "OrderedDict[str, nn.Linear]":
    """The module's `nn.Linear` submodules under the names an adapter uses.  A compiled module also holds its hoisted
    context / time sub-graphs, which reference the same Linear objects: each object is listed once, under its first (own)
    name.  A wrapper that keeps the network in `.unet` (the label-vector entry) does not add its prefix."""
    out = OrderedDict()
    for name, m in module.named_modules():
        if isinstance(m, nn.Linear):
            out[name[len("unet."):] if name.startswith("unet.") else name] = m
    return out


class _Adapter:
    def __init__(self, slot: int, scale: float):
        self.slot, self.scale = slot, scale
        self.factors: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}      # module -> (Up (N, rp), DownT (K, rp)), zero-padded ranks


class LoraSet:
    """The adapters of ONE module (an `optimize_model` result or the plain `nn.Module`).  Up to MAX_ADAPTERS at once.

    On the GPU every change is one launch of the grouped merge kernel over all adapted weights; on the CPU the same formula
    runs in torch (fp32), so host tests and tools work.  After a merge the version counter of every rewritten parameter is
    bumped (the kernel writes through raw pointers) and `on_change()` runs: by default the module's
    `exec_context.refresh_derived(full=True)`.  Owners that cache more than derived weights (hoisted text K/V, time tables)
    re-derive those themselves after calling in here (`DenoiseLoop.load_lora`, the hooks' `load_lora`).

    Memory: one snapshot per ADAPTED weight (taken when the first adapter touches it, freed when the last one leaves) plus the
    factors."""

    def __init__(self, module: nn.Module, on_change: Optional[Callable[[], object]] = None):
        self.module = module
        self.linears = target_linears(module)
        if not self.linears:
            raise ValueError("LoraSet: the module has no nn.Linear to adapt")
        ectx = getattr(module, "exec_context", None)
        self.on_change = on_change if on_change is not None else ((lambda: ectx.refresh_derived(full=True)) if ectx is not None else None)
        self._adapters: "OrderedDict[str, _Adapter]" = OrderedDict()
        self._base: Dict[str, torch.Tensor] = {}
        self._global = 1.0                   # diffusers' cross_attention_kwargs scale: one multiplier over every adapter
        self._scales: Optional[torch.Tensor] = None      # device table, MAX_ADAPTERS floats, allocated once
        self._plan = None
        self.last_unplaced: List[str] = []

    # ---- queries -------------------------------------------------------------------------------
    def names(self) -> List[str]:
        return list(self._adapters)

    def scales(self) -> Dict[str, float]:
        return {n: a.scale for n, a in self._adapters.items()}

    def adapted_modules(self) -> List[str]:
        return list(self._base)

    @property
    def global_scale(self) -> float:
        return self._global

    # ---- changes -------------------------------------------------------------------------------
    def load(self, name: str, state_dict: Mapping[str, torch.Tensor], scale: float = 1.0, strict: bool = True) -> List[str]:
        """Merge the adapter `state_dict` under `name` at `scale`.  Everything is checked before anything is written.
        Returns the keys that were not applied (text-encoder keys always; with strict=False also keys that name no Linear
        of this module, which strict=True refuses)."""
        if name in self._adapters:
            raise ValueError(f"a LoRA named {name!r} is already loaded (unload it first)")
        if len(self._adapters) >= MAX_ADAPTERS:
            raise ValueError(f"at most {MAX_ADAPTERS} adapters can be loaded at once")
        placed, unplaced = parse_lora_state_dict(state_dict, self.linears.keys())
        foreign = [k for k in unplaced if not is_text_encoder_key(k)]
        if strict and foreign:
            raise ValueError(f"LoRA {name!r}: {len(foreign)} keys name no nn.Linear of this model (convolution adapters are not "
                             f"supported; pass strict=False to load the rest): {foreign[:8]}{' ...' if len(foreign) > 8 else ''}")
        if not placed:
            raise ValueError(f"LoRA {name!r}: no key names an nn.Linear of this model")
        for mod, (down, up, _) in placed.items():
            check_shapes(mod, tuple(self.linears[mod].weight.shape), down, up)
        scale = float(scale)
        slot = min(set(range(MAX_ADAPTERS)) - {a.slot for a in self._adapters.values()})
        ad = _Adapter(slot, scale)
        with torch.no_grad():
            for mod, (down, up, alpha) in placed.items():
                w = self.linears[mod].weight
                r = down.shape[0]
                mult = 4 if w.dtype == torch.float32 else 32
                rp = -(-r // mult) * mult
                up_p = torch.zeros((w.shape[0], rp), dtype=w.dtype, device=w.device)
                down_t = torch.zeros((w.shape[1], rp), dtype=w.dtype, device=w.device)
                up_p[:, :r] = (up.to(device=w.device, dtype=torch.float32) * (alpha / r)).to(w.dtype)
                down_t[:, :r] = down.to(device=w.device, dtype=w.dtype).t()
                ad.factors[mod] = (up_p, down_t)
                if mod not in self._base:
                    self._base[mod] = w.detach().clone(memory_format=torch.contiguous_format)
        self._adapters[name] = ad
        self._plan = None
        self._merge()
        self.last_unplaced = unplaced
        return unplaced

    def set_scale(self, name: str, scale: float) -> None:
        self.set_scales({name: scale})

    def set_scales(self, scales: Mapping[str, float]) -> None:
        """New scales for some of the loaded adapters: a copy into the device scale table and one launch."""
        for n in scales:
            if n not in self._adapters:
                raise KeyError(f"no LoRA named {n!r} is loaded (loaded: {self.names()})")
        vals = {n: float(s) for n, s in scales.items()}
        for n, s in vals.items():
            self._adapters[n].scale = s
        self._merge()

    def set_global_scale(self, scale: float) -> bool:
        """One multiplier over every loaded adapter (what diffusers' `cross_attention_kwargs={"scale": s}` means).  Merges
        again only when it differs from the current one; returns whether it did."""
        scale = float(scale)
        if scale == self._global:
            return False
        self._global = scale
        if self._adapters:
            self._merge()
        return True

    def unload(self, name: str) -> None:
        """Remove one adapter.  Weights no other adapter touches get their base's bits back and their snapshot is freed."""
        if name not in self._adapters:
            raise KeyError(f"no LoRA named {name!r} is loaded (loaded: {self.names()})")
        del self._adapters[name]
        self._plan = None
        self._merge()
        still = {m for a in self._adapters.values() for m in a.factors}
        for mod in [m for m in self._base if m not in still]:
            del self._base[mod]
        self._plan = None

    def unload_all(self) -> None:
        if not self._adapters:
            return
        self._adapters.clear()
        self._plan = None
        self._merge()
        self._base.clear()
        self._plan = None

    # ---- the merge -----------------------------------------------------------------------------
    def _effective(self) -> List[float]:
        eff = [0.0] * MAX_ADAPTERS
        for a in self._adapters.values():
            eff[a.slot] = a.scale * self._global
        return eff

    def _entries(self):
        """Per snapshotted module: (weight, base, [(Up, DownT, slot), ...]) in load order (the kernel's summation order)."""
        out = []
        for mod, base in self._base.items():
            facs = [(*a.factors[mod], a.slot) for a in self._adapters.values() if mod in a.factors]
            out.append((self.linears[mod].weight, base, facs))
        return out

    def _merge(self) -> None:
        if not self._base:
            return
        eff = self._effective()
        entries = self._entries()
        w0 = entries[0][0]
        with torch.no_grad():
            if w0.device.type == "cuda":
                from . import ops
                if any(not w.is_contiguous() for w, _, _ in entries):
                    raise ops.BackendError("LoraSet: an adapted weight is not contiguous")
                if self._scales is None:
                    self._scales = torch.zeros(MAX_ADAPTERS, dtype=torch.float32, device=w0.device)
                if self._plan is None:
                    self._plan = ops.lora_plan([(w.detach(), b, f) for w, b, f in entries])
                self._scales.copy_(torch.tensor(eff, dtype=torch.float32))
                ops.lora_merge(self._plan, self._scales)
            else:
                for w, base, facs in entries:
                    _merge_torch(w, base, facs, eff)
        for w, _, _ in entries:
            torch.autograd.graph.increment_version(w)
        if self.on_change is not None:
            self.on_change()


def _merge_torch(w: torch.Tensor, base: torch.Tensor, facs, eff) -> None:
    """The kernel's formula in torch (CPU): fp32 products and sums, one rounding to the storage dtype, base bits when every
    scale is zero."""
    live = [(up, down_t, eff[slot]) for up, down_t, slot in facs if eff[slot] != 0.0]
    if not live:
        w.detach().copy_(base)
        return
    delta = torch.zeros(w.shape, dtype=torch.float32)
    for up, down_t, s in live:
        delta.add_(up.float() @ down_t.float().t(), alpha=s)
    w.detach().copy_((base.float() + delta).to(w.dtype))


def attach(compiled: nn.Module) -> LoraSet:
    """The LoraSet of a module (an `optimize_model` result, or a plain `nn.Module`), created on first use.  One set per
    module: every owner that drives this module shares it."""
    holder = compiled.__dict__
    ls = holder.get("_lora_set")
    if ls is None:
        if not isinstance(compiled, nn.Module):
            raise TypeError("lora.attach: expected an nn.Module (the result of optimize_model, or the model itself)")
        ls = holder["_lora_set"] = LoraSet(compiled)
    return ls
