"""IP-Adapter image prompts inside the compiled UNet (Ye et al. 2023; diffusers' `load_ip_adapter` / IPAdapterAttnProcessor2_0,
ComfyUI's IPAdapter nodes): a decoupled cross-attention over a few image tokens, with its own `to_k_ip` / `to_v_ip` weights, added
to every cross-attention (`attn2`) site of a UNet compiled with `ip_adapter=N`:

    out = Attn(q, K_text, V_text) + sum_a  s[site, a] * m_a[t] * Attn(q, K_img_a, V_img_a)            (a over the adapter slots)

one launch per site (ops.attention_segments, csrc/attention_segments.hip): segment 0 is the text context - the k | v halves of the
hoisted context cache - and segment 1 + a the image K / V of slot a, N_a keys in a buffer of this state; each segment has its own
softmax, the sum is formed in fp32 from the un-rounded results and rounded once.

Everything a site reads lives in device buffers of the state module `gm.ip_adapter`, read by address, so every call below is an
in-place write and a captured graph stays:
  * `scales` (n_sites, 1 + A) fp32: column 0, the text column, is always 1; slot columns start at 0 = "off".  A site reads its own
    row as the kernel's `seg_scale`: a slot at 0 is SKIPPED by the whole grid (its K / V are never read), which leaves the bits of
    the module compiled without the pass;
  * per (rows, T) a weight buffer (rows, 1 + A, T) fp32, initialised to 1: the per-cell mask of every slot (`set_masks`);
  * per site and slot the stacked [to_k_ip; to_v_ip] weight (2 C_site, cross_dim), zero until `load`;
  * per (rows, site, slot) the image K / V (rows, N_a, 2 C_site) in the model dtype, zero until `set_image`.
`bind(rows, latent_hw, device)` allocates them outside any capture; nothing is ever reallocated.

Numbered checkpoint keys (`ip_adapter.{1,3,5,...}.to_k_ip.weight`): number 2i + 1 is the i-th cross-attention in diffusers'
`attn_processors` order - all of `down_blocks`, then all of `up_blocks`, then `mid_block`, each in module order - which is NOT this
project's down / mid / up module order.  Diffusers is not a dependency, so that order is restated here from the published loaders:
parity with real checkpoints is unpinned.

`attention_ip_wrapper` is the fx leaf optimizers/insert_ip_adapter.py puts in place of `attention_wrapper` at the attn2 sites: HIP
for device tensors, `reference` - a plain torch statement of the formula - for CPU tensors, so that a traced CPU module can carry the
pass on its own.
"""
from __future__ import annotations

import re
from typing import Dict, Mapping, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn

from .regions import site_levels
from .state import RowBound, require_state

MAX_SLOTS = 4              # adapters per compiled module (1 text + 4 image segments of st_attention_segments' 8)
MAX_TOKENS = 255           # keys per segment (the text-context kernel's range)

_NUMBERED = re.compile(r"^(\d+)\.to_([kv])_ip\.weight$")
_PATHED = re.compile(r"^(.*?)(?:\.processor)?\.to_([kv])_ip(?:\.(\d+))?\.weight$")


def parse_token_counts(ip_adapter) -> Tuple[int, ...]:
    """`ip_adapter=N` or a tuple of up to MAX_SLOTS token counts -> the tuple."""
    counts = (ip_adapter,) if isinstance(ip_adapter, int) and not isinstance(ip_adapter, bool) else ip_adapter
    try:
        counts = tuple(counts)
    except TypeError:
        counts = ()
    if not 1 <= len(counts) <= MAX_SLOTS or not all(isinstance(n, int) and not isinstance(n, bool) and 1 <= n <= MAX_TOKENS for n in counts):
        raise ValueError(f"ip_adapter: an image token count in [1, {MAX_TOKENS}] (4: base, 16: plus) or a tuple of up to {MAX_SLOTS} of them "
                         f"expected, got {ip_adapter!r}")
    return counts


def diffusers_order(sites: Sequence[str]):
    """Site indices in diffusers' `attn_processors` order: down_blocks, then up_blocks, then mid_block, each in module order."""
    def stage(path: str) -> int:
        p = "." + path
        return 0 if ".down_blocks." in p else (1 if ".up_blocks." in p else 2)
    return sorted(range(len(sites)), key=lambda i: (stage(sites[i]), i))


def mask_level_weights(masks: torch.Tensor, level: int) -> torch.Tensor:
    """(lh, lw) or (batch, lh, lw) masks -> the (batch, T_l) float32 weights of attention level `level`: the area mean over every
    2^level x 2^level cell, NOT normalised, flattened row-major (pure, on the host)."""
    m = torch.as_tensor(masks).detach().to("cpu", torch.float32)
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if m.dim() != 3:
        raise ValueError(f"ip_adapter masks must be (lh, lw) or (batch, lh, lw), got {tuple(torch.as_tensor(masks).shape)}")
    if not bool(torch.isfinite(m).all()) or bool((m < 0).any()):
        raise ValueError("ip_adapter masks must be finite and non-negative")
    cell = 1 << level
    lh, lw = m.shape[-2:]
    if lh % cell or lw % cell:
        raise ValueError(f"ip_adapter masks: a {lh} x {lw} mask does not divide into {cell} x {cell} cells (level {level})")
    if level:
        m = F.avg_pool2d(m.unsqueeze(1), cell).squeeze(1)
    return m.flatten(1).contiguous()


def project_image_embeds(image_proj_state_dict: Mapping[str, torch.Tensor], image_embeds: torch.Tensor) -> torch.Tensor:
    """The linear ImageProjection of the base adapters (`proj.weight|bias`, `norm.weight|bias`): (B, emb) -> (B, N, cross_dim)
    = LayerNorm(reshape(proj(e))), in fp32 torch, once per image.  Resampler projections (Plus, FaceID) are not built: pass their
    output tokens to `set_image` directly."""
    sd = image_proj_state_dict
    missing = [k for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias") if k not in sd]
    if missing:
        raise ValueError(f"project_image_embeds: the linear ImageProjection has proj.weight|bias and norm.weight|bias; missing {missing} "
                         "(a Resampler projection is not built here: pass its output tokens to set_image)")
    e = torch.as_tensor(image_embeds).float()
    if e.dim() == 1:
        e = e.unsqueeze(0)
    w, b = sd["proj.weight"].float().to(e.device), sd["proj.bias"].float().to(e.device)
    g, beta = sd["norm.weight"].float().to(e.device), sd["norm.bias"].float().to(e.device)
    cross = g.shape[0]
    if e.dim() != 2 or w.shape[1] != e.shape[1] or w.shape[0] % cross:
        raise ValueError(f"project_image_embeds: image_embeds {tuple(e.shape)} against proj.weight {tuple(w.shape)}, norm {cross}")
    y = F.linear(e, w, b).reshape(e.shape[0], w.shape[0] // cross, cross)
    return F.layer_norm(y, (cross,), g, beta, 1e-5)


class IPAdapter(RowBound, nn.Module):
    """State of one compiled module: the slots' token counts, the attn2 site paths with their widths, and the device buffers."""
    label = "ip_adapter"

    def __init__(self, tokens: Sequence[int], sites: Sequence[str], dims: Sequence[Tuple[int, int]], levels=None, like=None):
        super().__init__()
        self.tokens = parse_token_counts(tuple(tokens))
        self.sites = tuple(sites)
        self.dims = tuple((int(c), int(x)) for c, x in dims)       # per site (C_site, cross_dim)
        self.levels = None if levels is None else tuple(sorted(set(int(l) for l in levels)))
        # a parameter of the compiled module, held in a tuple (NOT registered here): its device and dtype are the model's
        self._like = (like,)
        # Plain attributes under names torch does not know, NOT registered buffers, for the reasons regions.Regions._weights gives:
        # state_dict() / buffers() do not see them and .to(dtype) / .half() leave them at their addresses and types
        self._scales: Optional[torch.Tensor] = None                               # (n_sites, 1 + A) fp32
        self._ip_weights: Dict[Tuple[int, int], torch.Tensor] = {}                # (site, slot) -> (2 C_site, cross_dim)
        self._weights: Dict[Tuple[int, int], torch.Tensor] = {}                   # (rows, T) -> (rows, 1 + A, T) fp32
        self._kv: Dict[Tuple[int, int, int], torch.Tensor] = {}                   # (rows, site, slot) -> (rows, N_a, 2 C_site)
        self._loaded = [False] * len(self.tokens)

    # ---- buffers ---------------------------------------------------------------------------------
    @property
    def slots(self) -> int:
        return len(self.tokens)

    def _model(self):
        p = self._like[0]
        if p is None:
            raise ValueError("ip_adapter: the state is not attached to a module's parameters")
        return p.device, p.dtype

    def _static(self) -> None:
        """The scale table and the adapter weights: on the model's device, allocated once."""
        if self._scales is not None:
            return
        dev, dtype = self._model()
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ip_adapter: allocate the buffers (bind) before the capture starts")
        sc = torch.zeros((len(self.sites), 1 + self.slots), dtype=torch.float32)
        sc[:, 0] = 1.0
        self._scales = sc.to(dev)
        for i, (c, x) in enumerate(self.dims):
            for a in range(self.slots):
                self._ip_weights[(i, a)] = torch.zeros((2 * c, x), dtype=dtype, device=dev)

    @property
    def scales(self) -> torch.Tensor:
        self._static()
        return self._scales

    def bind(self, rows: int, latent_hw, device) -> None:
        """Allocate every buffer of a UNet batch of `rows` rows at this latent size: mask weights 1, image K / V zero, and (once) the
        scale table and the adapter weights.  Outside any capture; what exists is kept, so binding twice is free."""
        rows, lh, lw, device = self._parse_bind(rows, latent_hw, device)
        dev, dtype = self._model()
        if torch.device(dev).type != device.type:
            raise ValueError(f"ip_adapter.bind: the module lives on {dev}, not {device}")
        self._static()
        for l in self._levels_for(lh, lw):
            T = (lh >> l) * (lw >> l)
            if (rows, T) not in self._weights:
                self._refuse_capture(dev)
                self._weights[(rows, T)] = torch.ones((rows, 1 + self.slots, T), dtype=torch.float32, device=dev)
        for i, (c, _) in enumerate(self.dims):
            for a, n in enumerate(self.tokens):
                if (rows, i, a) not in self._kv:
                    self._refuse_capture(dev)
                    self._kv[(rows, i, a)] = torch.zeros((rows, n, 2 * c), dtype=dtype, device=dev)

    def bound_rows(self):
        return sorted({r for r, _, _ in self._kv})

    def _slot(self, slot, what: str) -> int:
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.slots:
            raise ValueError(f"{what}: slot {slot!r} outside the {self.slots} adapter slot(s) this UNet was compiled with "
                             f"(ip_adapter={self.tokens})")
        return slot

    def weights_for(self, rows: int, T: int) -> torch.Tensor:
        buf = self._weights.get((int(rows), int(T)))
        if buf is None:
            raise ValueError(f"ip_adapter: no buffers for a cross-attention of {rows} rows x {T} queries (bound: {sorted(self._weights)}); "
                             "call gm.ip_adapter.bind(rows, latent_hw, device) before the first evaluation")
        return buf

    def kv_for(self, rows: int, site: int, slot: int) -> torch.Tensor:
        buf = self._kv.get((int(rows), site, slot))
        if buf is None:
            raise ValueError(f"ip_adapter: no image K/V buffers for {rows} rows (bound: {self.bound_rows()}); call "
                             "gm.ip_adapter.bind(rows, latent_hw, device) before the first evaluation")
        return buf

    # ---- checkpoints -----------------------------------------------------------------------------
    def _parse(self, state_dict: Mapping, slot: int):
        """-> ({(site, 'k' | 'v'): tensor}, image_proj dict or None), nothing written."""
        sd = dict(state_dict)
        image_proj = None
        if isinstance(sd.get("ip_adapter"), Mapping):                 # the published layout
            image_proj = dict(sd["image_proj"]) if isinstance(sd.get("image_proj"), Mapping) else None
            flat = dict(sd["ip_adapter"])
        else:
            flat = {k[len("ip_adapter."):]: v for k, v in sd.items() if isinstance(k, str) and k.startswith("ip_adapter.")}
            proj = {k[len("image_proj."):]: v for k, v in sd.items() if isinstance(k, str) and k.startswith("image_proj.")}
            image_proj = proj or None
            if not flat:
                flat = {k: v for k, v in sd.items() if isinstance(k, str) and not k.startswith("image_proj.")}
        n = len(self.sites)
        found: Dict[Tuple[int, str], torch.Tensor] = {}
        numbered = {}
        for key, val in flat.items():
            m = _NUMBERED.match(key)
            if m:
                numbered[(int(m.group(1)), m.group(2))] = val
        if numbered:
            numbers = sorted({k for k, _ in numbered})
            if numbers != [2 * i + 1 for i in range(n)] or len(numbered) != 2 * n:
                raise ValueError(f"ip_adapter.load: the checkpoint has to_k_ip / to_v_ip weights for {len(numbers)} cross-attentions "
                                 f"(numbers {numbers[:3]}...), this UNet has {n} sites (numbers 1, 3, ..., {2 * n - 1})")
            order = diffusers_order(self.sites)
            for (num, which), val in numbered.items():
                found[(order[(num - 1) // 2], which)] = val
        else:
            index = {p: i for i, p in enumerate(self.sites)}
            for key, val in flat.items():
                m = _PATHED.match(key)
                if not m:
                    continue
                path, which, j = m.group(1), m.group(2), m.group(3)
                if j is not None and int(j) != slot:                  # another adapter's weights in a multi-adapter state dict
                    continue
                if path not in index:
                    raise ValueError(f"ip_adapter.load: {key!r} names no cross-attention site of this UNet (sites: {list(self.sites[:2])} ...)")
                found[(index[path], which)] = val
            if len(found) != 2 * n:
                raise ValueError(f"ip_adapter.load: the checkpoint has {len(found)} to_k_ip / to_v_ip weights for slot {slot}, this UNet "
                                 f"has {n} sites and needs {2 * n}")
        for (i, which), val in found.items():
            if not torch.is_tensor(val) or tuple(val.shape) != self.dims[i]:
                got = tuple(val.shape) if torch.is_tensor(val) else type(val).__name__
                raise ValueError(f"ip_adapter.load: to_{which}_ip of site {self.sites[i]} must be (C_site, cross_dim) = {self.dims[i]}, got {got}")
        return found, image_proj

    def load(self, state_dict: Mapping, slot: int = 0):
        """Copy an adapter's to_k_ip / to_v_ip weights into the slot's stacked buffers, in place.  Three key forms: the published
        layout {"image_proj": {...}, "ip_adapter": {"1.to_k_ip.weight", "1.to_v_ip.weight", "3...."}}; the same flattened with dots;
        path-spelled `<site path>.processor.to_{k,v}_ip.<slot>.weight` or `<site path>.to_{k,v}_ip.weight`.  Numbered keys follow
        diffusers' attn_processors order (module docstring: restated, parity with real checkpoints unpinned).  Every shape and the
        site count are validated before anything is written.  Returns the checkpoint's image_proj sub-dict (or None).  The image
        K / V of an image set earlier were projected with the old weights: call `set_image` again."""
        slot = self._slot(slot, "ip_adapter.load")
        found, image_proj = self._parse(state_dict, slot)
        self._static()
        with torch.no_grad():
            for i, (c, _) in enumerate(self.dims):
                w = self._ip_weights[(i, slot)]
                w[:c].copy_(found[(i, "k")])
                w[c:].copy_(found[(i, "v")])
        self._loaded[slot] = True
        return image_proj

    def unload(self, slot: int = 0) -> None:
        """The slot back to "off": scale column 0, adapter weights and image K / V zero, masks 1."""
        slot = self._slot(slot, "ip_adapter.unload")
        self._static()
        self._scales[:, 1 + slot].zero_()
        for (i, a), w in self._ip_weights.items():
            if a == slot:
                w.zero_()
        for (r, i, a), buf in self._kv.items():
            if a == slot:
                buf.zero_()
        for buf in self._weights.values():
            buf[:, 1 + slot].fill_(1.0)
        self._loaded[slot] = False

    # ---- the live knobs --------------------------------------------------------------------------
    def resolve_scale(self, scale) -> torch.Tensor:
        """A float, or a mapping {regular expression: float} `re.search`ed against the site paths ("mid" selects every site under
        `mid_block`, as for `pag_layers`): the first expression that matches a site gives its scale, a site none matches gets 0.
        -> (n_sites,) float32 on the host."""
        if isinstance(scale, Mapping):
            rules = [(re.compile(k), float(v)) for k, v in scale.items()]
            vals = [next((v for p, v in rules if p.search(path)), 0.0) for path in self.sites]
        else:
            if isinstance(scale, bool) or torch.is_tensor(scale) and scale.numel() != 1:
                raise ValueError(f"ip_adapter scale: a float or a mapping of regular expressions to floats expected, got {scale!r}")
            vals = [float(scale)] * len(self.sites)
        out = torch.tensor(vals, dtype=torch.float32)
        if not bool(torch.isfinite(out).all()):
            raise ValueError(f"ip_adapter scale: finite values expected, got {scale!r}")
        return out

    def set_scale(self, scale, slot: int = 0) -> None:
        slot = self._slot(slot, "ip_adapter.set_scale")
        col = self.resolve_scale(scale)
        self._static()
        self._scales[:, 1 + slot].copy_(col)

    def set_masks(self, masks, slot: int = 0, rows: Optional[int] = None) -> None:
        """Per-cell weight of the slot's image prompt: (lh, lw) or (batch, lh, lw) at latent resolution, non-negative and finite; the
        level weights are the area mean per 2^l x 2^l cell (`mask_level_weights`), not normalised, written to EVERY row (row r takes
        mask r % batch).  None: 1 everywhere."""
        slot = self._slot(slot, "ip_adapter.set_masks")
        rows = self._rows(rows, "ip_adapter.set_masks")
        mine = [(T, buf) for (r, T), buf in self._weights.items() if r == rows]
        if masks is None:
            for _, buf in mine:
                buf[:, 1 + slot].fill_(1.0)
            return
        m = torch.as_tensor(masks)
        lh, lw = int(m.shape[-2]), int(m.shape[-1])
        new = []
        for l in self._levels_for(lh, lw):
            w = mask_level_weights(m, l)
            T = w.shape[1]
            if (rows, T) not in self._weights:
                raise ValueError(f"ip_adapter.set_masks: masks of {lh} x {lw} do not match the latent size bound for {rows} rows "
                                 f"(buffers: {sorted(t for t, _ in mine)} queries)")
            if rows % w.shape[0]:
                raise ValueError(f"ip_adapter.set_masks: {rows} rows do not divide into a per-batch mask of {w.shape[0]} entries")
            new.append((self._weights[(rows, T)], w.repeat(rows // w.shape[0], 1)))
        for buf, w in new:          # (nothing is written unless every level validated)
            buf[:, 1 + slot].copy_(w)

    def set_image(self, tokens: torch.Tensor, negative_tokens: Optional[torch.Tensor] = None, slot: int = 0, rows: Optional[int] = None,
                  chunks: int = 1, negative: Optional[bool] = None) -> None:
        """Project the image tokens (B or 1, N_a, cross_dim) of the slot through every site's stacked [to_k_ip; to_v_ip] weight
        (ops.linear; F.linear for a CPU module) into the bound K / V buffers of `rows` = chunks * B rows, in place.  `chunks` says
        how the UNet batch divides into equal blocks, as for regions, and `negative` whether the first block is the negative one
        (default: yes when chunks > 1): it takes `negative_tokens` (default: zero tokens, which give zero K / V and therefore no
        contribution), every other block - PAG's perturbed block too - takes `tokens`."""
        slot = self._slot(slot, "ip_adapter.set_image")
        rows = self._rows(rows, "ip_adapter.set_image")
        if isinstance(chunks, bool) or not isinstance(chunks, int) or chunks < 1 or rows % chunks:
            raise ValueError(f"ip_adapter.set_image: {rows} rows do not divide into chunks={chunks!r} equal blocks")
        B, N = rows // chunks, self.tokens[slot]
        negative = chunks > 1 if negative is None else bool(negative)
        dev, dtype = self._model()
        cross = {x for _, x in self.dims}

        def block(t, what):
            t = torch.as_tensor(t)
            if t.dim() != 3 or t.shape[0] not in (1, B) or t.shape[1] != N or t.shape[2] not in cross:
                raise ValueError(f"ip_adapter.set_image: {what} must be (B or 1, N, cross_dim) = ({B} or 1, {N}, {sorted(cross)[0]}) for slot "
                                 f"{slot} (compiled with ip_adapter={self.tokens}), got {tuple(t.shape)}")
            return t.to(dev, dtype).expand(B, -1, -1)

        pos = block(tokens, "tokens")
        neg = torch.zeros_like(pos) if negative_tokens is None else block(negative_tokens, "negative_tokens")
        if not negative and negative_tokens is not None:
            raise ValueError("ip_adapter.set_image: negative_tokens need a negative row block (guidance; chunks 2 or 3)")
        x = torch.cat(([neg] if negative else [pos]) + [pos] * (chunks - 1))
        x = x.contiguous()
        with torch.no_grad():
            for i in range(len(self.sites)):
                w = self._ip_weights[(i, slot)]
                if dev.type == "cpu":
                    kv = F.linear(x, w)
                else:
                    from . import ops
                    kv = ops.linear(x, w)
                self._kv[(rows, i, slot)].copy_(kv)

    def extra_repr(self) -> str:
        return f"tokens={self.tokens}, sites={len(self.sites)}, levels={self.levels}, loaded={self._loaded}, bound={self.bound_rows()}"


def reference(q: torch.Tensor, segments, weights: torch.Tensor, seg_scale: torch.Tensor, num_heads: int, sm_scale: float) -> torch.Tensor:
    """Plain torch: the formula of the module docstring on (B, T, H*D) / (B, len_r, H*D) projections; weights (B, S, T), seg_scale (S)."""
    from .pag import identity_attention_reference
    wide = torch.promote_types(q.dtype, torch.float32)
    acc = None
    for r, (k, v) in enumerate(segments):
        a = identity_attention_reference(q, k, v, num_heads, sm_scale, 0).to(wide)
        w = (seg_scale[r].float() * weights[:, r].float()).to(wide)
        term = w.unsqueeze(-1) * a
        acc = term if acc is None else acc + term
    return acc.to(q.dtype)


def attention_ip_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                         state: IPAdapter, site: int) -> torch.Tensor:
    """fx leaf: attention_wrapper over the text segment (k, v) and the image segments of the state's slots at this site."""
    rows, T, C = q.shape
    w = state.weights_for(rows, T)
    sc = state.scales[site]
    segs = [(k, v)]
    for a in range(state.slots):
        kv = state.kv_for(rows, site, a)
        segs.append((kv[..., :C], kv[..., C:]))
    if q.device.type == "cpu":
        return reference(q, segs, w, sc, num_heads, sm_scale)
    from . import ops
    if C != num_heads * head_dim:
        raise ops.BackendError(f"attention_ip_wrapper: C={C} != num_heads*head_dim={num_heads * head_dim}")
    return ops.attention_segments(q, segs, w, sc, num_heads, sm_scale)


torch.fx.wrap("attention_ip_wrapper")


def state_of(module, what: str) -> IPAdapter:
    """The IP-Adapter state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "ip_adapter", IPAdapter, what, "IP-Adapter cross-attention sites", "ip_adapter=N")


def check_combination(ip_adapter, regions, fp8) -> None:
    if ip_adapter is None:
        return
    if regions is not None:
        raise ValueError("ip_adapter=N cannot be combined with regions=R: one pass per cross-attention site (a follow-up)")
    if fp8:
        raise ValueError("ip_adapter=N cannot be combined with fp8=True: the fp8 plan does not cover IP-Adapter cross-attention sites")
