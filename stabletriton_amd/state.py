"""What the per-feature state modules (freeu, pag, seg, regions, ip_adapter, t2i_adapter, controlnet) share: the lookup of a
compiled module's state, the base of the states whose device buffers are bound per UNet row count and latent size, and on top of
it the state of the residual sites (t2i_adapter, controlnet)."""
from __future__ import annotations

import contextlib
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import nn

_FALLBACK_LEVELS = 4       # levels tried when the site paths do not spell their stage (regions.Regions.levels)


def compiled_state(module, attr: str, cls):
    """`module.<attr>` when the module was compiled with that feature's sites, else None."""
    st = getattr(module, attr, None)
    return st if isinstance(st, cls) else None


def require_state(module, attr: str, cls, what: str, sites_phrase: str, flag_hint: str):
    """`compiled_state`, or a ValueError that names the missing compile argument."""
    st = compiled_state(module, attr, cls)
    if st is None:
        raise ValueError(f"{what}: this UNet was compiled without {sites_phrase}; compile it with {flag_hint} "
                         "(optimize_model / compile_unet_from_state_dict / attach_to_diffusers / compile_comfy_unet / patch_comfy_model)")
    return st


def latent_size(latent_hw) -> Tuple[int, int]:
    """One side of a square latent, or (height, width)."""
    if isinstance(latent_hw, (tuple, list, torch.Size)):
        return int(latent_hw[0]), int(latent_hw[1])
    return int(latent_hw), int(latent_hw)


class RowBound:
    """Mixin of the states that `bind(rows, latent_hw, device)` buffers; the class says `label` and `bound_rows()`."""
    label = ""

    def _rows(self, rows: Optional[int], what: str) -> int:
        have = self.bound_rows()
        if rows is None:
            if len(have) != 1:
                raise ValueError(f"{what}: pass rows=: this state is bound for the row counts {have} (bind(rows, latent_hw, device) first)")
            return have[0]
        if int(rows) not in have:
            raise ValueError(f"{what}: no buffers for {rows} rows (bound: {have}); call bind(rows, latent_hw, device) first")
        return int(rows)

    def _levels_for(self, lh: int, lw: int):
        cand = self.levels if self.levels is not None else range(_FALLBACK_LEVELS)
        out = [l for l in cand if lh % (1 << l) == 0 and lw % (1 << l) == 0 and (lh >> l) and (lw >> l)]
        if self.levels is not None and len(out) != len(self.levels):
            raise ValueError(f"{self.label}: a {lh} x {lw} latent does not divide into the attention levels {self.levels} of this UNet")
        return out

    def _parse_bind(self, rows: int, latent_hw, device):
        lh, lw = latent_size(latent_hw)
        rows = int(rows)
        if rows < 1 or lh < 1 or lw < 1:
            raise ValueError(f"{self.label}.bind: rows {rows}, latent {lh} x {lw}")
        return rows, lh, lw, torch.device(device)

    def _refuse_capture(self, device: torch.device, what: str = "the buffers") -> None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self.label}.bind: allocate {what} before the capture starts")


def comfy_control(control, accepted: str, of: str):
    """ComfyUI's `control` dict, checked, as (its input list, its output list, the middle block's entry or None); `accepted` / `of`
    name the lists the caller takes and whose they are.  Copies: the caller's lists are not consumed."""
    if not isinstance(control, dict):
        raise NotImplementedError(f"control must be a dict of lists ({accepted}), got {type(control).__name__}")
    extra = sorted(k for k in control if k not in ("input", "middle", "output"))
    if extra:
        raise NotImplementedError(f"control entries {extra} are not supported by the compiled UNet ({accepted} of {of} are)")
    middle = list(control.get("middle") or [])
    if any(e is not None for e in middle[:-1]):
        raise NotImplementedError('control["middle"] carries more than one residual; the middle block takes the last entry')
    return list(control.get("input") or []), list(control.get("output") or []), middle[-1] if middle else None


def finite_scale(label: str, scale) -> float:
    scale = float(scale)
    if not (scale == scale and abs(scale) != float("inf")):
        raise ValueError(f"{label}: scale must be finite, got {scale!r}")
    return scale


class _SiteTables(NamedTuple):
    """What a `ResidualSites` state owns on one device, in the order `_own()` is indexed by."""
    scale: torch.Tensor                    # fp32, one entry: the state's own scale
    step: torch.Tensor                     # int32, one entry, always 0: the index the sites read `scale` at
    weights: Optional[torch.Tensor]        # fp32, one factor per site, or None for a state without site weights


class ResidualSites(RowBound, nn.Module):
    """Base of the two states whose sites add `s * r_k` to an activation in place (csrc/t2i_adapter.hip), s = table[*step] read
    on the device: t2i_adapter.T2IAdapterState and controlnet.ControlNetState.  `sites` are (name, channels, latent halvings, ...)
    tuples.  Static buffers per bound row count and site size, a one-entry scale table and a step counter, all read by ADDRESS, so
    `set` / `set_scale` / `clear` are in-place writes a captured graph picks up; a caller with per-step scales hands its own table and
    step counter to the sites with `using(step, table)` around its UNet calls.  The class says `label` and `words`."""
    words = ("residual", "residuals", "rows")      # one site's tensor in messages, its plural, the rows it may have

    def __init__(self, sites: Sequence[tuple], dtype: Optional[torch.dtype] = None):
        super().__init__()
        self.sites = tuple(s[0] for s in sites)
        self.channels = tuple(int(s[1]) for s in sites)
        self.levels = tuple(int(s[2]) for s in sites)
        self.dtype = dtype                                 # the dtype `bind` allocates in when it is not told another
        # (rows, site, h, w) -> (buffer rows, C, h, w) channels_last, never reallocated.  Plain dicts under names torch does not
        # know, as in regions.Regions: not registered buffers, so .to(dtype) / state_dict() leave them alone at their addresses
        self._buffers: Dict[Tuple[int, int, int, int], torch.Tensor] = {}
        self._tables: Dict[torch.device, _SiteTables] = {}
        self._use = None                                   # (step, table) of the caller inside `using`
        self.host_scale = 0.0                              # the state's own scale as a Python float (the CPU route computes with it)
        self.host_weights = None                           # likewise one factor per site, for a state that has them

    # ---- geometry --------------------------------------------------------------------------------
    def site_shapes(self, latent_hw):
        """(C, h, w) of every site at this latent size: each halving is the UNet's stride-2 convolution, ceil(n / 2) (the T2I
        adapter's AvgPool2d(ceil_mode=True) and PixelUnshuffle of a multiple of 16 pixels give the same sizes)."""
        lh, lw = latent_size(latent_hw)
        out = []
        for c, l in zip(self.channels, self.levels):
            h, w = lh, lw
            for _ in range(l):
                h, w = (h + 1) // 2, (w + 1) // 2
            out.append((c, h, w))
        return out

    # ---- buffers ---------------------------------------------------------------------------------
    def bind(self, rows: int, latent_hw, device, dtype: Optional[torch.dtype] = None, buffer_rows: Optional[int] = None) -> None:
        """Allocate, outside any capture, the zeroed buffers of a UNet batch of `rows` rows at this latent size, the one-entry scale
        table (0 = off), the step counter and the site weights where the state has them.  `buffer_rows` (a divisor of rows; default
        rows): how many rows the buffers hold - the row blocks [negative | positive | perturbed] of a guided call can share one copy
        of `batch` rows.  A buffer that exists is kept (its address is what captured graphs read), so binding twice is free."""
        rows, (lh, lw), device = int(rows), latent_size(latent_hw), torch.device(device)
        b_rows = rows if buffer_rows is None else int(buffer_rows)
        if rows < 1 or lh < 1 or lw < 1 or b_rows < 1 or rows % b_rows:      # (not _parse_bind: this text names the buffers' rows too)
            raise ValueError(f"{self.label}.bind: rows {rows}, latent {lh} x {lw}, {self.words[0]}_rows {b_rows} (a divisor of rows)")
        dtype = dtype or self.dtype or torch.float32
        if device not in self._tables:
            self._refuse_capture(device)
            self._tables[device] = _SiteTables(
                torch.full((1,), self.host_scale, dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.int32, device=device),
                None if self.host_weights is None else torch.tensor(self.host_weights, dtype=torch.float32, device=device))
        for k, (c, h, w) in enumerate(self.site_shapes((lh, lw))):
            buf = self._buffers.get((rows, k, h, w))
            if buf is None:
                self._refuse_capture(device)
                self._buffers[(rows, k, h, w)] = torch.zeros((b_rows, c, h, w), dtype=dtype, device=device).contiguous(
                    memory_format=torch.channels_last)
            elif buf.device != device or buf.dtype != dtype or buf.shape[0] != b_rows:
                raise ValueError(f"{self.label}.bind: the buffers of {rows} rows at site {self.sites[k]} are {tuple(buf.shape)} {buf.dtype} "
                                 f"on {buf.device}; asked for {b_rows} {self.words[0]} rows of {dtype} on {device}")

    def bound_rows(self):
        return sorted({key[0] for key in self._buffers})

    def buffer_for(self, rows: int, k: int, h: int, w: int) -> torch.Tensor:
        """The buffer site k of a call with `rows` rows reads at the site size h x w."""
        buf = self._buffers.get((int(rows), int(k), int(h), int(w)))
        if buf is None:
            raise ValueError(f"{self.label}: no {self.words[0]} buffer for site {self.sites[k]} at {rows} rows x {h} x {w} (bound: "
                             f"{sorted(self._buffers)}); call gm.{self.label}.bind(rows, latent_hw, device) before the first evaluation")
        return buf

    def _own(self, device=None) -> _SiteTables:
        """The record (scale table, step, site weights or None) of `device`, or of the one bound device."""
        if not self._tables:
            raise ValueError(f"{self.label}: nothing is bound; call bind(rows, latent_hw, device) first")
        if device is None:
            if len(self._tables) != 1:
                raise ValueError(f"{self.label}: bound on {sorted(str(d) for d in self._tables)}: one state serves one device")
            return next(iter(self._tables.values()))
        if torch.device(device) not in self._tables:
            raise ValueError(f"{self.label}: nothing is bound on {device}; call bind(rows, latent_hw, device) first")
        return self._tables[torch.device(device)]

    # ---- values ----------------------------------------------------------------------------------
    def _check_list(self, values, what: str) -> None:
        one, many, b_rows = self.words
        n = len(self.sites)
        if not isinstance(values, (list, tuple)) or len(values) != n:
            got = len(values) if isinstance(values, (list, tuple)) else type(values).__name__
            raise ValueError(f"{what}: takes {n} {many}, one per site {self.sites}, got {got}")
        for k, v in enumerate(values):
            if not torch.is_tensor(v) or v.dim() != 4 or v.shape[1] != self.channels[k]:
                shape = tuple(v.shape) if torch.is_tensor(v) else type(v).__name__
                raise ValueError(f"{what}: {one} {k} (site {self.sites[k]}) must be ({b_rows}, {self.channels[k]}, h, w), got {shape}")

    def check(self, values, rows: int, what: str):
        """The (buffer, tensor) pairs `set` would write into the buffers bound for `rows`, validated; nothing is written."""
        self._check_list(values, what)
        one, pairs = self.words[0], []
        for k, v in enumerate(values):
            buf = self._buffers.get((rows, k, int(v.shape[2]), int(v.shape[3])))
            if buf is None:
                sizes = sorted(key[2:] for key in self._buffers if key[0] == rows and key[1] == k)
                raise ValueError(f"{what}: {one} {k} (site {self.sites[k]}) is {tuple(v.shape[2:])}; the buffers bound for {rows} rows "
                                 f"have the sizes {sizes} there (a control image is 8 x the latent size)")
            if v.shape[0] not in (1, buf.shape[0]):
                raise ValueError(f"{what}: {one} {k} (site {self.sites[k]}) has {v.shape[0]} rows; the buffers hold {buf.shape[0]} "
                                 "(or 1 for every row)")
            pairs.append((buf, v))
        return pairs

    def set(self, values, scale: Optional[float] = 1.0, rows: Optional[int] = None) -> None:
        """Copy one tensor per site into the buffers of `rows` in place, and (scale not None) set the state's own scale."""
        rows = self._rows(rows, f"{self.label}.set")
        pairs = self.check(values, rows, f"{self.label}.set")
        for buf, v in pairs:          # (nothing is written unless every site validated)
            buf.copy_(v.detach().to(buf.dtype).expand(buf.shape))
        if scale is not None:
            self.set_scale(scale)

    def set_scale(self, scale: float) -> None:
        """The state's own scale (what the sites read outside `using`): an in-place write on every bound device."""
        scale = finite_scale(self.label, scale)
        for own in self._tables.values():
            own.scale.fill_(scale)
        self.host_scale = scale

    def clear(self) -> None:
        """Back to "off": scale 0 (the buffers and the weights keep their contents; at scale 0 nobody reads the buffers)."""
        for own in self._tables.values():
            own.scale.zero_()
        self.host_scale = 0.0

    @contextlib.contextmanager
    def using(self, step: torch.Tensor, table: torch.Tensor):
        """Around the caller's own UNet calls: the sites read `table[*step]` (an fp32 device table, an int32 device counter, both by
        address) instead of the state's own scale."""
        if step.dtype != torch.int32 or step.numel() != 1 or table.dtype != torch.float32 or table.dim() != 1:
            raise ValueError(f"{self.label}.using: step is an int32 tensor of one entry, table a 1-D fp32 tensor")
        prev, self._use = self._use, (step, table)
        try:
            yield self
        finally:
            self._use = prev

    def current(self, device):
        """(step, table, site weights or None) the sites of a call on `device` read."""
        own = self._own(device)
        step, table = (own.step, own.scale) if self._use is None else self._use
        return step, table, own.weights

    def cpu_scale(self, step: torch.Tensor, table: torch.Tensor) -> float:
        """What a CPU site computes with for the (step, table) of `current`: the state's own scale as a float, or inside `using`
        table[*step] under the kernel's clamp (a step past the table reads its last entry, one below it its first)."""
        if self._use is None:
            return self.host_scale
        return float(table[min(max(int(step.reshape(-1)[0]), 0), table.numel() - 1)])

    def extra_repr(self) -> str:
        return f"sites={self.sites}, channels={self.channels}, levels={self.levels}, bound={sorted(self._buffers)}"
