"""What the per-feature state modules (freeu, pag, seg, regions, ip_adapter, t2i_adapter) share: the lookup of a compiled module's
state, and the base of the states whose device buffers are bound per UNet row count and latent size."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

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
