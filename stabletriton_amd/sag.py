"""Self-attention guidance (SAG; Hong et al., "Improving Sample Quality of Diffusion Models Using Self-Attention Guidance", 2023;
ComfyUI's core `Self-Attention Guidance` node, nodes_sag.py, restated for an eps-predicting loop) on the compiled UNet.

SAG needs classifier-free guidance and a SECOND, dependent UNet evaluation per step.  Per step, with x the fp32 latent and sigma the
step's noise level:
    1. the ordinary call on [negative | positive]; at ONE self-attention site (default: the first `attn1` of the middle block) the
       negative rows also leave A[b, j] = (1 / H) sum_h sum_i softmax(q k^T * scale)[i, j], the probability matrix's column sums
       averaged over the heads: how much attention key token j receives (ops.attention_colsum, csrc/attention_colsum.hip);
    2. x0 = x - sigma e_neg;  mask = A > threshold on the site's token grid, nearest-upsampled to the latent;  the masked cells of
       x0 are replaced by a nine-tap Gaussian blur (reflect padding), the noise sigma e_neg is put back and the result scaled as a
       UNet input (ops.sag_degrade, csrc/sag.hip, one launch);
    3. the UNet on those rows under the NEGATIVE conditioning: e_sag;
    4. e = cfg(e_neg, e_pos) + s (e_neg - e_sag)   (ops.sag_*_step: the guided updates with one more fma).
Defaults are ComfyUI's: scale 0.5, blur sigma 2, threshold 1.

The state module `gm.sag` holds the site's path, the HOST integer `rows` - the leading `rows` batch entries of a call record A, 0 =
none - and the call's latent size, both set for the duration of a caller's own UNet calls with `state.using(rows, latent_hw)`, and
per bound (rows, latent size): A, the mask `sag_degrade` used (`state.mask`: users visualise it), the column-sum workspace and the
DEVICE parameter row (threshold, blur sigma) the degrade launch reads by address - `set_params` writes it in place, so a captured
graph follows without a new capture.  `bind(rows, latent_hw, tokens, heads, device)` allocates outside any capture.

`attention_sag_wrapper` is the fx leaf optimizers/insert_sag.py puts in place of `attention_wrapper` at the site: ops.attention,
unchanged, then ops.attention_colsum when rows > 0.  With rows == 0 it is ops.attention: the launch and the bits of a module compiled
without the pass.  The hook wrappers only evaluate the UNet; a pipeline that orchestrates the second call itself uses `degrade`.
"""
from __future__ import annotations

import contextlib
import math
import numbers
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from .state import RowBound, latent_size, require_state

DEFAULT_SITE = r"mid_block\.attentions\.0\.transformer_blocks\.0\.attn1$"
DEFAULT_SCALE, DEFAULT_SIGMA, DEFAULT_THRESHOLD = 0.5, 2.0, 1.0
TAPS = 9                     # the blur's kernel size (ST: SAG_TAPS); the latent's sides must exceed its reach of 4


def check_params(sigma, threshold) -> Tuple[float, float]:
    for name, v in (("sigma", sigma), ("threshold", threshold)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
            raise ValueError(f"SAG: {name} must be a finite number, got {v!r}")
    if sigma <= 0:
        raise ValueError(f"SAG: the blur's sigma must be positive, got {sigma!r}")
    return float(sigma), float(threshold)


def site_grid(latent_hw, tokens: int) -> Tuple[int, int]:
    """(th, tw) of a site with `tokens` tokens in a call whose latent is `latent_hw` (seg.site_grid's rule)."""
    from .seg import site_grid as grid
    try:
        return grid(latent_hw, tokens)
    except ValueError as e:
        raise ValueError(str(e).replace("SEG:", "SAG:")) from None


def colsum_reference(q: torch.Tensor, k: torch.Tensor, num_heads: int, sm_scale: float) -> torch.Tensor:
    """Plain torch, the slow path of ops.attention_colsum: the fp32 softmax of (B, T, H*D) projections, summed over the queries and
    averaged over the heads -> (B, T) fp32."""
    B, T, C = q.shape
    d = C // num_heads

    def heads(t):
        return t.float().reshape(B, T, num_heads, d).transpose(1, 2)

    p = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-2, -1)) * sm_scale, dim=-1)
    return p.sum(dim=2).mean(dim=1)


def taps(sigma: float):
    e = [math.exp(-0.5 * (d / sigma) ** 2) for d in range(-(TAPS // 2), TAPS // 2 + 1)]
    total = math.fsum(e)
    return [v / total for v in e]


def degrade_reference(latent: torch.Tensor, eps_neg: torch.Tensor, amap: torch.Tensor, grid_hw, sigma: float, in_scale: float,
                      threshold: float, blur_sigma: float):
    """Plain torch, in the dtype of `latent` (fp64 in the tests): step 2 of the module docstring -> (the second call's input before
    its rounding, the boolean mask (B, lh, lw))."""
    B, C, lh, lw = latent.shape
    th, tw = grid_hw
    x0 = latent - sigma * eps_neg.to(latent.dtype)
    ys = (torch.arange(lh, device=amap.device) * th) // lh
    xs = (torch.arange(lw, device=amap.device) * tw) // lw
    mask = (amap.reshape(B, th, tw) > threshold)[:, ys][:, :, xs].to(latent.device)
    g = torch.tensor(taps(blur_sigma), dtype=latent.dtype, device=latent.device)
    r = TAPS // 2
    pad = torch.nn.functional.pad(x0, (r, r, r, r), mode="reflect")
    blur = sum(g[d] * pad[:, :, :, d:d + lw] for d in range(TAPS))
    blur = sum(g[d] * blur[:, :, d:d + lh, :] for d in range(TAPS))
    out = (torch.where(mask[:, None], blur, x0) + sigma * eps_neg.to(latent.dtype)) * in_scale
    return out, mask


def _device(device) -> torch.device:
    """`device` with its index spelled out, so that "cuda" and "cuda:0" name one binding."""
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


class _Bound:
    """What the state owns for one (rows, latent size) on one device."""

    def __init__(self, rows: int, lh: int, lw: int, grid, heads: int, device):
        th, tw = grid
        from . import ops
        self.grid = grid
        self.A = torch.zeros((rows, th * tw), dtype=torch.float32, device=device)
        self.mask = torch.zeros((rows, lh, lw), dtype=torch.float32, device=device)
        self.workspace = ops.attention_colsum_workspace(rows, th * tw, heads, device) if device.type == "cuda" else None


class SAG(RowBound, nn.Module):
    label = "SAG"

    def __init__(self, site: str = "", layer: str = ""):
        super().__init__()
        self.site, self.layer = site, layer
        self.sites = (site,)
        self.rows = 0
        self.latent_hw = None
        self.sigma, self.threshold = DEFAULT_SIGMA, DEFAULT_THRESHOLD
        # plain dicts under names torch does not know (state.ResidualSites' rule): .to() / state_dict() leave the addresses alone
        self._bound: Dict[tuple, _Bound] = {}
        self._params: Dict[torch.device, torch.Tensor] = {}

    # ---- the current call ----
    @contextlib.contextmanager
    def using(self, rows: int, latent_hw=None):
        """`rows` (the leading batch entries that record A; 0: none) and the latent size of the UNet calls made inside the block;
        the previous values come back afterwards."""
        if isinstance(rows, bool) or not isinstance(rows, int) or rows < 0:
            raise ValueError(f"SAG: rows must be a non-negative integer (0: off), got {rows!r}")
        if rows and latent_hw is None:
            raise ValueError("SAG: using(rows, latent_hw) needs the call's latent size: the site's buffers are bound per size")
        before = (self.rows, self.latent_hw)
        self.rows = rows
        if latent_hw is not None:
            self.latent_hw = latent_size(latent_hw)
        try:
            yield self
        finally:
            self.rows, self.latent_hw = before

    # ---- buffers ----
    def bind(self, rows: int, latent_hw, tokens: int, heads: int, device) -> _Bound:
        """Allocate, outside any capture, A, the mask and the workspace of `rows` recording entries at this latent size (the site
        has `tokens` tokens and `heads` heads) and the device's parameter row; what exists is kept at its address."""
        rows, lh, lw, device = self._parse_bind(rows, latent_hw, device)
        device = _device(device)
        if min(lh, lw) <= TAPS // 2:
            raise ValueError(f"SAG: a {lh} x {lw} latent is no larger than the blur's reach of {TAPS // 2} pixels")
        key = (device, rows, lh, lw)
        if key not in self._bound:
            self._refuse_capture(device)
            self._bound[key] = _Bound(rows, lh, lw, site_grid((lh, lw), tokens), heads, device)
        if device not in self._params:
            self._refuse_capture(device, "the parameter row")
            self._params[device] = torch.tensor([self.threshold, self.sigma], dtype=torch.float32, device=device)
        return self._bound[key]

    def bound_rows(self):
        return sorted({key[1] for key in self._bound})

    def bound(self, rows: int, latent_hw, device) -> _Bound:
        lh, lw = latent_size(latent_hw)
        got = self._bound.get((_device(device), int(rows), lh, lw))
        if got is None:
            raise ValueError(f"SAG: nothing is bound for {rows} rows at a {lh} x {lw} latent on {device} (bound: "
                             f"{sorted(k[1:] for k in self._bound)}); call bind(rows, latent_hw, tokens, heads, device) first")
        return got

    def params(self, device) -> torch.Tensor:
        """The device row (threshold, blur sigma) `sag_degrade` reads."""
        device = _device(device)
        if device not in self._params:
            raise ValueError(f"SAG: nothing is bound on {device}; call bind(rows, latent_hw, tokens, heads, device) first")
        return self._params[device]

    def set_params(self, sigma: Optional[float] = None, threshold: Optional[float] = None) -> None:
        """The blur's sigma and / or the threshold: validated, then written into every bound parameter row in place."""
        self.sigma, self.threshold = check_params(self.sigma if sigma is None else sigma, self.threshold if threshold is None else threshold)
        for row in self._params.values():
            row.copy_(torch.tensor([self.threshold, self.sigma], dtype=torch.float32))

    @property
    def mask(self) -> torch.Tensor:
        """The 1 / 0 map (rows, lh, lw) the last degrade launch used; with several bindings, the most recent one's."""
        if not self._bound:
            raise ValueError("SAG: nothing is bound")
        return next(reversed(self._bound.values())).mask

    def extra_repr(self) -> str:
        return f"site={self.site!r}, rows={self.rows}, sigma={self.sigma}, threshold={self.threshold}, bound={sorted(k[1:] for k in self._bound)}"


def attention_sag_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                          state: SAG) -> torch.Tensor:
    """fx leaf: attention_wrapper that also records A for the leading state.rows batch entries."""
    rows = state.rows
    if rows > q.shape[0]:
        raise ValueError(f"SAG: rows = {rows} of a UNet batch of {q.shape[0]}")
    if q.device.type == "cpu":
        from .pag import identity_attention_reference
        out = identity_attention_reference(q, k, v, num_heads, sm_scale, 0)
        if rows:
            b = state.bind(rows, state.latent_hw, q.shape[1], num_heads, q.device)
            b.A.copy_(colsum_reference(q[:rows], k[:rows], num_heads, sm_scale))
        return out
    from . import ops
    if q.shape[-1] != num_heads * head_dim:
        raise ops.BackendError(f"attention_sag_wrapper: C={q.shape[-1]} != num_heads*head_dim={num_heads * head_dim}")
    out = ops.attention(q, k, v, num_heads, sm_scale)
    if rows:
        b = state.bound(rows, state.latent_hw, q.device) if torch.cuda.is_current_stream_capturing() else state.bind(
            rows, state.latent_hw, q.shape[1], num_heads, q.device)
        if b.A.shape[1] != q.shape[1]:
            raise ValueError(f"SAG: the site has {q.shape[1]} tokens, the buffers bound for this latent size {b.A.shape[1]}")
        ops.attention_colsum(q[:rows], k[:rows], num_heads, sm_scale, out=b.A, workspace=b.workspace)      # (views: the leading sub-batch)
    return out


torch.fx.wrap("attention_sag_wrapper")


def degrade(state: SAG, latent: torch.Tensor, eps_neg: torch.Tensor, sigmas: torch.Tensor, in_scale: torch.Tensor, step: torch.Tensor,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """For a caller that orchestrates the second UNet call itself (as tiles.gather / tiles.blend and inpaint.blend are exposed): the
    second call's input from the fp32 latent (B, 4, lh, lw), the negative prediction `eps_neg` of the call that has just recorded A
    under `state.using(B, latent_hw)`, the fp32 tables `sigmas` / `in_scale` and the int32 device counter `step`.  Tensors are made
    channels_last where they are not; the mask that was used is `state.mask`."""
    from . import ops
    B, _, lh, lw = latent.shape
    b = state.bound(B, (lh, lw), latent.device)
    cl = torch.channels_last
    latent, eps_neg = latent.contiguous(memory_format=cl), eps_neg.contiguous(memory_format=cl)
    if out is None:
        out = torch.empty_like(eps_neg, memory_format=cl)
    ops.sag_degrade(latent, eps_neg, b.A, b.grid, sigmas, in_scale, step, state.params(latent.device), out, b.mask)
    return out


def state_of(module, what: str) -> SAG:
    """The SAG state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "sag", SAG, what, "a self-attention guidance site", "sag_layer=True")
