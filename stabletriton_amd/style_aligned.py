"""StyleAligned inside the compiled UNet: the images of one batch drawn toward the style of the first, with no extra weights
(Hertz et al., "Style Aligned Image Generation via Shared Attention", 2023; diffusers' community `pipeline_sdxl_style_aligned`,
ComfyUI's "StyleAligned Batch Align" node).

A UNet call's batch is cut into blocks of `per` entries - one block per row block of a guided call, [negative | positive] - and the
first entry of a block is its style row.  In the selected self-attention (`attn1`) sites every other entry b, with s = b - b % per:
  1. AdaIN of queries and keys (option `adain` = "qk"; "qkv": the values too; None: skipped) along the token axis, per channel of
     H*D: x[b] <- (x[b] - mu[b]) / sd[b] * sd[s] + mu[s], sd = sqrt(unbiased variance + 1e-5) - the published values;
  2. shared attention: `attn1(x)[b] = Attn(q[b], [k[b] | k[s]], [v[b] | v[s]])` under one softmax.
Style rows run ordinary self-attention on untouched q / k, so the style image does not depend on the others.

`per` is a host integer of the state module `gm.style_aligned`, fixed for a capture (0: ordinary attention); callers that share one
compiled module set it for the duration of their own UNet calls with `state.using(per, step=..., table=...)`.  `step` / `table` are
the device gate of ops.attention_joint: where table[*step] == 0 the sites run ordinary attention on untouched q / k.  Without them
the state's own one-entry table (1 = on) and zero counter are used.

`attention_style_wrapper` is the fx leaf optimizers/insert_style_aligned.py puts in place of `attention_wrapper` at the selected
sites: HIP (ops.style_adain in place on the q and k columns of the fused projection buffer, csrc/style_adain.hip, then
ops.attention_shared, csrc/attention_joint.hip) for device tensors, plain torch statements for CPU tensors so that a traced CPU module
can carry the pass on its own.  With per <= 1 it is ops.attention: the launch and the bits of a module compiled without the pass.

Out of scope: shared GroupNorm / LayerNorm statistics (`share_group_norm` / `share_layer_norm`), `shared_score_scale` /
`shared_score_shift`, `full_attention_share` and `only_self_level`.  In the ComfyUI node's terms this is `share_attn` = q+k (or
q+k+v) with `share_norm` = disabled.  Parity with either published implementation is unpinned.
"""
from __future__ import annotations

import contextlib
from typing import Sequence

import torch
from torch import nn

from .state import require_state

ADAIN_EPS = 1e-5
ADAIN_OPTIONS = ("qk", "qkv", None)


class StyleAligned(nn.Module):
    """State of one compiled module with StyleAligned sites: the selected site names and their channel widths, the option `adain`, and
    the host values `per` and `gate` of the current call.  `gate`: the (step, table) device tensors, or None = the state's own
    always-on pair."""
    label = "style_aligned"

    def __init__(self, sites: Sequence[str] = (), layers: Sequence[str] = (), channels: Sequence[int] = (), adain="qk"):
        super().__init__()
        self.sites = tuple(sites)
        self.layers = tuple(layers)
        self.channels = tuple(int(c) for c in channels)
        self.per = 0
        self.gate = None
        self.set_adain(adain)
        self._own = {}
        self._workspace = {}                               # device -> fp32 scratch of ops.style_adain, read by address

    def set_adain(self, adain) -> None:
        if adain not in ADAIN_OPTIONS:
            raise ValueError(f"style_aligned: adain must be one of {ADAIN_OPTIONS}, got {adain!r}")
        self.adain = adain

    def set_per(self, per: int) -> None:
        if isinstance(per, bool) or not isinstance(per, int) or per < 0:
            raise ValueError(f"style_aligned: per must be a non-negative integer (0: off; rows per block, the first is the style row), got {per!r}")
        self.per = per

    def own_gate(self, device: torch.device):
        """The state's own (zero step, one-entry table = 1) on `device`: made at the first call there, which must not be captured."""
        key = (device.type, device.index)
        if key not in self._own:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("style_aligned: run one call outside the capture first (the state's own gate is allocated there), or "
                                   "pass step= / table= to using()")
            self._own[key] = (torch.zeros(1, dtype=torch.int32, device=device), torch.ones(1, dtype=torch.float32, device=device))
        return self._own[key]

    def bind(self, rows: int, latent_hw, device) -> None:
        """Allocate, outside any capture, the AdaIN scratch for UNet calls of `rows` rows at this latent size: sized for the widest
        site at the latent's own token count, which bounds every site (a level halves the tokens per side and at most doubles the
        channels).  A scratch that is large enough is kept: captured graphs read it by address."""
        from .state import latent_size
        lh, lw = latent_size(latent_hw)
        self.workspace(int(rows), lh * lw, max(self.channels, default=8), 3, torch.device(device))

    def workspace(self, B: int, T: int, C: int, n_slices: int, device: torch.device) -> torch.Tensor:
        """The scratch on `device`, grown (outside a capture only) when this call needs more than it holds."""
        from . import _C, ops
        need = _C.load().st_style_adain_workspace(B, T, C, n_slices)
        key = (device.type, device.index)
        have = self._workspace.get(key)
        if have is None or have.numel() < need:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("style_aligned: the AdaIN scratch is too small for this call; bind(rows, latent_hw, device) or run one "
                                   "call outside the capture first")
            have = self._workspace[key] = ops.style_adain_workspace(B, T, C, n_slices, device)
        return have

    @contextlib.contextmanager
    def using(self, per: int, *, step=None, table=None):
        """`per`, and the device gate (`step` int32 of one entry, `table` fp32 (n,); both or neither), of the calls made inside the
        block; the previous values come back afterwards."""
        if (step is None) != (table is None):
            raise ValueError("style_aligned.using: pass step= and table= together, or neither")
        before = (self.per, self.gate)
        self.set_per(per)
        self.gate = None if step is None else (step, table)
        try:
            yield self
        finally:
            self.per, self.gate = before

    def extra_repr(self) -> str:
        return f"sites={len(self.sites)}, per={self.per}, adain={self.adain!r}"


def _style_rows(B: int, per: int, device) -> torch.Tensor:
    rows = torch.arange(B, device=device)
    return rows - rows % per


def adain_reference(x: torch.Tensor, per: int, eps: float = ADAIN_EPS) -> torch.Tensor:
    """Plain torch, out of place: x (B, T, C) with every entry b, b % per != 0, renormalised along the token axis to the mean and
    standard deviation (sqrt(unbiased variance + eps)) of entry b - b % per; the style rows are returned as they are."""
    B = x.shape[0]
    style = _style_rows(B, per, x.device)
    mu = x.mean(dim=1, keepdim=True)
    sd = (x.var(dim=1, unbiased=True, keepdim=True) + eps).sqrt()
    out = (x - mu) / sd * sd.index_select(0, style) + mu.index_select(0, style)
    return torch.where((style == torch.arange(B, device=x.device)).reshape(B, 1, 1), x, out)


def shared_attention_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, sm_scale: float, per: int) -> torch.Tensor:
    """Plain torch: the attention core on (B, T, H*D) projections where entry b, b % per != 0, attends to [k[b] ; k[b - b % per]]
    and the first entry of every block of `per` to k[b] alone."""
    B, T, C = q.shape
    d = C // num_heads

    def core(q_, k_, v_):
        def heads(t):
            return t.reshape(t.shape[0], t.shape[1], num_heads, d).transpose(1, 2)
        w = torch.softmax(torch.matmul(heads(q_), heads(k_).transpose(-2, -1)) * sm_scale, dim=-1)
        return torch.matmul(w, heads(v_)).transpose(1, 2).reshape(q_.shape[0], T, C)

    plain = core(q, k, v)
    if per <= 1 or B == 1:
        return plain
    style = _style_rows(B, per, q.device)
    joint = core(q, torch.cat([k, k.index_select(0, style)], dim=1), torch.cat([v, v.index_select(0, style)], dim=1))
    return torch.where((style == torch.arange(B, device=q.device)).reshape(B, 1, 1), plain, joint)


def attention_style_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                            state: StyleAligned) -> torch.Tensor:
    """fx leaf: attention_wrapper whose entries renormalise q / k to, and share the keys of, the first entry of their block of
    state.per."""
    per = state.per
    if q.device.type == "cpu":
        plain = shared_attention_reference(q, k, v, num_heads, sm_scale, 1)
        if per <= 1:
            return plain
        qa, ka = (adain_reference(t, per) for t in (q, k)) if state.adain else (q, k)
        va = adain_reference(v, per) if state.adain == "qkv" else v
        on_rows = shared_attention_reference(qa, ka, va, num_heads, sm_scale, per)
        if state.gate is None:
            return on_rows
        step, table = state.gate
        on = table.index_select(0, step.reshape(1).long().clamp(0, table.numel() - 1)) != 0
        return torch.where(on, on_rows, plain)
    from . import ops
    if q.shape[-1] != num_heads * head_dim:
        raise ops.BackendError(f"attention_style_wrapper: C={q.shape[-1]} != num_heads*head_dim={num_heads * head_dim}")
    if per <= 1:
        return ops.attention(q, k, v, num_heads, sm_scale)
    gate = state.gate if state.gate is not None else state.own_gate(q.device)
    if state.adain:
        B, T, C = q.shape
        n = 3 if state.adain == "qkv" else 2
        scratch = state.workspace(B, T, C, n, q.device) if q.dtype != torch.float32 else None      # (strict mode: the slow path)
        if n == 3:
            q, k, v = ops.style_adain((q, k, v), per, gate=gate, workspace=scratch)
        else:
            q, k = ops.style_adain((q, k), per, gate=gate, workspace=scratch)
    return ops.attention_shared(q, k, v, num_heads, sm_scale, per, gate=gate)


torch.fx.wrap("attention_style_wrapper")


def state_of(module, what: str) -> StyleAligned:
    """The StyleAligned state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "style_aligned", StyleAligned, what, "StyleAligned sites", 'style_aligned_layers=(".*",)')
