"""Perturbed-attention guidance (PAG; Ahn et al., "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance", 2024)
inside the compiled UNet.

The UNet evaluates one more block of batch rows, the "perturbed" prediction: the positive conditioning and the same latent, but
in the selected self-attention (`attn1`) sites the softmax matrix of those rows is the identity, so the attention core returns
`v` and `attn1(x) = to_out(to_v(x))` (diffusers' PAGCFGIdentitySelfAttnProcessor2_0).  The sampler then adds
`s * (e_pos - e_pert)` to the guided prediction (diffusers' PAGMixin; pipeline.DenoiseLoop does it in the update launch).

Batch layout: the perturbed rows are the LAST `B // chunks` batch entries of a UNet call - `chunks` = 3 for
[negative | positive | perturbed], 2 for [positive | perturbed], 1 for a fully perturbed call (ComfyUI's node), 0 for ordinary
attention.  `chunks` is a host integer of the state module `gm.pag`: the layout is a property of the caller's batch, fixed for a
capture.  Callers that share one compiled module set it for the duration of their own UNet calls with `state.using(chunks)`.

`attention_pag_wrapper` is the fx leaf optimizers/insert_pag.py puts in place of `attention_wrapper` at the selected sites: HIP
(ops.attention_pag, csrc/pag.hip) for device tensors, a plain torch statement for CPU tensors so that a traced CPU module can carry
the pass on its own.  With chunks == 0 it is ops.attention: the launch and the bits of a module compiled without the pass.
"""
from __future__ import annotations

import contextlib
from typing import Sequence

import torch
from torch import nn

from .state import require_state

TRAIN_TIMESTEPS = 1000      # diffusers' adaptive rule counts down from the training schedule's length


class PerturbedRows(nn.Module):
    """State of one compiled module whose selected self-attention sites perturb the last B // chunks batch entries of a call (PAG
    here, seg.SEG): the selected site names (attn1 module paths) and the host values `chunks` and `latent_hw` of the current call."""
    label = ""

    def __init__(self, sites: Sequence[str] = (), layers: Sequence[str] = ()):
        super().__init__()
        self.sites = tuple(sites)
        self.layers = tuple(layers)
        self.chunks = 0
        self.latent_hw = None

    def set_chunks(self, chunks: int) -> None:
        if isinstance(chunks, bool) or not isinstance(chunks, int) or chunks < 0:
            raise ValueError(f"{self.label}: chunks must be a non-negative integer (0: off; the last B // chunks batch entries are perturbed), got {chunks!r}")
        self.chunks = chunks

    @contextlib.contextmanager
    def using(self, chunks: int, latent_hw=None):
        """`chunks` and the latent size of the calls made inside the block; the previous values come back afterwards (owners that
        share one compiled module do not disturb each other)."""
        before = (self.chunks, self.latent_hw)
        self.set_chunks(chunks)
        if latent_hw is not None:
            self.latent_hw = (int(latent_hw[0]), int(latent_hw[1]))
        try:
            yield self
        finally:
            self.chunks, self.latent_hw = before

    def tail_count(self, batch: int) -> int:
        """How many trailing batch entries of a call with `batch` entries are perturbed."""
        c = self.chunks
        if c == 0:
            return 0
        if batch % c != 0:
            raise ValueError(f"{self.label}: a UNet batch of {batch} rows does not divide into {c} chunks")
        return batch // c

    def extra_repr(self) -> str:
        return f"sites={len(self.sites)}, chunks={self.chunks}"


class PAG(PerturbedRows):
    """The perturbed rows return v; nothing depends on the latent size (`latent_hw` is carried and never read)."""
    label = "PAG"
    ident_count = PerturbedRows.tail_count


def identity_attention_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, sm_scale: float, ident: int) -> torch.Tensor:
    """Plain torch: the attention core on (B, T, H*D) projections whose last `ident` batch entries return v."""
    B, T, C = q.shape
    lead = B - ident
    d = C // num_heads
    outs = []
    if lead > 0:
        def heads(t):
            return t[:lead].reshape(lead, t.shape[1], num_heads, d).transpose(1, 2)
        w = torch.softmax(torch.matmul(heads(q), heads(k).transpose(-2, -1)) * sm_scale, dim=-1)
        outs.append(torch.matmul(w, heads(v)).transpose(1, 2).reshape(lead, T, C))
    if ident > 0:
        outs.append(v[lead:])
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def attention_pag_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                          state: PAG) -> torch.Tensor:
    """fx leaf: attention_wrapper whose last B // state.chunks batch entries are perturbed (out = v)."""
    ident = state.ident_count(q.shape[0])
    if q.device.type == "cpu":
        return identity_attention_reference(q, k, v, num_heads, sm_scale, ident)
    from . import ops
    if q.shape[-1] != num_heads * head_dim:
        raise ops.BackendError(f"attention_pag_wrapper: C={q.shape[-1]} != num_heads*head_dim={num_heads * head_dim}")
    if ident == 0:
        return ops.attention(q, k, v, num_heads, sm_scale)
    return ops.attention_pag(q, k, v, num_heads, sm_scale, ident)


torch.fx.wrap("attention_pag_wrapper")


def adaptive_scales(timesteps, pag_scale: float, pag_adaptive_scale: float = 0.0):
    """The per-step table of diffusers' `_get_pag_scale`: s_i = max(0, pag_scale - pag_adaptive_scale * (1000 - t_i)) when
    pag_adaptive_scale > 0, else pag_scale at every step."""
    ts = [float(t) for t in timesteps]
    if pag_adaptive_scale > 0:
        return [max(0.0, float(pag_scale) - float(pag_adaptive_scale) * (TRAIN_TIMESTEPS - t)) for t in ts]
    return [float(pag_scale)] * len(ts)


def state_of(module, what: str) -> PAG:
    """The PAG state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "pag", PAG, what, "perturbed-attention sites", 'pag_layers=("mid",)')
