"""Reference-only control inside the compiled UNet: steering by a reference image with no extra weights (A1111's ControlNet
`reference_only`, ComfyUI's `ReferenceOnlySimple`, diffusers' community `stable_diffusion_xl_reference` pipeline).

The noised reference latent rides through the UNet as one more block of batch rows.  In the selected self-attention (`attn1`)
sites every generated row attends to its own tokens AND to the reference row's tokens under one softmax:
`attn1(x) = Attn(q, [k | k_ref], [v | v_ref])`; the reference rows themselves run ordinary self-attention.

Batch layout: the reference rows are the LAST `B // chunks` batch entries of a UNet call - `chunks` = 3 for
[negative | positive | reference], 2 for [positive | reference], 0 for ordinary attention.  With R = B // chunks and
lead = B - R, entry b < lead attends to [own | entry lead + b % R].  `chunks` is a host integer of the state module
`gm.reference`, fixed for a capture; callers that share one compiled module set it for the duration of their own UNet calls with
`state.using(chunks, step=..., table=...)`.  `step` / `table` are the device gate of ops.attention_joint: an int32 counter and an fp32
table read at every launch; where table[*step] == 0 the sites run ordinary attention and the reference rows' keys are never read.
Without them the state's own one-entry table (1 = on) and zero counter are used.

`attention_reference_wrapper` is the fx leaf optimizers/insert_reference.py puts in place of `attention_wrapper` at the selected
sites: HIP (ops.attention_joint, csrc/attention_joint.hip) for device tensors, a plain torch statement for CPU tensors so that a
traced CPU module can carry the pass on its own.  With chunks == 0 it is ops.attention: the launch and the bits of a module
compiled without the pass.

Parity with A1111, ComfyUI and diffusers is unpinned (each noises, orders and weights the reference its own way); their
`style_fidelity`, a continuous strength and the AdaIN (GroupNorm statistics) variant are out of scope.
"""
from __future__ import annotations

import contextlib

import torch

from .pag import PerturbedRows
from .state import require_state


class ReferenceRows(PerturbedRows):
    """The last B // chunks batch entries of a call are reference rows; the others also attend to them at the selected sites.
    `gate`: the (step, table) device tensors of the current calls, or None = the state's own always-on pair."""
    label = "reference"
    reference_count = PerturbedRows.tail_count

    def __init__(self, sites=(), layers=()):
        super().__init__(sites, layers)
        self.gate = None
        self._own = {}

    def own_gate(self, device: torch.device):
        """The state's own (zero step, one-entry table = 1) on `device`: made at the first call there, which must not be captured."""
        key = (device.type, device.index)
        if key not in self._own:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("reference: run one call outside the capture first (the state's own gate is allocated there), or "
                                   "pass step= / table= to using()")
            self._own[key] = (torch.zeros(1, dtype=torch.int32, device=device), torch.ones(1, dtype=torch.float32, device=device))
        return self._own[key]

    @contextlib.contextmanager
    def using(self, chunks: int, *, step=None, table=None):
        """`chunks`, and the device gate (`step` int32 of one entry, `table` fp32 (n,); both or neither, keyword-only: the base
        class's second positional argument is a latent size), of the calls made inside the block; the previous values come back
        afterwards."""
        if (step is None) != (table is None):
            raise ValueError("reference.using: pass step= and table= together, or neither")
        before = (self.chunks, self.gate)
        self.set_chunks(chunks)
        self.gate = None if step is None else (step, table)
        try:
            yield self
        finally:
            self.chunks, self.gate = before


def joint_attention_reference(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k2: torch.Tensor, v2: torch.Tensor, num_heads: int,
                              sm_scale: float, lead: int) -> torch.Tensor:
    """Plain torch: the attention core on (B, T, H*D) projections whose first `lead` batch entries attend to [k[b] ; k2[b % B2]]."""
    B, T, C = q.shape
    d = C // num_heads

    def core(q_, k_, v_):
        def heads(t):
            return t.reshape(t.shape[0], t.shape[1], num_heads, d).transpose(1, 2)
        w = torch.softmax(torch.matmul(heads(q_), heads(k_).transpose(-2, -1)) * sm_scale, dim=-1)
        return torch.matmul(w, heads(v_)).transpose(1, 2).reshape(q_.shape[0], T, C)

    outs = []
    if lead > 0:
        rows = torch.arange(lead, device=q.device) % k2.shape[0]
        outs.append(core(q[:lead], torch.cat([k[:lead], k2[rows]], dim=1), torch.cat([v[:lead], v2[rows]], dim=1)))
    if lead < B:
        outs.append(core(q[lead:], k[lead:], v[lead:]))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def attention_reference_wrapper(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, output, sm_scale: float, num_heads: int, head_dim: int,
                                state: ReferenceRows) -> torch.Tensor:
    """fx leaf: attention_wrapper whose leading batch entries also attend to the last B // state.chunks entries' keys."""
    B = q.shape[0]
    ref = state.reference_count(B)
    lead = B - ref
    if q.device.type == "cpu":
        if ref == 0 or lead == 0:
            return joint_attention_reference(q, k, v, k, v, num_heads, sm_scale, 0)
        joint = joint_attention_reference(q, k, v, k[lead:], v[lead:], num_heads, sm_scale, lead)
        if state.gate is None:
            return joint
        step, table = state.gate
        on = table.index_select(0, step.reshape(1).long().clamp(0, table.numel() - 1)) != 0
        return torch.where(on, joint, joint_attention_reference(q, k, v, k, v, num_heads, sm_scale, 0))
    from . import ops
    if q.shape[-1] != num_heads * head_dim:
        raise ops.BackendError(f"attention_reference_wrapper: C={q.shape[-1]} != num_heads*head_dim={num_heads * head_dim}")
    if ref == 0 or lead == 0:
        return ops.attention(q, k, v, num_heads, sm_scale)
    gate = state.gate if state.gate is not None else state.own_gate(q.device)
    return ops.attention_joint(q, k, v, k[lead:], v[lead:], num_heads, sm_scale, lead=lead, gate=gate)


torch.fx.wrap("attention_reference_wrapper")


def state_of(module, what: str) -> ReferenceRows:
    """The reference state of a compiled module, or a ValueError that names the missing compile argument."""
    return require_state(module, "reference", ReferenceRows, what, "reference-only sites", 'reference_layers=(".*",)')
