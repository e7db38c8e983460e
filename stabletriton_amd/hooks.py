"""Host hooks: drop the compiled UNet into the call sites that drive it.

Diffusers - reference call site implementations/Diffusers/load_sdxl_pipeline.py:17-46: an fp16 SDXL pipeline whose
`pipe.unet` is replaced by the compiled module with three `config` attributes re-attached.  The pipeline
(diffusers 0.21.2, third party) then calls, once per step and with classifier-free guidance (batch 2):

    unet(latent_model_input, t, encoder_hidden_states=prompt_embeds, cross_attention_kwargs=None,
         added_cond_kwargs={"text_embeds": ..., "time_ids": ...}, return_dict=False)[0]

`DiffusersUNet` answers exactly that call.  With an fp16 module (the reference's own line: `.half().cuda()`) the HIP
kernels compute in fp16 and nothing is cast at this boundary; a bf16 or fp32 (strict parity) module takes the pipeline's
fp16 tensors through one cast in and one cast out.  The text-context K/V projections (140 GEMMs, step-invariant) are evaluated once per prompt - the cache is keyed
on the identity (a held reference, not the address) and version of `encoder_hidden_states` - and every step replays ONE captured hipGraph.

ComfyUI - the reference's hook is an empty file (implementations/ComfyUI/example.py), so the contract here is ComfyUI's
own `diffusion_model.forward(x, timesteps, context, y, control, transformer_options, **kw)`: `y` is the ready-made
2816-wide vector (pooled text embedding | Fourier features of the six size/crop ids), timesteps has one entry per row.
`ComfyUNet` wraps a module compiled from `UNetWithLabelVector` (same weights, `y` instead of added_cond_kwargs).

Both packages are duck-typed (neither is a dependency).
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import torch
from torch import nn

from .optimization import optimize_model
from .optimizers.graphs import make_dynamic_graphed_callable
from .state import compiled_state
from .unet import SDXL_BASE, UNet2DConditionModel, UNetSpec, UNetWithLabelVector, make_config


class _HoistedUNet(nn.Module):
    """Shared by both adapters: dtype casts at the boundary, per-prompt context cache, one captured graph per input shape."""

    def __init__(self, compiled, compute_dtype: torch.dtype, cuda_graph: bool = True):
        super().__init__()
        if not hasattr(compiled, "forward_with_context"):
            raise ValueError("expected a module from optimize_model(..., cuda_graph=False): the adapter captures its own graphs")
        self.compiled = compiled
        self.compute_dtype = compute_dtype
        self.cuda_graph = cuda_graph
        self._ctx: Dict[tuple, tuple] = {}        # ehs shape -> static context tensors (read by the captured graphs)
        # per shape: the tensor the cached context was built from, HELD (not its address: the caching allocator hands the
        # next prompt's tensor the address of a freed one, with _version 0 again), the version it had then, and a private
        # copy of its contents, to recognise the same prompt in a new tensor object.  Per shape: a caller that alternates
        # two context shapes (cond / uncond batches of different lengths) keeps both.
        self._ctx_src: Dict[tuple, torch.Tensor] = {}
        self._ctx_version: Dict[tuple, int] = {}
        self._ctx_copy: Dict[tuple, torch.Tensor] = {}
        self._steps: Dict[tuple, object] = {}     # ehs shape -> (graphed) step function
        self._new_prompt = False                  # set when a context was (re)projected: the fp8 plan measures its scales again
        self._last_t = None                       # fp8 plan only: the last call's (largest) timestep, to tell where a trajectory starts
        self._perturbed_chunks = 0                # enable_pag / enable_seg: the last B // chunks rows of a call are perturbed (0: none)
        self._regions = None                      # set_regions: (masks, chunks), applied to the buffers of a call's (rows, latent size)
        self._regions_applied = {}                # ... rows -> the latent size the buffers of that row count were last written for
        self._ip_images = {}                      # set_ip_adapter_image: slot -> (tokens, negative_tokens, chunks)
        self._ip_masks = {}                       # set_ip_adapter_masks: slot -> masks
        self._ip_applied = {}                     # ... rows -> the latent size the buffers of that row count were last written for
        self._residuals_last = None               # T2I-Adapter / ControlNet: (state, rows, the residual tensors last copied - HELD, not their addresses -, their versions)

    def refresh_weights(self) -> int:
        """Re-derive fused / folded weight buffers after an in-place weight update (also done at every new prompt).
        The hoisted text-context K/V were projected with the old weights: the next call recomputes them (and, with the fp8
        plan, measures the activation scales again)."""
        self._ctx_src.clear()
        self._ctx_copy.clear()
        return self.compiled.exec_context.refresh_derived(full=True)

    # ---- LoRA adapters (lora.py): merged in place; the captured graphs stay, the hoisted K/V are projected again -------
    def _lora_set(self):
        from . import lora
        return lora.attach(self.compiled)

    def load_lora(self, name: str, state_dict, scale: float = 1.0, strict: bool = True, convs: bool = False, lycoris: bool = False):
        """Merge a LoRA state dict (PEFT / diffusers / kohya keys; DoRA magnitudes apply) into the compiled UNet; `convs=True`
        also takes its convolution factors (LoCon), `lycoris=True` its Tucker cores, LoHa and LoKr factors.  Returns the keys
        not applied."""
        left = self._lora_set().load(name, state_dict, scale, strict, convs, lycoris)
        self.refresh_weights()
        return left

    def set_lora_scale(self, name: str, scale: float) -> None:
        self._lora_set().set_scale(name, scale)
        self.refresh_weights()

    def unload_lora(self, name: str) -> None:
        self._lora_set().unload(name)
        self.refresh_weights()

    # ---- FreeU (freeu.py): a device row the compiled graph reads by address; the captured graphs stay ------------------
    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float, version: int = 1) -> None:
        """diffusers' `UNet2DConditionModel.enable_freeu(s1, s2, b1, b2)`; version 2 = ComfyUI's FreeU_V2 backbone rule.
        Raises on a wrapper compiled without `freeu=True` (the sites are part of the compiled graph)."""
        from . import freeu
        freeu.state_of(self.compiled, "enable_freeu").set(s1, s2, b1, b2, version)

    def disable_freeu(self) -> None:
        from . import freeu
        freeu.state_of(self.compiled, "disable_freeu").disable()

    # ---- perturbed-attention guidance (pag.py): which rows of a call are the perturbed ones; one captured graph per setting ----
    def enable_pag(self, chunks: int) -> None:
        """The last B // chunks batch rows of every following call take the perturbed self-attention (out = v at the sites
        compiled in with `pag_layers`): 3 for diffusers' PAG pipelines with guidance ([uncond | cond | cond]), 2 without
        ([cond | cond]), 1 for a fully perturbed call (ComfyUI's PerturbedAttentionGuidance node).  Only the UNet is evaluated
        here: the guidance combine stays with the calling pipeline.  Raises on a wrapper compiled without `pag_layers`."""
        from . import pag
        pag.state_of(self.compiled, "enable_pag")
        if isinstance(chunks, bool) or not isinstance(chunks, int) or chunks < 1:
            raise ValueError(f"enable_pag: chunks must be a positive integer (3, 2 or 1), got {chunks!r}")
        self._perturbed_chunks = chunks       # (the state's own `chunks` is set around this wrapper's calls only: _perturbed_scope)

    def disable_pag(self) -> None:
        from . import pag
        pag.state_of(self.compiled, "disable_pag")
        self._perturbed_chunks = 0

    def _perturbed_scope(self, chunks: int, latent_hw):
        """The PAG, SEG or reference state's `using` (a module has at most one of them) around this wrapper's own calls."""
        from . import pag, reference, seg
        ref = compiled_state(self.compiled, "reference", reference.ReferenceRows)
        if ref is not None:
            return ref.using(chunks)
        state = compiled_state(self.compiled, "pag", pag.PAG) or compiled_state(self.compiled, "seg", seg.SEG)
        return state.using(chunks, latent_hw) if state is not None else contextlib.nullcontext()

    # ---- reference-only control (reference.py): which rows of a call are the reference rows; one captured graph per setting ----
    def enable_reference(self, chunks: int) -> None:
        """The last B // chunks batch rows of every following call are reference rows: at the sites compiled in with
        `reference_layers` every other row attends to its own tokens and to the tokens of its reference row (row lead + b % (B //
        chunks), lead = B - B // chunks) under one softmax; 3 for [uncond | cond | reference], 2 for [generated | reference].  The
        caller orders its batch with the reference rows last, noises them itself and drops their prediction.  Raises on a wrapper
        compiled without `reference_layers`."""
        from . import reference
        reference.state_of(self.compiled, "enable_reference")
        if isinstance(chunks, bool) or not isinstance(chunks, int) or chunks < 2:
            raise ValueError(f"enable_reference: chunks must be an integer of 2 or more (3 or 2), got {chunks!r}")
        self._perturbed_chunks = chunks

    def disable_reference(self) -> None:
        from . import reference
        reference.state_of(self.compiled, "disable_reference")
        self._perturbed_chunks = 0

    def _apply_reference(self, sample: torch.Tensor) -> None:
        """The state's own always-on gate on this call's device: allocated outside any capture (the sites only look it up)."""
        from . import reference
        state = compiled_state(self.compiled, "reference", reference.ReferenceRows)
        if state is not None and self._perturbed_chunks and not torch.cuda.is_current_stream_capturing():
            state.own_gate(sample.device)

    # ---- smoothed energy guidance (seg.py): which rows of a call take blurred queries; sigma is a device row, written in place ----
    def enable_seg(self, chunks: int, sigma: float = float("inf")) -> None:
        """The last B // chunks batch rows of every following call take the smoothed-energy self-attention (queries Gaussian-blurred
        over the latent grid at the sites compiled in with `seg_layers`; sigma = infinity: their spatial mean): 3 for a pipeline
        with guidance ([uncond | cond | cond]), 2 without ([cond | cond]), 1 for a fully perturbed call (ComfyUI's SEG node makes
        one).  Only the UNet is evaluated here: the guidance combine stays with the calling pipeline.  One captured graph per
        `chunks`; sigma needs none (`set_seg_sigma`).  Raises on a wrapper compiled without `seg_layers`."""
        from . import seg
        state = seg.state_of(self.compiled, "enable_seg")
        if isinstance(chunks, bool) or not isinstance(chunks, int) or chunks < 1:
            raise ValueError(f"enable_seg: chunks must be a positive integer (3, 2 or 1), got {chunks!r}")
        state.set_sigma(sigma)
        self._perturbed_chunks = chunks

    def set_seg_sigma(self, sigma: float) -> None:
        """The blur's sigma for the following calls: an in-place write of the parameter rows the captured graphs read by address."""
        from . import seg
        seg.state_of(self.compiled, "set_seg_sigma").set_sigma(sigma)

    def disable_seg(self) -> None:
        from . import seg
        seg.state_of(self.compiled, "disable_seg")
        self._perturbed_chunks = 0

    def _apply_seg(self, sample: torch.Tensor) -> None:
        """Allocate the parameter rows of this call's latent size, outside any capture (the sites only look them up)."""
        from . import seg
        state = compiled_state(self.compiled, "seg", seg.SEG)
        if state is None or not self._perturbed_chunks or torch.cuda.is_current_stream_capturing():
            return
        state.bind((int(sample.shape[-2]), int(sample.shape[-1])), sample.device)

    # ---- regional prompts (regions.py): weight buffers the cross-attention sites read by address; the captured graphs stay ----
    def set_regions(self, masks: torch.Tensor, chunks: int = 2) -> None:
        """Region masks, (R, lh, lw) or (batch, R, lh, lw) at latent resolution, for every following call whose
        `encoder_hidden_states` is the R prompts concatenated along the token axis.  `chunks` says how a call's batch divides,
        as in `enable_pag`: 2 = [uncond | cond], 3 = [uncond | cond | cond (perturbed)] - the first block is the negative one and
        keeps segment 0, the others take the masks; 1 = every row takes them (a call without a negative block).  The buffers of a
        batch size and latent size are allocated at the first call that has them, and written in place; a call whose latent is
        not the masks' size raises.  Raises on a wrapper compiled without `regions=R`."""
        from . import regions
        st = regions.state_of(self.compiled, "set_regions")
        regions.positive_rows(chunks, chunks)                    # (validates chunks)
        masks = torch.as_tensor(masks)
        regions._as_batched(masks, st.R, "set_regions")          # (validates the masks now, not at the next call)
        self._regions = (masks, chunks)
        self._regions_applied = {}

    def clear_regions(self) -> None:
        """Back to "off": every row takes segment 0 alone, the bits of a wrapper compiled without `regions` on the first prompt."""
        from . import regions
        regions.state_of(self.compiled, "clear_regions").clear()
        self._regions = None
        self._regions_applied = {}

    def _apply_regions(self, sample: torch.Tensor) -> None:
        """Bind the buffers of this call's batch and latent size and, when masks are set, write them for this geometry.  Buffers
        are found by (rows, queries), so two latent shapes with the same row count can share one (128 x 64 and 64 x 128): the
        weights are written again whenever the geometry of a row count changes, and masks of another size than the call's
        latent raise.  Without masks nothing is written: new buffers are "off", and another owner's setting is left alone."""
        from . import regions
        state = compiled_state(self.compiled, "regions", regions.Regions)
        if state is None or torch.cuda.is_current_stream_capturing():
            return
        rows, hw = int(sample.shape[0]), (int(sample.shape[-2]), int(sample.shape[-1]))
        state.bind(rows, hw, sample.device)
        if self._regions is None or self._regions_applied.get(rows) == hw:
            return
        masks, chunks = self._regions
        if tuple(masks.shape[-2:]) != hw:
            raise ValueError(f"set_regions: the masks are {tuple(masks.shape[-2:])}, this call's latent is {hw}: masks are given at "
                             "latent resolution")
        state.set(masks, regions.positive_rows(rows, chunks), rows)
        self._regions_applied[rows] = hw

    # ---- IP-Adapter image prompts (ip_adapter.py): buffers the cross-attention sites read by address; the captured graphs stay ----
    def _ip(self, what: str):
        from . import ip_adapter
        return ip_adapter.state_of(self.compiled, what)

    def load_ip_adapter(self, state_dict, slot: int = 0):
        """Copy an IP-Adapter checkpoint's to_k_ip / to_v_ip weights into adapter slot `slot` (ip_adapter.IPAdapter.load); returns
        its image_proj sub-dict.  An image set earlier is projected again with the new weights at the next call.
        `added_cond_kwargs["image_embeds"]` is NOT read by the wrappers: project the embeddings once
        (ip_adapter.project_image_embeds, or a Resampler of the caller's) and pass the tokens to `set_ip_adapter_image`.  Raises on a
        wrapper compiled without `ip_adapter=N`."""
        proj = self._ip("load_ip_adapter").load(state_dict, slot)
        self._ip_applied = {}
        return proj

    def set_ip_adapter_image(self, tokens: torch.Tensor, negative_tokens: Optional[torch.Tensor] = None, slot: int = 0,
                             chunks: int = 2) -> None:
        """Image tokens (batch or 1, N, cross_dim) of slot `slot` for every following call.  `chunks` says how a call's batch
        divides, as in `set_regions`: 2 = [uncond | cond], 3 = [uncond | cond | cond (perturbed)] - the first block is the negative
        one and takes `negative_tokens` (default: zero tokens = no contribution), the others take `tokens`; 1 = every row takes
        `tokens`.  The K/V buffers of a batch size are allocated at the first call that has it and written in place."""
        from . import regions
        st = self._ip("set_ip_adapter_image")
        slot = st._slot(slot, "set_ip_adapter_image")
        regions.positive_rows(chunks, chunks)                    # (validates chunks)
        for t, what in ((tokens, "tokens"), (negative_tokens, "negative_tokens")):
            if t is not None and (torch.as_tensor(t).dim() != 3 or torch.as_tensor(t).shape[1] != st.tokens[slot]):
                raise ValueError(f"set_ip_adapter_image: {what} must be (batch or 1, N, cross_dim) with N = {st.tokens[slot]} tokens for slot "
                                 f"{slot} (compiled with ip_adapter={st.tokens}), got {tuple(torch.as_tensor(t).shape)}")
        if chunks == 1 and negative_tokens is not None:
            raise ValueError("set_ip_adapter_image: negative_tokens need a negative row block (chunks 2 or 3)")
        self._ip_images[slot] = (tokens, negative_tokens, chunks)
        self._ip_applied = {}

    def set_ip_adapter_scale(self, scale, slot: int = 0) -> None:
        """A float for every site, or a mapping {regular expression on the site paths: float} (first match wins, "mid" selects the
        middle block, unmatched sites get 0); 0 switches a site's image attention off at no cost.  Written at once, in place."""
        self._ip("set_ip_adapter_scale").set_scale(scale, slot)

    def set_ip_adapter_masks(self, masks: Optional[torch.Tensor], slot: int = 0) -> None:
        """Where slot `slot`'s image prompt applies: (lh, lw) or (batch, lh, lw) at latent resolution, written to every row of the
        following calls; None = everywhere.  A call whose latent is not the masks' size raises."""
        from . import ip_adapter
        st = self._ip("set_ip_adapter_masks")
        slot = st._slot(slot, "set_ip_adapter_masks")
        if masks is not None:
            ip_adapter.mask_level_weights(masks, 0)               # (validates the masks now, not at the next call)
        self._ip_masks[slot] = masks
        self._ip_applied = {}

    def unload_ip_adapter(self, slot: int = 0) -> None:
        """Slot `slot` back to "off": scale 0, weights and image K/V zero, masks 1 - the bits of the wrapper before the adapter."""
        st = self._ip("unload_ip_adapter")
        st.unload(slot)
        self._ip_images.pop(slot, None)
        self._ip_masks.pop(slot, None)

    def _apply_ip_adapter(self, sample: torch.Tensor) -> None:
        """Bind the buffers of this call's batch and latent size and write what was set for this geometry (as _apply_regions)."""
        from . import ip_adapter
        state = compiled_state(self.compiled, "ip_adapter", ip_adapter.IPAdapter)
        if state is None or torch.cuda.is_current_stream_capturing():
            return
        rows, hw = int(sample.shape[0]), (int(sample.shape[-2]), int(sample.shape[-1]))
        state.bind(rows, hw, sample.device)
        if self._ip_applied.get(rows) == hw:
            return
        for slot, (tokens, negative, chunks) in self._ip_images.items():
            state.set_image(tokens, negative, slot, rows, chunks)
        for slot, masks in self._ip_masks.items():
            if masks is not None and tuple(torch.as_tensor(masks).shape[-2:]) != hw:
                raise ValueError(f"set_ip_adapter_masks: the masks are {tuple(torch.as_tensor(masks).shape[-2:])}, this call's latent is {hw}: "
                                 "masks are given at latent resolution")
            state.set_masks(masks, slot, rows)
        self._ip_applied[rows] = hw

    # ---- T2I-Adapter / ControlNet residuals (t2i_adapter.py, controlnet.py): static buffers the residual sites read by address;
    # the captured graphs stay.  A compiled module carries at most one of the two states -------------------------------------------
    def _t2i_state(self):
        from . import t2i_adapter
        return compiled_state(self.compiled, "t2i_adapter", t2i_adapter.T2IAdapterState)

    def _cn_state(self):
        from . import controlnet
        return compiled_state(self.compiled, "controlnet", controlnet.ControlNetState)

    def _apply_residuals(self, sample: torch.Tensor, state, values, what: str) -> None:
        """Bind `state`'s buffers of this call's batch and latent size (outside any capture) and write this call's residuals: one
        tensor per site (None: zeros there), already scaled by the caller (and summed over several adapters / a MultiControlNet), so
        the scale is 1; `values` None: scale 0, nothing else is touched.  The very tensors of the previous call at their versions are
        not copied again: the wrapper HOLDS those tensors until the next call with others (identity is only safe while the objects
        live; at 1024 x 1024, bf16, two rows that is about 26 MB kept alive for a T2I adapter), and the rule looks at the caller's
        tensors alone - somebody who writes the shared buffers through `gm.t2i_adapter.set` / `gm.controlnet.set` in between, and
        then calls with the same tensor objects, is not noticed."""
        if state is None:
            return
        rows, hw = int(sample.shape[0]), (int(sample.shape[-2]), int(sample.shape[-1]))
        if not torch.cuda.is_current_stream_capturing():
            state.bind(rows, hw, sample.device, dtype=self.compute_dtype)
        if values is None:
            if state.host_scale != 0.0:
                state.clear()
            return
        if len(values) != len(state.sites):
            raise ValueError(f"{what}: {len(state.sites)} tensors expected, one per site {state.sites}, got {len(values)}")
        versions = tuple(None if v is None else v._version for v in values)
        last = self._residuals_last
        same = (last is not None and last[0] is state and last[1] == rows and last[3] == versions and len(last[2]) == len(values)
                and all(a is b for a, b in zip(last[2], values)))
        if not same:
            shapes = state.site_shapes(hw)
            full = [torch.zeros((1,) + shapes[k], dtype=self.compute_dtype, device=sample.device) if v is None else v
                    for k, v in enumerate(values)]
            state.set(full, None, rows)
            self._residuals_last = (state, rows, list(values), versions)
        if state.host_scale != 1.0:
            state.set_scale(1.0)

    def _context_for(self, ehs: torch.Tensor) -> tuple:
        """Static K/V context buffers for this prompt.  Fast path: the very tensor object the cache was built from, at the
        version it had then.  A different object of the same shape (ComfyUI re-concatenates cond | uncond on every call) is
        compared BY CONTENT with the kept copy (one device compare + host sync, ~1 % of a step) and adopted when equal;
        anything else re-projects the context (one pass of 140 small GEMMs).  Under a stream capture of the caller's own
        the compare (a host sync) is skipped and the call counts as a new prompt."""
        shape = tuple(ehs.shape)
        if ehs is self._ctx_src.get(shape) and ehs._version == self._ctx_version.get(shape) and shape in self._ctx:
            return self._ctx[shape]
        copy = self._ctx_copy.get(shape)
        same = (copy is not None and shape in self._ctx and copy.dtype == ehs.dtype and copy.device == ehs.device
                and not torch.cuda.is_current_stream_capturing() and torch.equal(ehs, copy))
        if not same:
            self.compiled.exec_context.refresh_derived(full=True)
            with torch.no_grad():
                new = self.compiled.precompute_context(ehs.to(self.compute_dtype))
            old = self._ctx.get(shape)
            if old is None:
                self._ctx[shape] = tuple(t.clone() for t in new)
            else:
                for dst, src in zip(old, new):
                    dst.copy_(src)
            self._ctx_copy[shape] = ehs.detach().clone()
            self._new_prompt = True
        self._ctx_src[shape], self._ctx_version[shape] = ehs, ehs._version      # held: its address cannot be recycled under the cache
        return self._ctx[shape]

    def _step_fn(self, shape: tuple):
        fn = self._steps.get(shape)
        if fn is None:
            ctx = self._ctx[shape]                 # closed over: the graph reads these buffers in place

            def step(sample, timesteps, cond, chunks=0):      # (a plain integer: part of the graph cache's key)
                with self._perturbed_scope(chunks, tuple(sample.shape[-2:])):
                    return self.compiled.forward_with_context(sample, timesteps, ctx, cond)[0]

            fn = make_dynamic_graphed_callable(step) if self.cuda_graph else step
            self._steps[shape] = fn
        return fn

    def _fp8_restart(self, x, timesteps, shape, cond) -> None:
        """fp8 plan: the delayed activation scales restart from the first evaluation of every TRAJECTORY, as `DenoiseLoop` does
        (the hooks only restarted them when the prompt changed, so a new seed under the same prompt quantised its
        first step with the scales of the previous trajectory's last one).  A trajectory start is a new prompt or a timestep
        that is larger than the last call's (within a trajectory the timesteps fall); reading the timestep costs one host
        sync per call, paid only in this mode.  Under a stream capture of the caller's own nothing can be measured: a captured
        call replays whatever scales the last eager call left - evaluate the trajectory's first step eagerly before capturing."""
        if torch.cuda.is_current_stream_capturing():
            return
        t = float(timesteps.max())
        start = self._new_prompt or self._last_t is None or t > self._last_t
        self._last_t = t
        if start:
            from .optimization import recalibrate_fp8
            ctx = self._ctx[shape]
            def run_once():
                with self._perturbed_scope(self._perturbed_chunks, tuple(x.shape[-2:])):
                    return self.compiled.forward_with_context(x, timesteps, ctx, cond)

            ectx = getattr(self.compiled, "exec_context", None)
            if ectx is not None and ectx.fp8 is None:
                with torch.no_grad():
                    run_once()          # the very first evaluation creates the scale slots; after it this trajectory starts like every later one
            recalibrate_fp8(self.compiled, run_once)

    def _run(self, sample, timesteps, ehs, cond, t2i=None, controlnet=None):
        # (.to() is the identity when the caller already computes in this dtype: an fp16 pipeline over an fp16 module)
        io_dtype = sample.dtype
        dev = sample.device
        self._apply_regions(sample)
        self._apply_ip_adapter(sample)
        self._apply_seg(sample)
        self._apply_reference(sample)
        self._apply_residuals(sample, self._t2i_state(), t2i, "T2I-Adapter residuals")
        self._apply_residuals(sample, self._cn_state(), controlnet, "ControlNet residuals")
        self._context_for(ehs)
        if not torch.is_tensor(timesteps):
            timesteps = torch.tensor(float(timesteps), dtype=torch.float32)
        timesteps = timesteps.to(device=dev, dtype=torch.float32)
        if timesteps.dim() > 1 or (timesteps.dim() == 1 and timesteps.numel() not in (1, sample.shape[0])):
            raise ValueError(f"timesteps of shape {tuple(timesteps.shape)} do not match batch {sample.shape[0]}")
        x = sample.to(self.compute_dtype)
        if getattr(self.compiled, "fp8_plan", False):
            self._fp8_restart(x, timesteps, tuple(ehs.shape), cond)
        self._new_prompt = False
        with torch.no_grad():
            extra = (self._perturbed_chunks,) if self._perturbed_chunks else ()      # (0 keeps the cache entry of a call without it)
            out = self._step_fn(tuple(ehs.shape))(x, timesteps, cond, *extra)
        return out.to(io_dtype)


class DiffusersUNet(_HoistedUNet):
    """`pipe.unet` replacement (duck-typed `UNet2DConditionModel.forward` of diffusers 0.21.2)."""

    def __init__(self, compiled, spec: UNetSpec = SDXL_BASE, compute_dtype: torch.dtype = torch.bfloat16, cuda_graph: bool = True):
        super().__init__(compiled, compute_dtype, cuda_graph)
        self.config = make_config(spec)            # what the pipeline reads (load_sdxl_pipeline.py:29-34)

    @property
    def dtype(self):
        return self.compute_dtype

    def forward(self, sample, timestep, encoder_hidden_states=None, class_labels=None, timestep_cond=None,
                attention_mask=None, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict: bool = False,
                down_block_additional_residuals=None, mid_block_additional_residual=None, down_intrablock_additional_residuals=None,
                **ignored):
        if encoder_hidden_states is None or added_cond_kwargs is None:
            raise ValueError("the SDXL UNet needs encoder_hidden_states and added_cond_kwargs{text_embeds, time_ids}")
        for name, val in (("class_labels", class_labels), ("timestep_cond", timestep_cond), ("attention_mask", attention_mask)):
            if val is not None:
                raise NotImplementedError(f"{name} is not part of the SDXL-base UNet path")
        loras = self.compiled.__dict__.get("_lora_set")
        if loras is not None and loras.names():
            # adapters loaded through load_lora: {"scale": s} is diffusers' global multiplier over all of them (1 when the
            # pipeline passes none); a new value merges again, the same value costs nothing
            kw = dict(cross_attention_kwargs or {})
            scale = float(kw.pop("scale", 1.0))
            if kw:
                raise NotImplementedError(f"cross_attention_kwargs {sorted(kw)} (attention processors) are not supported")
            if loras.set_global_scale(scale):
                self.refresh_weights()
        elif cross_attention_kwargs:
            # a pipeline with merged LoRA weights still passes {"scale": s}: scale 1 changes nothing once the weights are merged;
            # anything else would need attention processors the compiled graph has not
            extra = {k: v for k, v in cross_attention_kwargs.items() if not (k == "scale" and float(v) == 1.0)}
            if extra:
                raise NotImplementedError(f"cross_attention_kwargs {sorted(extra)} (attention processors / a LoRA scale other than 1) are not "
                                          "supported: load the adapter with load_lora(name, state_dict, scale) and the scale is honoured")
        t2i = None
        if self._t2i_state() is not None:
            # compiled with t2i_adapter=True: the T2I-Adapter pipeline's residuals (already scaled by adapter_conditioning_scale) are
            # honoured, ControlNet's are refused; a wrapper compiled without the flag ignores all three, as it always has
            if down_block_additional_residuals is not None or mid_block_additional_residual is not None:
                raise NotImplementedError("down_block_additional_residuals / mid_block_additional_residual (ControlNet) are not supported "
                                          "by the compiled UNet: only down_intrablock_additional_residuals (T2I-Adapter) are")
            if down_intrablock_additional_residuals is not None:
                t2i = list(down_intrablock_additional_residuals)
        cn = None
        cn_state = self._cn_state()
        if cn_state is not None:
            # compiled with controlnet=True: the ControlNet pipeline's residuals (already scaled by controlnet_conditioning_scale and
            # summed over a MultiControlNet) are honoured, the T2I-Adapter's are refused
            if down_intrablock_additional_residuals is not None:
                raise NotImplementedError("down_intrablock_additional_residuals (T2I-Adapter) are not supported by a UNet compiled with "
                                          "controlnet=True: only down_block_additional_residuals / mid_block_additional_residual are")
            if down_block_additional_residuals is not None or mid_block_additional_residual is not None:
                down = list(down_block_additional_residuals) if down_block_additional_residuals is not None else [None] * (len(cn_state.sites) - 1)
                cn = down + [mid_block_additional_residual]
        cd = self.compute_dtype
        cond = {"text_embeds": added_cond_kwargs["text_embeds"].to(cd), "time_ids": added_cond_kwargs["time_ids"].to(cd)}
        out = self._run(sample, timestep, encoder_hidden_states, cond, t2i, cn)
        if return_dict:
            from types import SimpleNamespace
            return SimpleNamespace(sample=out)
        return [out]                                # the pipeline takes [0] (reference unet_pt.py:542 returns a list)


def compile_unet_from_state_dict(state_dict, spec: UNetSpec = SDXL_BASE, dtype=None, device="cuda",
                                 cuda_graph: bool = True, freeu: bool = False, pag_layers=None, regions=None,
                                 region_tokens: int = 77, ip_adapter=None, seg_layers=None, t2i_adapter: bool = False,
                                 controlnet: bool = False, reference_layers=None) -> DiffusersUNet:
    """Build the UNet, load a Diffusers-keyed state_dict (any float dtype), compile, wrap for the pipeline.
    `dtype` None = the state_dict's own dtype (fp16 for the reference's `variant="fp16"` checkpoint).
    `freeu=True` compiles the FreeU sites in: `enable_freeu(s1, s2, b1, b2)` / `disable_freeu()` then work as on diffusers' UNet.
    `pag_layers=("mid",)` compiles the perturbed-attention sites in (diffusers' `pag_applied_layers`): `enable_pag(chunks)` /
    `disable_pag()` then say which rows of a call are the perturbed ones.
    `seg_layers=("mid",)` compiles the smoothed-energy sites in (seg.py; not with `pag_layers`): `enable_seg(chunks, sigma)` /
    `set_seg_sigma(sigma)` / `disable_seg()` drive them.
    `regions=R` compiles regional cross-attention in (regions.py): the pipeline passes R prompts of `region_tokens` tokens
    concatenated along the token axis as `encoder_hidden_states`; `set_regions(masks, chunks)` / `clear_regions()` drive it.
    `ip_adapter=N` (or a tuple of token counts, one per adapter) compiles IP-Adapter image attention in (ip_adapter.py):
    `load_ip_adapter`, `set_ip_adapter_image`, `set_ip_adapter_scale`, `set_ip_adapter_masks`, `unload_ip_adapter` drive it;
    `added_cond_kwargs["image_embeds"]` is not read.
    `t2i_adapter=True` compiles the T2I-Adapter residual sites in (t2i_adapter.py): `down_intrablock_additional_residuals` of a call
    are then added at the sites (None: off, at no cost), ControlNet's residual arguments raise.
    `controlnet=True` compiles the ControlNet sites in (controlnet.py; not with `t2i_adapter`): `down_block_additional_residuals` and
    `mid_block_additional_residual` of a call are then added for the decoder (None: off), the T2I-Adapter's argument raises.
    `reference_layers=(".*",)` compiles the reference-only sites in (reference.py; not with `pag_layers` / `seg_layers`):
    `enable_reference(chunks)` / `disable_reference()` then say which rows of a call are the reference rows."""
    if dtype is None:
        dtype = next(iter(state_dict.values())).dtype
    with torch.device("meta"):
        model = UNet2DConditionModel(spec)
    model = model.to_empty(device=device).to(dtype)
    model.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in state_dict.items()})
    compiled = optimize_model(model, cuda_graph=False, freeu=freeu, pag_layers=pag_layers, regions=regions, region_tokens=region_tokens,
                              ip_adapter=ip_adapter, seg_layers=seg_layers, t2i_adapter=t2i_adapter, controlnet=controlnet,
                              reference_layers=reference_layers)
    return DiffusersUNet(compiled, spec, dtype, cuda_graph)


def attach_to_diffusers(pipe, spec: UNetSpec = SDXL_BASE, dtype=None, cuda_graph: bool = True, freeu: bool = False, pag_layers=None,
                        regions=None, region_tokens: int = 77, ip_adapter=None, seg_layers=None, t2i_adapter: bool = False,
                        controlnet: bool = False, reference_layers=None):
    """`pipe.unet = compiled UNet` (same weights; the counterpart of load_sdxl_pipeline.py:24-35), returns the pipeline.
    `dtype` None = the pipeline's own UNet dtype (fp16 at the reference call site): no casts at the boundary."""
    device = next(pipe.unet.parameters()).device
    pipe.unet = compile_unet_from_state_dict(pipe.unet.state_dict(), spec, dtype, device, cuda_graph, freeu=freeu, pag_layers=pag_layers,
                                             regions=regions, region_tokens=region_tokens, ip_adapter=ip_adapter, seg_layers=seg_layers,
                                             t2i_adapter=t2i_adapter, controlnet=controlnet, reference_layers=reference_layers)
    return pipe


class ComfyUNet(_HoistedUNet):
    """`diffusion_model` replacement with ComfyUI's calling convention."""

    def forward(self, x, timesteps=None, context=None, y=None, control=None, transformer_options: Optional[dict] = None, **kwargs):
        if timesteps is None or context is None or y is None:
            raise ValueError("ComfyUNet needs timesteps, context (text states) and y (pooled text | size/crop features)")
        t2i = cn = None
        if control is not None and self._cn_state() is not None:
            from . import controlnet
            cn = controlnet.comfy_residuals(self._cn_state(), control)      # a ControlNet's output / middle entries; anything else raises
        elif control is not None:
            state = self._t2i_state()
            if state is None:
                raise NotImplementedError("ControlNet residuals (`control`) are not supported by the compiled UNet")
            from . import t2i_adapter
            t2i = t2i_adapter.comfy_features(state, control)      # a T2I adapter's input / middle entries; anything else raises
        patches = (transformer_options or {}).get("patches") or (transformer_options or {}).get("patches_replace")
        if patches:
            raise NotImplementedError("transformer_options patches are not supported by the compiled UNet")
        if y.shape[0] != x.shape[0] or context.shape[0] != x.shape[0]:
            raise ValueError("x, context and y must share the batch dimension")
        return self._run(x, timesteps, context, y.to(self.compute_dtype), t2i, cn)


def compile_comfy_unet(unet: UNet2DConditionModel, cuda_graph: bool = True, freeu: bool = False, pag_layers=None, regions=None,
                       region_tokens: int = 77, ip_adapter=None, seg_layers=None, t2i_adapter: bool = False,
                       controlnet: bool = False, reference_layers=None) -> ComfyUNet:
    """Compile the `y`-vector entry of a UNet (weights shared with `unet`).  `freeu=True`: with FreeU sites, driven by
    `enable_freeu(s1, s2, b1, b2, version=2)` (the FreeU_V2 node) or version 1 (the FreeU node).  `pag_layers=("mid",)`: with
    perturbed-attention sites; the PerturbedAttentionGuidance node's extra, fully perturbed call is `enable_pag(1)`.  `regions=R`:
    with regional cross-attention (conditioning masks / "attention couple"): `context` is the R conditionings concatenated along
    the token axis, `set_regions(masks, chunks)` / `clear_regions()` drive it.  `ip_adapter=N`: with IP-Adapter image attention
    (the IPAdapter nodes), driven by `load_ip_adapter` / `set_ip_adapter_image` / `set_ip_adapter_scale` / `set_ip_adapter_masks` /
    `unload_ip_adapter`.  `seg_layers=("mid",)`: with smoothed-energy sites (the SEG node); its extra, fully perturbed call is
    `enable_seg(1, sigma)`.  `t2i_adapter=True`: with T2I-Adapter residual sites: `control={"input": [...], "middle": [...]}` of a call
    is consumed the way ComfyUI's apply_control does (from the end of each list, None entries skipped) and must land on the sites.
    `controlnet=True`: with ControlNet sites (not with `t2i_adapter`): `control={"output": [...], "middle": [...]}` of a call, entry i of
    `output` being skip i in encoder order (ComfyUI pops from the end while the decoder consumes its skips last-first); a non-empty
    `"input"` raises.  `reference_layers=(".*",)`: with reference-only sites (the ReferenceOnlySimple node's batch of
    [generated | reference] latents is `enable_reference(2)`)."""
    dtype = next(unet.parameters()).dtype
    compiled = optimize_model(UNetWithLabelVector(unet), cuda_graph=False, freeu=freeu, pag_layers=pag_layers, regions=regions,
                              region_tokens=region_tokens, ip_adapter=ip_adapter, seg_layers=seg_layers, t2i_adapter=t2i_adapter,
                              controlnet=controlnet, reference_layers=reference_layers)
    return ComfyUNet(compiled, dtype, cuda_graph)


def patch_comfy_model(model_patcher, unet: UNet2DConditionModel, cuda_graph: bool = True, freeu: bool = False, pag_layers=None,
                      regions=None, region_tokens: int = 77, ip_adapter=None, seg_layers=None, t2i_adapter: bool = False,
                      controlnet: bool = False, reference_layers=None) -> ComfyUNet:
    """Replace `model_patcher.model.diffusion_model` (duck-typed ComfyUI ModelPatcher) with the compiled UNet."""
    adapter = compile_comfy_unet(unet, cuda_graph, freeu=freeu, pag_layers=pag_layers, regions=regions, region_tokens=region_tokens,
                                 ip_adapter=ip_adapter, seg_layers=seg_layers, t2i_adapter=t2i_adapter, controlnet=controlnet,
                                 reference_layers=reference_layers)
    model_patcher.model.diffusion_model = adapter
    return adapter
