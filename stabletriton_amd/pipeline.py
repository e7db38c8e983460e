"""The 50-step denoise loop on the device, captured as a hipGraph.

The reference captures ONE UNet forward per graph and leaves the loop to the
Diffusers pipeline (optimizers/cuda/graphs.py:100-110,
implementations/Diffusers/load_sdxl_pipeline.py:39-46).  BASELINE.json's
north_star asks for the whole loop as a hipGraph: here every step is
[UNet forward -> Euler update of the fp32 latent -> scaled bf16 input of the next
step], all on the device, so the 50 steps can be captured back to back and a
run is one graph launch.  `mode="step"` captures a single step driven by a
device-side step counter instead (replayed n times), `mode="eager"` captures
nothing (used for per-kernel timing and debugging).

With `guidance_scale` the loop runs classifier-free guidance the way the reference's Diffusers call site does
(diffusers' StableDiffusionXLPipeline: UNet batch 2B = [negative | positive] conditioning, one latent per image):
the UNet input, text context and time tables get 2B rows, and the Euler update is `st_cfg_euler_step`, which
combines the two halves, optionally applies guidance rescale, and writes both halves of the next input.  The
guidance (and rescale) values live in device tables of n_steps floats: `set_guidance` changes them without a
new capture.

With `DPMSolverTables` (scheduler.dpmpp_2m_tables) the update is DPM-Solver++(2M), `st_dpmpp2m_step`, guided or not.  The
solver carries the previous step's prediction of the clean latent in a static fp32 `history` buffer, and a device int
`start` marks the step a trajectory starts from (0 after set_noise, t_start after set_image): that step is first-order and
does not read the history.  Both, with the coefficient table, are read by address from the captured graph.  The solver
follows from the type of the tables; Euler tables keep the Euler update and its buffers.

With `SDETables` (scheduler.euler_ancestral_tables, dpmpp_2m_sde_tables) the update is `st_sde_step`: the DPM++ row plus
fresh Gaussian noise on every step, drawn inside the kernel from a counter-based generator (rng.py) keyed by a device
table of B 64-bit seeds and the step's schedule index.  Nothing is advanced between steps, so modes loop, step and eager
draw the same noise and every replay repeats its bits.  `set_seed` writes the seeds in place (no new capture).  A seed
also starts any sampler without a host tensor: `denoise(seed=s)` takes the initial noise from the same generator
(counter word 0).  Euler and DPM++ loops allocate the seed table only when a seed is used, and their graph never reads it.

LoRA adapters (`load_lora`, `set_lora_scale`, `unload_lora`; lora.py) are merged into the UNet's Linear (with `convs=True` also Conv2d) weights in place by
one grouped kernel launch.  The weights keep their addresses, so the captured graph stays; the loop re-derives, in place,
what it had computed from them: derived weights, the hoisted text-context K/V and the time tables.

FreeU (`set_freeu`; freeu.py) is a device row of five floats the sites of a UNet compiled with `freeu=True` read by
address: setting or clearing it is an in-place write, the captured graph stays.

Perturbed-attention guidance (`pag_scale`, `set_pag`; pag.py) adds one more block of UNet rows, [negative | positive | perturbed]
(3B) or, without `guidance_scale`, [positive | perturbed] (2B): the perturbed rows carry the positive conditioning and the same
latent, and the self-attention sites of a UNet compiled with `pag_layers` return v for them (one copy launch per site instead of
the attention).  The update is the `st_pag_*` form of the loop's sampler, which adds pag[i] (e_pos - e_pert) before the rescale; the
scale is one more device table of n_steps floats, so `set_pag` needs no new capture.

Smoothed energy guidance (`seg_scale`, `seg_sigma`, `set_seg`; seg.py) is the same row layout, scale table and `st_pag_*` update
with another perturbation: the self-attention sites of a UNet compiled with `seg_layers` blur the perturbed rows' queries over the
latent grid (two more launches per site than plain attention: the blur and the tail's own attention launch).  sigma lives in device
parameter rows the blur reads by address, so `set_seg(scale, sigma)` needs no new capture, finite <-> infinity included.  Not
together with `pag_scale`.

Regional prompts (`set_regions`; regions.py) on a UNet compiled with `regions=R`: the loop is built with `tokens = R * region_tokens`,
the positive text state is the R prompts concatenated along the token axis, and every cross-attention combines the R per-prompt
results per latent cell with weights derived from `set_regions(masks)`.  The weights are device buffers the sites read by address:
setting or clearing them is an in-place write, before or after `capture()`.  Until `set_regions` the loop computes what a UNet
compiled without `regions` computes on the first prompt.

IP-Adapter image prompts (`load_ip_adapter`, `set_ip_adapter_image`, `set_ip_adapter_scale`, `set_ip_adapter_masks`,
`unload_ip_adapter`; ip_adapter.py) on a UNet compiled with `ip_adapter=N`: every cross-attention adds a decoupled attention over the
image tokens of each adapter slot, in the same launch, under per-site scales in a device table.  Adapter weights, image K/V, scales
and masks are device buffers the sites read by address: every one of the five calls is an in-place write, before or after
`capture()`.  A slot at scale 0 - the state until `set_ip_adapter_scale` - is skipped by the kernel: the bits of a UNet compiled
without `ip_adapter`.

T2I-Adapter structural control (`set_t2i_adapter`, `set_t2i_adapter_scale`; t2i_adapter.py) on a UNet compiled with
`t2i_adapter=True`: four feature maps per control image, written once into static buffers, are added at the UNet's residual sites
under a per-step scale table (`scale` for the first int(n_steps * factor) steps, 0 after).  The sites read the table at
`step_ids[i:i+1]` (modes loop / eager) or at the step counter (mode step); a step at scale 0 - every step until `set_t2i_adapter` -
writes nothing: the bits of a UNet compiled without sites.

ControlNet (`controlnet=`, `set_controlnet`, `set_controlnet_scale`; controlnet.py) on a UNet compiled with `controlnet=True`:
`controlnet=` is the compiled branch (`optimize_model(ControlNetXL(...), cuda_graph=False)`).  Every step calls the branch on the
UNet's own `x_in`, timestep and conditioning rows plus the control image's embedding (a static buffer of `rows` rows), then the UNet
with the branch's outputs lent to its sites (`state.using(step, table, residuals=...)`: no copies, the capture records their
addresses) under a per-step scale table that is 0 outside [int(n * start), int(n * end)).  Nothing of this is captured by value:
`set_controlnet` / `set_controlnet_scale` are in-place writes before or after `capture()`.  The captured graph is static, so a
step at scale 0 still runs the branch; only the sites' launch leaves early, and the UNet gives the bits of one compiled without
sites.  Not built: several branches in one loop, guess mode's cond-only rows, the branch's own context / time split (its plain
forward runs).

Tiled denoising (`tile_hw`, `tile_stride`, `tile_wrap_w`, `tile_weights`, `set_tile_weights`; tiles.py) makes `latent_hw` a canvas
larger than the UNet denoises in one piece (MultiDiffusion; with Gaussian weights Mixture of Diffusers): the UNet runs on the T
overlapping windows of the canvas as batch rows - `x_in`, the conditioning buffers, the hoisted context and the time tables have
B * blocks * T rows, row (blk * B + b) * T + t - while `latent`, `history`, the seeds' noise, the canvas noise prediction and a
canvas-sized `x_step` keep the canvas shape.  One step is UNet on the windows -> `st_tile_blend` (per canvas pixel the weighted mean of
the covering windows' predictions) -> the loop's own update kernel, unchanged, on the canvas -> `st_tile_gather` (the next input cut
into windows): two more launches per step, every sampler and guidance form as before.  Guidance rescale therefore takes its statistics
over the canvas, not per window.  The weight map is a device buffer the blend reads by address: `set_tile_weights` is an in-place write,
before or after `capture()`.  `set_conditioning` takes B rows (one prompt for all of a sample's windows) or B * T rows (one prompt per
window, sample-major).  PAG and SEG work (their row block is outermost; the perturbed scope and SEG's blur see the window size).  UNets
compiled with `regions`, `ip_adapter`, `t2i_adapter` or `controlnet` are refused: their states bind per latent size and row count, and cropping them
per window is not built.  The fp8 plan is allowed with tiles and not covered by tests.  `tile_hw=None` is the untiled loop exactly:
`x_step is x_in`, no further buffers or launches.

Masked inpainting (`inpaint=True`, `set_inpaint`; inpaint.py) keeps part of an image fixed: behind every sampler update one more launch,
`st_inpaint_blend`, puts the pixels to keep back to init + sigma[i + 1] * noise (the trajectory's own start noise, which `set_noise` and
`set_image` also copy into a static buffer) on the fp32 latent and rewrites the next input of every row block; a pixel to repaint is
not written.  The blend is behind the step, so every sampler, CFG, rescale, PAG and SEG, LoRA and FreeU are as before, the DPM history
is left alone, and a tiled loop blends on the canvas, ahead of `st_tile_gather`.  Init latent, mask and the differential mode's threshold
table are device buffers read by address: `set_inpaint` is an in-place write, before or after `capture()`; binary / soft and threshold
mode share the captured launch (a NaN threshold entry = no threshold).  Mask all ones - the state until `set_inpaint`, and after
`set_inpaint(None)` - writes nothing: the bits of a loop built without the flag, at one early-exit launch per step.  `inpaint=False` is
the present loop exactly: no buffers, no launch.  Not built: nine-channel inpainting checkpoints, mask resampling.

Reference-only control (`reference=True`, `set_reference`; reference.py) on a UNet compiled with `reference_layers`: the UNet evaluates
one more block of batch rows, [negative | positive | reference] or [positive | reference], the noised reference latent under the
positive conditioning, and in the selected self-attention sites every other row attends to its own tokens and to its reference
row's tokens under one softmax (one launch per site, csrc/attention_joint.hip).  The sampler update sees the leading row blocks of
the prediction and of the next input as views and is unchanged; behind it (and behind the inpaint blend) one launch of the existing
`st_inpaint_blend` with an all-zero mask writes the reference block's next input, (init + sigma[i + 1] * noise) * in_scale[i + 1].
The sites read a per-step device table (1 inside [start * n, end * n), 0 = ordinary attention, the reference rows' keys are never
read) at the step counter: `set_reference` / `set_reference(None)` are in-place writes, before or after `capture()`.  The captured graph
is static, so a loop gated off still evaluates the reference rows.  Not with `pag_scale`, `seg_scale`, `tile_hw`, or UNets compiled with
`regions`, `ip_adapter`, `t2i_adapter`, `controlnet`.  Parity with A1111, ComfyUI and diffusers is unpinned; `style_fidelity`, a continuous
strength and the AdaIN variant are out of scope.
"""
from __future__ import annotations

import contextlib
import numbers
from typing import Callable, Dict, Optional, Sequence, Union

import torch

from . import ops, seg
from .optimizers.graphs import no_gc_during_capture
from .scheduler import DPMSolverTables, EulerTables, SDETables, euler_discrete_tables
from .state import compiled_state


REFERENCE_COUNTER_WORD = (1 << 32) - 1      # rng.py's counter word of set_reference(seed=): behind every start (0) and step (i + 1) word


class DenoiseLoop:
    def __init__(self, unet: Callable, batch: int, latent_hw, dtype: torch.dtype, device,
                 tables: Optional[Union[EulerTables, DPMSolverTables, SDETables]] = None, cross_dim: int = 2048, pooled_dim: int = 1280,
                 tokens: int = 77, mode: str = "loop", n_time_ids: int = 6,
                 guidance_scale: Optional[Union[float, Sequence[float]]] = None,
                 guidance_rescale: Optional[Union[float, Sequence[float]]] = None,
                 pag_scale: Optional[Union[float, Sequence[float]]] = None,
                 seg_scale: Optional[Union[float, Sequence[float]]] = None, seg_sigma: float = float("inf"),
                 tile_hw=None, tile_stride=None, tile_wrap_w: bool = False, tile_weights="uniform", controlnet: Optional[Callable] = None,
                 inpaint: bool = False, reference: bool = False):
        assert mode in ("loop", "step", "eager")
        if seg_scale is not None and pag_scale is not None:
            raise ValueError("seg_scale cannot be combined with pag_scale: both claim the perturbed row block of the UNet batch")
        if guidance_rescale is not None and guidance_scale is None:
            raise ValueError("guidance_rescale needs guidance_scale")
        from . import controlnet as _cn, ip_adapter as _ip, pag, regions as _regions, t2i_adapter as _t2i
        if controlnet is not None:                         # the branch's residuals need the UNet's sites
            _cn.state_of(unet, "DenoiseLoop(controlnet=...)")
        # perturbed-attention guidance: the UNet's sites must exist (compiled in), and the loop names the perturbed row block
        # around its own UNet calls only (chunks 3 = [neg | pos | pert], 2 = [pos | pert])
        self._perturbed = None
        if pag_scale is not None:
            self._perturbed = pag.state_of(unet, "DenoiseLoop(pag_scale=...)")
        # smoothed energy guidance: the same perturbed row block under another perturbation (blurred queries); everything below
        # that speaks of `pag_scale` - rows, conditioning, the scale table, the update launches - serves both
        if seg_scale is not None:
            self._perturbed = seg.state_of(unet, "DenoiseLoop(seg_scale=...)")
            seg.check_sigma(seg_sigma)
            pag_scale = seg_scale
        self._perturbed_chunks = 0 if pag_scale is None else (3 if guidance_scale is not None else 2)
        # reference-only control: the UNet's sites must exist, and the reference rows are one more row block behind the others
        self._reference = None
        if reference:
            from . import reference as _reference
            self._reference = _reference.state_of(unet, "DenoiseLoop(reference=True)")
            if pag_scale is not None or tile_hw is not None:
                raise ValueError("DenoiseLoop: reference=True cannot be combined with pag_scale, seg_scale or tile_hw")
            for name, cls in (("regions", _regions.Regions), ("ip_adapter", _ip.IPAdapter), ("t2i_adapter", _t2i.T2IAdapterState),
                              ("controlnet", _cn.ControlNetState)):
                if compiled_state(unet, name, cls) is not None:
                    raise ValueError(f"DenoiseLoop: reference=True cannot be combined with a UNet compiled with {name}: its row-bound "
                                     "state is not verified with a reference row block")
        self._reference_chunks = 0 if not reference else (3 if guidance_scale is not None else 2)
        # regional prompts: the sites are part of the compiled UNet, the text context carries its R prompts side by side
        self._regions_state = compiled_state(unet, "regions", _regions.Regions)
        if self._regions_state is not None and tokens != self._regions_state.R * self._regions_state.seg_len:
            st = self._regions_state
            raise ValueError(f"DenoiseLoop: this UNet was compiled with regions={st.R}, region_tokens={st.seg_len}: build the loop with "
                             f"tokens={st.R * st.seg_len} ({st.R} prompts concatenated), got tokens={tokens}")
        self.unet, self.mode, self.dtype = unet, mode, dtype
        self.device = torch.device(device)
        self.tables = tables or euler_discrete_tables(50)
        n = self.n_steps = self.tables.n_steps
        dev = self.device
        cl = torch.channels_last
        # `latent_hw`: one side of a square latent, or (height, width) - SDXL's aspect buckets (1216 x 832 px = 152 x 104);
        # both sides multiples of 4: the UNet halves the latent twice (Downsample2D, unet_pt.py:246-256) and doubles it back
        lh, lw = (int(latent_hw[0]), int(latent_hw[1])) if isinstance(latent_hw, (tuple, list)) else (int(latent_hw), int(latent_hw))
        self.batch = batch
        # tiled denoising: (lh, lw) is the canvas, the UNet sees its T windows of (th, tw) as batch rows (window-minor)
        self.tile_grid = None
        th, tw, T = lh, lw, 1
        if tile_hw is not None:
            from . import tiles as _tiles
            for name, cls in (("regions", _regions.Regions), ("ip_adapter", _ip.IPAdapter), ("t2i_adapter", _t2i.T2IAdapterState),
                              ("controlnet", _cn.ControlNetState)):
                if compiled_state(unet, name, cls) is not None:
                    raise ValueError(f"DenoiseLoop: tile_hw cannot be combined with a UNet compiled with {name}: its state binds per latent "
                                     "size and row count, and cropping it per window is not built")
            self.tile_grid = _tiles.TileGrid((lh, lw), tile_hw, tile_stride, tile_wrap_w)
            (th, tw), T = self.tile_grid.tile_hw, self.tile_grid.T
            tile_map = _tiles.weight_map(tile_weights, (th, tw))
        elif tile_stride is not None or tile_wrap_w or not (isinstance(tile_weights, str) and tile_weights == "uniform"):
            raise ValueError("DenoiseLoop: tile_stride, tile_wrap_w and tile_weights need tile_hw")
        self._T = T
        # guidance: the UNet sees [negative | positive]; with pag_scale one more block, [.. | perturbed]
        canvas_rows = batch * ((2 if guidance_scale is not None else 1) + (1 if pag_scale is not None else 0) + (1 if reference else 0))
        self._lead_rows = canvas_rows - (batch if reference else 0)      # the row blocks the sampler update reads and writes
        rows = canvas_rows * T
        if self._regions_state is not None:                # the weight buffers of this row count: allocated once, "off"
            self._regions_state.bind(rows, (lh, lw), dev)
        self._ip_state = compiled_state(unet, "ip_adapter", _ip.IPAdapter)
        if self._ip_state is not None:                     # scale table, mask weights, image K/V of this row count: allocated once, "off"
            self._ip_state.bind(rows, (lh, lw), dev)
        # residual sites, T2I-Adapter's or ControlNet's (a UNet carries at most one of the two states): the state's buffers of this
        # row count - T2I features of `batch` rows shared by every row block, ControlNet residuals of `rows` rows -, this loop's own
        # per-step scale table (0 = off) under the feature's name and - with a ControlNet branch - the static buffer of the control
        # image's embedding, `rows` rows: all read by address, allocated once, outside capture
        t2i = compiled_state(unet, "t2i_adapter", _t2i.T2IAdapterState)
        self._sites = t2i if t2i is not None else compiled_state(unet, "controlnet", _cn.ControlNetState)
        self.controlnet, self.controlnet_cond, self._sites_table = controlnet, None, None
        if self._sites is not None:
            self._sites.bind(rows, (lh, lw), dev, dtype, batch if t2i is not None else rows)
            self._sites_table = torch.zeros(n, dtype=torch.float32, device=dev)
            if controlnet is not None:
                self.controlnet_cond = torch.zeros((rows, self._sites.channels[0], lh, lw), dtype=dtype, device=dev).contiguous(
                    memory_format=cl)
        self.t2i_table = self._sites_table if t2i is not None else None
        self.controlnet_table = self._sites_table if t2i is None else None
        self._latent_hw = (th, tw)                         # what the UNet sees: the window when tiled
        if isinstance(self._perturbed, seg.SEG):           # the blur's parameter rows of this latent size: allocated once, outside capture
            self._perturbed.bind((th, tw), dev)
            self._perturbed.set_sigma(seg_sigma)
        self.latent = torch.zeros((batch, 4, lh, lw), dtype=torch.float32, device=dev).contiguous(memory_format=cl)
        self.x_in = torch.zeros((rows, 4, th, tw), dtype=dtype, device=dev).contiguous(memory_format=cl)
        # what the update kernels write: the UNet's own input, or - tiled - a canvas the windows are gathered from; with it the
        # canvas noise prediction the windows' predictions are blended into, and the blend's weight map
        self.x_step, self.eps_canvas, self.tile_weights = self.x_in, None, None
        if self.tile_grid is not None:
            self.x_step = torch.zeros((canvas_rows, 4, lh, lw), dtype=dtype, device=dev).contiguous(memory_format=cl)
            self.eps_canvas = torch.zeros_like(self.x_step)
            self.tile_weights = tile_map.to(dev)
        self.ehs = torch.zeros((rows, tokens, cross_dim), dtype=dtype, device=dev)
        self.text_embeds = torch.zeros((rows, pooled_dim), dtype=dtype, device=dev)
        self.time_ids = torch.zeros((rows, n_time_ids), dtype=dtype, device=dev)
        self.timesteps = torch.tensor(self.tables.timesteps, dtype=torch.float32, device=dev)
        # the update's tables: Euler reads dsigma; DPM-Solver++(2M) its coefficient rows, the previous step's clean-latent
        # prediction (history) and the trajectory's start step; the stochastic samplers the same with a noise column and a
        # device table of one 64-bit seed per sample (int64 holding the seed's bits)
        self.dsigma = self.coef = self.history = self.start = self.seeds = None
        if isinstance(self.tables, SDETables):
            self.coef = torch.tensor(self.tables.coefficients(), dtype=torch.float32, device=dev)
            self.history = torch.zeros_like(self.latent)
            self.start = torch.zeros(1, dtype=torch.int32, device=dev)
            self.seeds = torch.zeros(batch, dtype=torch.int64, device=dev)
        elif isinstance(self.tables, DPMSolverTables):
            self.coef = torch.tensor(self.tables.coefficients(), dtype=torch.float32, device=dev)
            self.history = torch.zeros_like(self.latent)
            self.start = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            self.dsigma = torch.tensor(self.tables.dsigma(), dtype=torch.float32, device=dev)
        self.in_scale = torch.tensor(self.tables.in_scale(), dtype=torch.float32, device=dev)
        self.step_ids = torch.arange(n, dtype=torch.int32, device=dev)      # constants for the unrolled loop
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)           # counter for mode="step"
        # guidance: static per-step tables and the rescale path's scratch, read by address from the captured graph
        self.guidance = self.rescale = self.cfg_workspace = None
        if guidance_scale is not None:
            self.guidance = torch.zeros(n, dtype=torch.float32, device=dev)
            if guidance_rescale is not None:
                self.rescale = torch.zeros(n, dtype=torch.float32, device=dev)
                self.cfg_workspace = ops.cfg_workspace(self.latent)
            self.set_guidance(guidance_scale, guidance_rescale)
        self.pag = None
        if pag_scale is not None:
            self.pag = torch.zeros(n, dtype=torch.float32, device=dev)
            self.pag.copy_(self._step_table(pag_scale, "scale", "set_seg" if isinstance(self._perturbed, seg.SEG) else "set_pag"))
        # masked inpainting (inpaint.py): the latent to keep, the trajectory's unit start noise, the mask (all ones = "off": the blend
        # writes nothing), the threshold table of the differential mode (a NaN entry = no threshold at that step: the mask is the
        # blend weight itself) and sigma[i + 1] per step; canvas-sized when tiled, read by address, allocated once, outside capture
        self.inpaint_init = self.inpaint_noise = self.inpaint_mask = self.inpaint_thr = self.sigma_next = None
        if inpaint:
            self.inpaint_init = torch.zeros_like(self.latent)
            self.inpaint_noise = torch.zeros_like(self.latent)
            self.inpaint_mask = torch.ones((batch, lh, lw), dtype=torch.float32, device=dev)
            self.inpaint_thr = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
            self.sigma_next = torch.tensor(self.tables.sigmas[1:], dtype=torch.float32, device=dev)
        # reference-only control: the reference latent and its unit noise, the scratch latent and the all-zero mask ("keep every
        # pixel") of the launch that re-noises the block for the next step, and the sites' per-step gate (all 0 = off); read by
        # address, allocated once, outside capture
        self.reference_init = self.reference_noise = self._reference_latent = self._reference_mask = self.reference_table = None
        if reference:
            self.reference_init = torch.zeros_like(self.latent)
            self.reference_noise = torch.zeros_like(self.latent)
            self._reference_latent = torch.zeros_like(self.latent)
            self._reference_mask = torch.zeros((1, lh, lw), dtype=torch.float32, device=dev)
            self.reference_table = torch.zeros(n, dtype=torch.float32, device=dev)
            if self.sigma_next is None:
                self.sigma_next = torch.tensor(self.tables.sigmas[1:], dtype=torch.float32, device=dev)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._captured_steps = 0
        # text-context projections are step-invariant: evaluated once per prompt when the compiled
        # UNet exposes the split (optimization._install_context_split)
        self._split = hasattr(unet, "precompute_context") and hasattr(unet, "forward_with_context")
        self.ctx = None
        # the time path (timestep features, embedding MLPs, resnet time projections) depends only on the
        # schedule entry and the added conditioning: one table row per step, filled in set_conditioning
        self._tsplit = self._split and hasattr(unet, "precompute_time")
        self.time_tables = None
        self._conditioned = False        # set_conditioning has filled the static conditioning buffers

    # ---- inputs --------------------------------------------------------------------------
    def set_guidance(self, scale: Union[float, Sequence[float]], rescale: Optional[Union[float, Sequence[float]]] = None) -> None:
        """Guidance scale (and guidance rescale, diffusers' `guidance_rescale`) per step: a float, or a sequence of n_steps floats.
        Written into the device tables in place: the next run uses them without a new capture.  `rescale=None` leaves the
        rescale table as it is."""
        if self.guidance is None:
            raise ValueError("set_guidance: this loop was built without guidance_scale")
        if rescale is not None and self.rescale is None:
            raise ValueError("set_guidance: this loop was built without guidance_rescale")
        g = self._step_table(scale, "scale")
        r = self._step_table(rescale, "rescale") if rescale is not None else None
        self.guidance.copy_(g)
        if r is not None:
            self.rescale.copy_(r)

    def _step_table(self, v, what: str, who: str = "set_guidance") -> torch.Tensor:
        try:
            vals = [float(x) for x in v]
        except TypeError:                                  # a scalar (float, numpy scalar, 0-d tensor)
            vals = [float(v)] * self.n_steps
        if len(vals) != self.n_steps:
            raise ValueError(f"{who}: {what} takes a float or {self.n_steps} values (one per step), got {len(vals)}")
        return torch.tensor(vals, dtype=torch.float32)

    def set_pag(self, scale: Union[float, Sequence[float]]) -> None:
        """Perturbed-attention guidance scale per step: a float, or n_steps floats (pag.adaptive_scales gives diffusers' adaptive
        table).  Written into the device table in place: no new capture.  Scale 0 keeps the perturbed rows and gives the value
        the loop would compute without them."""
        if self.pag is None or isinstance(self._perturbed, seg.SEG):
            raise ValueError("set_pag: this loop was built without pag_scale")
        self.pag.copy_(self._step_table(scale, "scale", "set_pag"))

    def set_seg(self, scale: Optional[Union[float, Sequence[float]]] = None, sigma: Optional[float] = None) -> None:
        """Smoothed energy guidance: the scale per step (a float, or n_steps floats) and / or the blur's sigma (float("inf"): the
        spatial mean).  Both are in-place writes of device buffers the captured graph reads by address: no new capture.  Scale 0
        keeps the perturbed rows and gives the value the loop would compute without them.  sigma belongs to the UNet's SEG state:
        loops that share one compiled UNet share it."""
        if not isinstance(self._perturbed, seg.SEG):
            raise ValueError("set_seg: this loop was built without seg_scale")
        table = self._step_table(scale, "scale", "set_seg") if scale is not None else None
        if sigma is not None:
            self._perturbed.set_sigma(sigma)
        if table is not None:
            self.pag.copy_(table)

    def set_conditioning(self, encoder_hidden_states, text_embeds, time_ids, negative_encoder_hidden_states=None,
                         negative_text_embeds=None, negative_time_ids=None) -> None:
        """Prompt conditioning, B rows each.  With guidance the negative prompt's rows go first; a missing negative text
        state or pooled embedding is zeros (SDXL's force_zeros_for_empty_prompt), missing negative time ids copy the
        positive ones.  A tiled loop takes B rows (repeated over a sample's T windows) or B * T rows (one prompt per window,
        sample-major and window-minor), for the negatives likewise."""
        st = self._regions_state
        if (st is not None and negative_encoder_hidden_states is not None and st.R > 1
                and negative_encoder_hidden_states.shape[1] == st.seg_len):
            # one negative prompt for the whole picture: the same text in every segment
            negative_encoder_hidden_states = negative_encoder_hidden_states.repeat(1, st.R, 1)
        negatives = (negative_encoder_hidden_states, negative_text_embeds, negative_time_ids)
        b = self.batch * self._T                           # rows of one block
        if self.tile_grid is not None:
            encoder_hidden_states, text_embeds, time_ids, *negatives = (
                self._window_rows(t) for t in (encoder_hidden_states, text_embeds, time_ids, *negatives))
            negative_encoder_hidden_states, negative_text_embeds, negative_time_ids = negatives
        if self.guidance is None:
            if any(t is not None for t in negatives):
                raise ValueError("set_conditioning: negative conditioning needs a loop built with guidance_scale")
            for buf, pos in ((self.ehs, encoder_hidden_states), (self.text_embeds, text_embeds), (self.time_ids, time_ids)):
                buf[:b].copy_(pos)
                if self.pag is not None or self._reference is not None:      # the perturbed / reference rows carry the positive conditioning
                    buf[b:].copy_(pos)
        else:
            for buf, pos, neg in ((self.ehs, encoder_hidden_states, negative_encoder_hidden_states),
                                  (self.text_embeds, text_embeds, negative_text_embeds),
                                  (self.time_ids, time_ids, time_ids if negative_time_ids is None else negative_time_ids)):
                buf[b:2 * b].copy_(pos)
                if self.pag is not None or self._reference is not None:      # the perturbed / reference rows carry the positive conditioning
                    buf[2 * b:].copy_(pos)
                if neg is None:
                    buf[:b].zero_()
                else:
                    buf[:b].copy_(neg)
        self._conditioned = True
        self._rederive_conditioning()

    def _window_rows(self, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Tiled: B rows -> each repeated over its sample's T windows; B * T rows -> as they are."""
        if t is None:
            return None
        B, T = self.batch, self._T
        if t.shape[0] == B * T:
            return t
        if t.shape[0] == B:
            return t.repeat_interleave(T, dim=0)
        raise ValueError(f"set_conditioning: a tiled loop takes B = {B} rows (one prompt per sample) or B * T = {B * T} rows (one per "
                         f"window), got {t.shape[0]}")

    def set_tile_weights(self, weights) -> None:
        """The blend's weight map: "uniform", "gaussian" (tiles.gaussian_weights, sigma 0.1) or an (h, w) tensor, finite and positive
        (checked here, on the host).  An in-place write of the device map the blend kernel reads by address: legal before or after
        `capture()`, never a new capture."""
        if self.tile_grid is None:
            raise ValueError("set_tile_weights: this loop was built without tile_hw")
        from . import tiles
        self.tile_weights.copy_(tiles.weight_map(weights, self.tile_grid.tile_hw))

    def set_inpaint(self, init_latent: Optional[torch.Tensor], mask=None, differential: bool = False, thresholds=None) -> None:
        """Masked inpainting (inpaint.py): keep `init_latent` (B or 1, 4, lh, lw) where `mask` is 0 and repaint where it is 1; the
        mask is (lh, lw), (1 | B, lh, lw) or (1 | B, 1, lh, lw) AT LATENT RESOLUTION (the canvas when tiled; inpaint.prepare_mask: finite,
        in [0, 1], never resampled).  Behind every sampler step the pixels to keep are put back to init + sigma[i + 1] * noise with the
        trajectory's own start noise (what set_noise / set_image / a seed started it from), a fractional mask value blends, and after
        the last step (sigma = 0) a pixel at mask 0 is `init_latent` bit for bit.  `differential=True` reads the mask as a change
        map (Differential Diffusion): a pixel of value m is frozen after step i while m <= thr[i], thr = `thresholds` (n_steps
        floats in [0, 1]) or inpaint.differential_thresholds(n_steps).  `set_inpaint(None)` is "off": the mask is all ones, the
        blend writes nothing, and the loop gives the bits of one built without `inpaint`.

        In-place writes of device buffers the captured graph reads by address, legal before or after `capture()`, never a new
        capture.  The two modes share one captured launch: the threshold table is always passed, and a table of NaN - the state
        without `differential` - tells the kernel to take the mask itself as the weight.  All arguments are validated before
        anything is written.  Strength 1: mode "loop", `set_inpaint`, `denoise`.  Partial strength: `set_image(init, noise, strength)`
        in mode "step" / "eager", `set_inpaint(init, mask)`, `run_steps`."""
        if self.inpaint_mask is None:
            raise ValueError("set_inpaint: this loop was built without inpaint=True")
        from . import inpaint
        if init_latent is None:
            if mask is not None or differential or thresholds is not None:
                raise ValueError("set_inpaint: takes (init_latent, mask[, differential, thresholds]) or None")
            self.inpaint_mask.fill_(1.0)
            self.inpaint_thr.fill_(float("nan"))
            return
        if mask is None:
            raise ValueError("set_inpaint: a mask is needed with init_latent (1 = repaint, 0 = keep)")
        init = torch.as_tensor(init_latent)
        if init.dim() != 4 or init.shape[0] not in (1, self.batch) or tuple(init.shape[1:]) != tuple(self.latent.shape[1:]):
            raise ValueError(f"set_inpaint: init_latent must be (1 | {self.batch}, {', '.join(str(v) for v in self.latent.shape[1:])}), got "
                             f"{tuple(init.shape)}")
        m = inpaint.prepare_mask(mask, self.batch, tuple(self.latent.shape[-2:]))
        if thresholds is not None and not differential:
            raise ValueError("set_inpaint: thresholds need differential=True")
        thr = torch.full((self.n_steps,), float("nan"), dtype=torch.float32)
        if differential:
            thr = inpaint.differential_thresholds(self.n_steps) if thresholds is None else self._step_table(thresholds, "thresholds", "set_inpaint")
            if thr.numel() != self.n_steps or not bool(torch.isfinite(thr).all()) or bool((thr < 0).any()) or bool((thr > 1).any()):
                raise ValueError(f"set_inpaint: thresholds are {self.n_steps} finite values in [0, 1]")
        self.inpaint_init.copy_(init.detach().to(self.device, torch.float32).expand_as(self.inpaint_init))
        self.inpaint_mask.copy_(m.expand_as(self.inpaint_mask))
        self.inpaint_thr.copy_(thr)

    def set_reference(self, latent: Optional[torch.Tensor], noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                      start: float = 0.0, end: float = 1.0) -> None:
        """Reference-only control: `latent` (1 | B, 4, lh, lw) is the reference image's latent; at step i the reference rows see
        (latent + sigma[i] * noise) * in_scale[i].  `noise`: unit noise of the same shape, or `seed`: an int (or B ints) in [0, 2^64)
        for rng.py's stream at counter word REFERENCE_COUNTER_WORD = 2^32 - 1 (the start noise is word 0 and step i's noise word i + 1,
        i < n_steps: no collision); the seeds are the call's own and leave `set_seed`'s table alone.  The sites are on for the steps
        in [int(start * n), int(end * n)).  `set_reference(None)` switches them off: the table is zeroed, the reference rows' keys are
        no longer read, and the result does not depend on the reference.
        In-place writes of device buffers the captured graph reads by address, legal before or after `capture()`, never a new capture.
        Call it before `set_noise` / `set_image` (they write the reference block's first input), or again after them: the call itself
        writes that input for the step the counter stands at, which it reads with `step.item()` - one host synchronisation."""
        if self._reference is None:
            raise ValueError("set_reference: this loop was built without reference=True")
        if latent is None:
            if noise is not None or seed is not None:
                raise ValueError("set_reference: takes (latent, noise | seed[, start, end]) or None")
            self.reference_table.zero_()
            return
        n = self.n_steps
        if not (0.0 <= float(start) <= float(end) <= 1.0):
            raise ValueError(f"set_reference: 0 <= start <= end <= 1 expected, got start={start}, end={end}")
        lat = torch.as_tensor(latent)
        if lat.dim() != 4 or lat.shape[0] not in (1, self.batch) or tuple(lat.shape[1:]) != tuple(self.latent.shape[1:]):
            raise ValueError(f"set_reference: latent must be (1 | {self.batch}, {', '.join(str(v) for v in self.latent.shape[1:])}), got "
                             f"{tuple(lat.shape)}")
        if (noise is None) == (seed is None):
            raise ValueError("set_reference: pass noise or seed (one of them)")
        if noise is not None:
            z = torch.as_tensor(noise)
            if z.dim() != 4 or z.shape[0] not in (1, self.batch) or tuple(z.shape[1:]) != tuple(self.latent.shape[1:]):
                raise ValueError(f"set_reference: noise must have the latent's shape, got {tuple(z.shape)}")
            z = z.detach().to(self.device, torch.float32).expand_as(self.reference_noise)
        else:
            z = torch.empty_like(self.latent)
            ops.philox_normal(z, self._seed_bits(seed, "set_reference").to(self.device), REFERENCE_COUNTER_WORD)
        table = torch.zeros(n, dtype=torch.float32)
        table[int(float(start) * n):int(float(end) * n)] = 1.0
        self.reference_init.copy_(lat.detach().to(self.device, torch.float32).expand_as(self.reference_init))
        self.reference_noise.copy_(z)
        self.reference_table.copy_(table)
        self._write_reference_input(int(self.step.item()) % n)

    def _rederive_conditioning(self) -> None:
        """Everything the loop computes once per prompt from the weights and its own static `ehs`, `text_embeds` and
        `time_ids` buffers, (re)computed IN PLACE: derived weights, the hoisted text-context K/V, the time tables.  Runs
        after new conditioning and after a weight change (LoRA load / scale / unload); never needs a new capture."""
        self.refresh_weights()
        if self._split:
            with torch.no_grad():
                new = self.unet.precompute_context(self.ehs)
            if self.ctx is None:
                self.ctx = tuple(t.clone() for t in new)          # static buffers the captured graph reads
            else:
                for dst, src in zip(self.ctx, new):
                    dst.copy_(src)
        if self._tsplit:
            # every schedule entry in ONE pass: the time path sees n_steps * batch rows (row s*B + b = step s, sample b),
            # so its GEMMs run once with M = n_steps * batch instead of n_steps times with M = batch
            n, b = self.n_steps, self.ehs.shape[0]
            with torch.no_grad():
                rows = self.x_in.new_empty((n * b, 1, 1, 1))                       # read for its batch size and dtype only
                cond = {"text_embeds": self.text_embeds.repeat(n, 1), "time_ids": self.time_ids.repeat(n, 1)}
                out = self.unet.precompute_time(rows, self.timesteps.repeat_interleave(b), cond)
                new = tuple(o.reshape(n, b, *o.shape[1:]) for o in out)
            if self.time_tables is None:
                self.time_tables = tuple(t.clone() for t in new)
            else:
                for dst, src in zip(self.time_tables, new):
                    dst.copy_(src)

    def refresh_weights(self) -> int:
        """Captured graphs read derived weight buffers (fused q|k|v, LayerNorm-folded projections) by address: after an
        in-place weight update (LoRA merge) re-derive them in place.  Called per prompt; call it yourself after updating
        weights between two runs of the same prompt."""
        ectx = getattr(self.unet, "exec_context", None)
        return ectx.refresh_derived(full=True) if ectx is not None else 0

    # ---- LoRA adapters (lora.py): merged into the UNet's weights in place, no new capture ------------------------------
    def _lora_set(self):
        from . import lora
        if not isinstance(self.unet, torch.nn.Module):
            raise TypeError("LoRA adapters need the loop's unet to be a module (the result of optimize_model)")
        return lora.attach(self.unet)

    def _weights_changed(self) -> None:
        """After a merge: the weights kept their addresses, so the captured graph stays; what was computed FROM them is
        recomputed in place - derived weights always, the hoisted text K/V and the time tables once conditioning is set -
        and under the fp8 plan the delayed scales are measured again, as at a trajectory start (set_noise)."""
        if self._conditioned:
            self._rederive_conditioning()
            if getattr(self.unet, "fp8_plan", False):
                self._recalibrate(int(self.step.item()) % self.n_steps)
        else:
            self.refresh_weights()

    def load_lora(self, name: str, state_dict, scale: float = 1.0, strict: bool = True, convs: bool = False, lycoris: bool = False):
        """Merge a LoRA state dict (PEFT / diffusers / kohya keys, lora.parse_lora_state_dict) into the UNet at `scale`.
        DoRA magnitudes apply; `convs=True` also takes the adapter's convolution factors (LoCon) on the UNet's Conv2d,
        `lycoris=True` its Tucker cores, LoHa and LoKr factors (lora.py).
        Returns the keys that were not applied.  A loop that shares its UNet with another owner shares the adapters; the
        other owner re-derives its own per-prompt state (its next set_conditioning does)."""
        left = self._lora_set().load(name, state_dict, scale, strict, convs, lycoris)
        self._weights_changed()
        return left

    def set_lora_scale(self, name: str, scale: float) -> None:
        self._lora_set().set_scale(name, scale)
        self._weights_changed()

    def unload_lora(self, name: str) -> None:
        """Remove an adapter; with none left every weight has its original bits again."""
        self._lora_set().unload(name)
        self._weights_changed()

    def set_freeu(self, s1: Optional[float] = None, s2: Optional[float] = None, b1: Optional[float] = None,
                  b2: Optional[float] = None, version: int = 1) -> None:
        """FreeU parameters (freeu.py; diffusers' argument order; version 1 = diffusers, 2 = ComfyUI FreeU_V2), or
        `set_freeu(None)` for neutral ones.  An in-place write of the device row the UNet's FreeU sites read: the next run
        uses it without a new capture.  The UNet must have been compiled with `freeu=True`."""
        from . import freeu
        state = freeu.state_of(self.unet, "set_freeu")
        if s1 is None:
            if not (s2 is None and b1 is None and b2 is None):
                raise ValueError("set_freeu: takes (s1, s2, b1, b2[, version]) or None")
            state.disable()
        else:
            state.set(s1, s2, b1, b2, version)

    def set_regions(self, masks: Optional[torch.Tensor]) -> None:
        """Region masks (regions.py): (R, lh, lw) for every sample or (B, R, lh, lw), non-negative, at latent resolution; segment r
        of the text context conditions the cells where mask r has weight (normalised over r per cell; a cell no mask covers takes
        segment 0).  The negative block under guidance keeps segment 0, PAG's perturbed block takes the positive weights.
        `set_regions(None)` is "off".  An in-place write of the buffers the UNet's cross-attention sites read: no new capture, legal
        before or after `capture()`.  The UNet must have been compiled with `regions=R`.  A loop that shares its UNet and its row
        count with another owner shares the weights."""
        from . import regions
        state = regions.state_of(self.unet, "set_regions")
        rows = self.x_in.shape[0]
        if masks is None:
            state.clear(rows)
            return
        if torch.is_tensor(masks) and masks.dim() == 4 and masks.shape[0] != self.batch:
            raise ValueError(f"set_regions: per-sample masks need B = {self.batch} entries, got {tuple(masks.shape)}")
        if torch.is_tensor(masks) and tuple(masks.shape[-2:]) != tuple(self.latent.shape[-2:]):
            raise ValueError(f"set_regions: masks are given at latent resolution {tuple(self.latent.shape[-2:])}, got {tuple(masks.shape)}")
        first = self.batch if self.guidance is not None else 0
        state.set(masks, range(first, rows), rows)

    # ---- IP-Adapter image prompts (ip_adapter.py): in-place writes of buffers the sites read by address, no new capture -----
    def _ip(self, what: str):
        from . import ip_adapter
        return ip_adapter.state_of(self.unet, what)

    def load_ip_adapter(self, state_dict, slot: int = 0):
        """Copy an IP-Adapter checkpoint's to_k_ip / to_v_ip weights into adapter slot `slot` (ip_adapter.IPAdapter.load: the
        published {"image_proj", "ip_adapter"} layout, the same flattened, or path-spelled keys; validated before anything is
        written).  Returns the checkpoint's image_proj sub-dict (ip_adapter.project_image_embeds turns CLIP image embeddings into
        tokens with it).  The UNet must have been compiled with `ip_adapter=N`.  Call `set_ip_adapter_image` afterwards."""
        return self._ip("load_ip_adapter").load(state_dict, slot)

    def set_ip_adapter_image(self, tokens: torch.Tensor, negative_tokens: Optional[torch.Tensor] = None, slot: int = 0) -> None:
        """Image tokens (B or 1, N, cross_dim) of slot `slot`, projected once into every site's K/V buffers.  Under guidance the
        negative block takes `negative_tokens` (default: zero tokens = no contribution), PAG's perturbed block the positive ones."""
        rows = self.x_in.shape[0]
        self._ip("set_ip_adapter_image").set_image(tokens, negative_tokens, slot, rows, rows // self.batch, self.guidance is not None)

    def set_ip_adapter_scale(self, scale, slot: int = 0) -> None:
        """A float for every site, or a mapping {regular expression on the site paths: float} (first match wins, "mid" selects the
        middle block, unmatched sites get 0).  Scale 0 switches a site's image attention off at no cost."""
        self._ip("set_ip_adapter_scale").set_scale(scale, slot)

    def set_ip_adapter_masks(self, masks: Optional[torch.Tensor], slot: int = 0) -> None:
        """Where slot `slot`'s image prompt applies: (lh, lw) or (B, lh, lw) at latent resolution, non-negative; None = everywhere."""
        if masks is not None:
            m = torch.as_tensor(masks)
            if m.dim() == 3 and m.shape[0] != self.batch:
                raise ValueError(f"set_ip_adapter_masks: per-sample masks need B = {self.batch} entries, got {tuple(m.shape)}")
            if tuple(m.shape[-2:]) != tuple(self.latent.shape[-2:]):
                raise ValueError(f"set_ip_adapter_masks: masks are given at latent resolution {tuple(self.latent.shape[-2:])}, got {tuple(m.shape)}")
        self._ip("set_ip_adapter_masks").set_masks(masks, slot, self.x_in.shape[0])

    def unload_ip_adapter(self, slot: int = 0) -> None:
        """Slot `slot` back to "off": scale 0, weights and image K/V zero, masks 1 - the bits of the loop before the adapter."""
        self._ip("unload_ip_adapter").unload(slot)

    # ---- T2I-Adapter (t2i_adapter.py): in-place writes of buffers the residual sites read by address, no new capture ---------
    def set_t2i_adapter(self, features, scale: float = 1.0, factor: float = 1.0) -> None:
        """The adapter's feature maps, one per site, each (B or 1, C_k, h_k, w_k) (t2i_adapter.FullAdapterXL on the control image;
        several adapters: the sum of their features), and the per-step scale table: `scale` for the steps i < int(n_steps * factor),
        0 after (diffusers' `adapter_conditioning_scale` / `adapter_conditioning_factor`).  Every row block of the UNet batch reads the
        same copy.  `set_t2i_adapter(None)` is "off": the bits of a UNet compiled without sites.  In-place writes, legal before or
        after `capture()`.  The UNet must have been compiled with `t2i_adapter=True`; a loop that shares its UNet and its row count
        with another shares the feature buffers (not the scales)."""
        from . import t2i_adapter
        state = t2i_adapter.state_of(self.unet, "set_t2i_adapter")
        if features is None:
            self.t2i_table.zero_()
            return
        table = t2i_adapter.scale_table(self.n_steps, scale, factor)
        state.set(features, None, self.x_in.shape[0])
        self.t2i_table.copy_(table)

    def set_t2i_adapter_scale(self, scale: Union[float, Sequence[float]]) -> None:
        """The sites' scale per step: a float, or n_steps floats.  Written into the device table in place: no new capture."""
        from . import t2i_adapter
        self._set_sites_scale(t2i_adapter, "set_t2i_adapter_scale", scale)

    def _set_sites_scale(self, feature, what: str, scale, site_weights=None) -> None:
        state = feature.state_of(self.unet, what)
        table = self._step_table(scale, "scale", what)      # (validated before anything is written)
        if site_weights is not None:
            state.set_site_weights(site_weights)
        self._sites_table.copy_(table)

    # ---- ControlNet (controlnet.py): in-place writes of buffers the branch and the sites read by address, no new capture --------
    def set_controlnet(self, image_or_cond_embed, scale: float = 1.0, start: float = 0.0, end: float = 1.0) -> None:
        """The control image (1, B or rows, 3, 8 lh, 8 lw) - embedded here by the branch's eager `embed_condition`, once - or its
        ready embedding (1, B or rows, widths[0], lh, lw), and the per-step scale table: `scale` for the steps
        int(n_steps * start) <= i < int(n_steps * end), 0 for the rest (diffusers' `controlnet_conditioning_scale`,
        `control_guidance_start` / `_end`).  Every row block of the UNet batch sees the same control.  `set_controlnet(None)` is
        "off": the bits of a loop on a UNet compiled without sites (the branch still runs: the captured graph is static).  In-place
        writes, legal before or after `capture()`.  The UNet must have been compiled with `controlnet=True`.  (An image is embedded by
        eager torch convolutions, which do not promise the same bits from one call to the next: two loops that are to agree bit for
        bit are handed one embedding.)"""
        from . import controlnet as _cn
        _cn.state_of(self.unet, "set_controlnet")
        if image_or_cond_embed is None:
            self.controlnet_table.zero_()
            return
        if self.controlnet is None:
            raise ValueError("set_controlnet: this loop was built without controlnet= (the compiled branch)")
        table = _cn.scale_table(self.n_steps, scale, start, end)
        c = image_or_cond_embed
        buf = self.controlnet_cond
        lh, lw = buf.shape[-2:]
        if torch.is_tensor(c) and c.dim() == 4 and c.shape[1] != buf.shape[1] and tuple(c.shape[-2:]) == (8 * lh, 8 * lw):
            embed = getattr(self.controlnet, "embed_condition", None)
            if embed is None:
                raise ValueError("set_controlnet: this branch has no embed_condition (the eager embedding of a control image); pass "
                                 "the embedding itself")
            p = next(self.controlnet.parameters())
            c = embed(c.to(p.device, p.dtype))
        if not torch.is_tensor(c) or c.dim() != 4 or tuple(c.shape[1:]) != tuple(buf.shape[1:]) or c.shape[0] < 1 or buf.shape[0] % c.shape[0]:
            shape = tuple(c.shape) if torch.is_tensor(c) else type(c).__name__
            raise ValueError(f"set_controlnet: takes a control image (rows, 3, {8 * lh}, {8 * lw}) or its embedding (rows, {buf.shape[1]}, "
                             f"{lh}, {lw}) with rows 1, the batch {self.batch} or all {buf.shape[0]}, got {shape}")
        buf.copy_(c.detach().to(buf.device, buf.dtype).repeat(buf.shape[0] // c.shape[0], 1, 1, 1))
        self.controlnet_table.copy_(table)

    def set_controlnet_scale(self, scale: Union[float, Sequence[float]], site_weights: Optional[Sequence[float]] = None) -> None:
        """The sites' scale per step: a float, or n_steps floats; `site_weights`: one factor per site on top of it (the skips in
        encoder order, the middle block's last; they belong to the UNet's state: loops that share one compiled UNet share them).
        Written into the device tables in place: no new capture."""
        from . import controlnet as _cn
        self._set_sites_scale(_cn, "set_controlnet_scale", scale, site_weights)

    def set_seed(self, seed: Union[int, Sequence[int]]) -> None:
        """The generator's seeds (rng.py): B ints in [0, 2^64), one per latent sample, or one int s for seeds s, s + 1, ...,
        s + B - 1 (mod 2^64).  Written into the device table in place: a captured graph reads it by address."""
        bits = self._seed_bits(seed, "set_seed")
        if self.seeds is None:                             # Euler / DPM++: only the initial noise reads the seeds
            self.seeds = torch.zeros(self.batch, dtype=torch.int64, device=self.device)
        self.seeds.copy_(bits)

    def _seed_bits(self, seed: Union[int, Sequence[int]], who: str) -> torch.Tensor:
        """`seed` as set_seed takes it -> a host int64 tensor of B entries holding the seeds' 64 bits."""
        def integer(v) -> bool:
            return isinstance(v, numbers.Integral) and not isinstance(v, bool)

        if integer(seed):
            s0 = int(seed)
            vals = [(s0 + b) % (1 << 64) if 0 <= s0 < 1 << 64 else s0 for b in range(self.batch)]
        else:
            try:
                vals = list(seed)
            except TypeError:
                raise ValueError(f"{who}: takes one int or B = {self.batch} ints, got {seed!r}") from None
            if not all(integer(v) for v in vals):
                raise ValueError(f"{who}: seeds are integers, got {vals!r}")
            vals = [int(v) for v in vals]
        if len(vals) != self.batch:
            raise ValueError(f"{who}: takes one int or B = {self.batch} ints, got {len(vals)}")
        if any(v < 0 or v >= 1 << 64 for v in vals):
            raise ValueError(f"{who}: seeds are 64-bit unsigned integers, in [0, 2^64)")
        return torch.tensor([v - (1 << 64) if v >= 1 << 63 else v for v in vals], dtype=torch.int64)

    def _seeded_unit(self, counter: int) -> torch.Tensor:
        z = torch.empty_like(self.latent)
        ops.philox_normal(z, self.seeds, counter)
        return z

    def set_noise(self, latent_unit: Optional[torch.Tensor] = None, seed: Optional[Union[int, Sequence[int]]] = None) -> None:
        """latent_unit ~ N(0,1); scaled by the scheduler's init sigma (fp32 state).  With `seed` the seeds are set first
        (set_seed), and without latent_unit the unit noise is the generator's stream at counter word 0."""
        if seed is not None:
            self.set_seed(seed)
        if latent_unit is None:
            if seed is None:
                raise ValueError("set_noise: pass latent_unit, seed, or both")
            latent_unit = self._seeded_unit(0)
        if self.inpaint_noise is not None:                 # the noise the blend re-noises the kept pixels with
            self.inpaint_noise.copy_(latent_unit)
        self.latent.copy_(latent_unit.to(self.device, torch.float32) * self.tables.init_noise_sigma)
        self._write_input(float(self.tables.in_scale()[0]))
        self._write_reference_input(0)
        self.step.zero_()
        if self.start is not None:
            self.start.zero_()
        self._recalibrate(0)

    def set_image(self, init_latent: torch.Tensor, noise_unit: Optional[torch.Tensor], strength: float,
                  seed: Optional[Union[int, Sequence[int]]] = None) -> int:
        """img2img start (the refiner's use, BASELINE config #5; restated diffusers img2img: `get_timesteps` +
        `scheduler.add_noise`): skip the first n - int(n * strength) schedule entries, start from
        init_latent + noise * sigma[t_start].  Returns the number of steps left to run (`run_steps(k)`, mode step / eager).
        With `seed` the seeds are set first, and noise_unit=None takes the generator's stream at counter word 0."""
        if self.mode == "loop":
            raise ValueError("set_image needs mode='step' or 'eager': the captured full-trajectory loop cannot start mid-schedule")
        n = self.n_steps
        t_start = max(n - min(int(n * strength), n), 0)
        if t_start >= n:
            raise ValueError(f"strength {strength} leaves no denoise step of the {n}-step schedule (int(n * strength) == 0)")
        if seed is not None:
            self.set_seed(seed)
        if noise_unit is None:
            if seed is None:
                raise ValueError("set_image: pass noise_unit, seed, or both")
            noise_unit = self._seeded_unit(0)
        if self.inpaint_noise is not None:
            self.inpaint_noise.copy_(noise_unit)
        sigma = float(self.tables.sigmas[t_start])
        lat = init_latent.to(self.device, torch.float32) + noise_unit.to(self.device, torch.float32) * sigma
        self.latent.copy_(lat)
        self._write_input(float(self.tables.in_scale()[t_start]))
        self._write_reference_input(t_start)
        self.step.fill_(t_start)
        if self.start is not None:
            self.start.fill_(t_start)
        self._recalibrate(t_start)
        return n - t_start

    def _write_input(self, scale: float) -> None:
        if self.guidance is None and self.pag is None and self._reference is None:
            self.x_step.copy_(self.latent * scale)
        else:
            v = self.latent * scale
            for r in range(self._lead_rows // self.batch):      # every row block sees the same latent
                self.x_step[r * self.batch:(r + 1) * self.batch].copy_(v)
        self._gather_windows()

    def _write_reference_input(self, i: int) -> None:
        """The reference block's input of schedule entry i, the trajectory's start: (init + sigma[i] * noise) * in_scale[i]."""
        if self._reference is not None:
            v = (self.reference_init + self.reference_noise * float(self.tables.sigmas[i])) * float(self.tables.in_scale()[i])
            self.x_step[self._lead_rows:].copy_(v)

    def _gather_windows(self) -> None:
        if self.tile_grid is not None:                     # the UNet's input: the windows of the canvas the update wrote
            g = self.tile_grid
            ops.tile_gather(self.x_step, self.x_in, g.ys, g.xs, g.wrap_w)

    def _recalibrate(self, i: int) -> None:
        """fp8 plan only: a trajectory starts from scales measured on its own first evaluation (not on the last step of
        whatever ran before), so the same inputs always give the same outputs."""
        if self.ctx is None and self._split:
            return                                   # no prompt yet: the first evaluation after compile measures by itself
        from .optimization import recalibrate_fp8
        row = tuple(tbl[i] for tbl in self.time_tables) if (self._tsplit and self.time_tables is not None) else None
        recalibrate_fp8(self.unet, lambda: self._unet(self.timesteps[i], row))

    # ---- one step ------------------------------------------------------------------------
    def _cond(self) -> Dict[str, torch.Tensor]:
        return {"text_embeds": self.text_embeds, "time_ids": self.time_ids}

    def _unet(self, t, time_row=None, step=None):
        with contextlib.ExitStack() as scopes:      # both for this loop's own calls only
            if self._sites is not None:          # the residual sites read this loop's scale table at `step`
                lent = ()
                if self.controlnet is not None:  # the branch on the UNet's own rows, then its outputs lent to the sites (no copies)
                    down, mid = self.controlnet(self.x_in, t, self.ehs, self._cond(), cond_embed=self.controlnet_cond)
                    lent = (list(down) + [mid],)
                scopes.enter_context(self._sites.using(self.step_ids[0:1] if step is None else step, self._sites_table, *lent))
            if self._reference is not None:      # the last B rows are the reference block; the sites read this loop's gate at `step`
                scopes.enter_context(self._reference.using(self._reference_chunks, step=self.step_ids[0:1] if step is None else step,
                                                           table=self.reference_table))
            if self._perturbed is not None:      # the last B rows are the perturbed block; SEG's sites derive their token grids from the latent size
                scopes.enter_context(self._perturbed.using(self._perturbed_chunks, self._latent_hw))
            return self._unet_call(t, time_row)

    def _unet_call(self, t, time_row=None):
        if self._split:
            if self.ctx is None:
                raise RuntimeError("set_conditioning() must be called before running the loop")
            if self._tsplit:
                return self.unet.forward_with_context(self.x_in, t, self.ctx, self._cond(), time_cache=time_row)[0]
            return self.unet.forward_with_context(self.x_in, t, self.ctx, self._cond())[0]
        return self.unet(self.x_in, t, self.ehs, self._cond())[0]

    def _step_const(self, i: int) -> None:
        row = tuple(tbl[i] for tbl in self.time_tables) if self._tsplit else None      # static views: no launch
        eps = self._unet(self.timesteps[i], row, self.step_ids[i:i + 1])
        self._update(eps, self.step_ids[i:i + 1])

    def _step_counted(self) -> None:
        idx = self.step.long()
        t = self.timesteps.index_select(0, idx)[0]
        row = tuple(tbl.index_select(0, idx)[0] for tbl in self.time_tables) if self._tsplit else None
        eps = self._unet(t, row, self.step)
        self._update(eps, self.step)
        ops.step_advance(self.step, self.n_steps)

    def _update(self, eps: torch.Tensor, step: torch.Tensor) -> None:
        if self.tile_grid is not None:                     # the windows' predictions -> one prediction per canvas pixel
            g = self.tile_grid
            ops.tile_blend(eps, self.eps_canvas, self.tile_weights, g.ys, g.xs, g.wrap_w)
            eps = self.eps_canvas
        if self._reference is not None:                    # the sampler sees the leading row blocks (views): its kernels are unchanged
            eps = eps[:self._lead_rows]
        self._sampler_update(eps, step)
        if self.inpaint_mask is not None:                  # behind the update, on what it wrote: pixels to repaint are not touched
            ops.inpaint_blend(self.latent, self._x_lead, self.inpaint_init, self.inpaint_noise, self.inpaint_mask, self.sigma_next,
                              self.in_scale, step, self.inpaint_thr)
        if self._reference is not None:                    # the reference block's next input: every pixel "kept" = init + sigma[i + 1] * noise
            ops.inpaint_blend(self._reference_latent, self.x_step[self._lead_rows:], self.reference_init, self.reference_noise,
                              self._reference_mask, self.sigma_next, self.in_scale, step, None)
        self._gather_windows()

    @property
    def _x_lead(self) -> torch.Tensor:
        """What the update kernels write: `x_step`, without the reference block when there is one."""
        return self.x_step if self._reference is None else self.x_step[:self._lead_rows]

    def _sampler_update(self, eps: torch.Tensor, step: torch.Tensor) -> None:
        if self.pag is not None:
            if isinstance(self.tables, SDETables):
                ops.pag_sde_step(self.latent, eps, self._x_lead, self.history, self.coef, self.in_scale, step, self.start, self.seeds,
                                 self.pag, self.guidance, self.rescale, self.cfg_workspace)
            elif self.coef is not None:
                ops.pag_dpmpp2m_step(self.latent, eps, self._x_lead, self.history, self.coef, self.in_scale, step, self.start, self.pag,
                                     self.guidance, self.rescale, self.cfg_workspace)
            else:
                ops.pag_euler_step(self.latent, eps, self._x_lead, self.dsigma, self.in_scale, self.guidance, self.pag, step, self.rescale,
                                   self.cfg_workspace)
        elif isinstance(self.tables, SDETables):
            ops.sde_step(self.latent, eps, self._x_lead, self.history, self.coef, self.in_scale, step, self.start, self.seeds,
                         self.guidance, self.rescale, self.cfg_workspace)
        elif self.coef is not None:
            ops.dpmpp2m_step(self.latent, eps, self._x_lead, self.history, self.coef, self.in_scale, step, self.start, self.guidance,
                             self.rescale, self.cfg_workspace)
        elif self.guidance is None:
            ops.euler_step(self.latent, eps, self._x_lead, self.dsigma, self.in_scale, step)
        else:
            ops.cfg_euler_step(self.latent, eps, self._x_lead, self.dsigma, self.in_scale, self.guidance, step, self.rescale,
                               self.cfg_workspace)

    # ---- capture / run -------------------------------------------------------------------
    def capture(self, warmup: int = 1) -> None:
        if self.mode == "eager" or self.graph is not None:
            return
        keep = (self.latent.clone(), self.x_in.clone(), self.step.clone(), None if self.history is None else self.history.clone(),
                None if self.tile_grid is None else self.x_step.clone())
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step_counted() if self.mode == "step" else self._step_const(0)
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        self._restore(keep)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with no_gc_during_capture(), torch.cuda.graph(g):
            if self.mode == "step":
                self._step_counted()
                self._captured_steps = 1
            else:
                for i in range(self.n_steps):
                    self._step_const(i)
                self._captured_steps = self.n_steps
        self.graph = g
        self._restore(keep)
        # (fp8 plan: the warm-up evaluation above measured the scales its own way; start them over exactly as set_noise /
        #  set_image do, so the first trajectory after a capture equals every later one)
        self._recalibrate(int(keep[2].item()) % self.n_steps)

    def _restore(self, keep) -> None:
        self.latent.copy_(keep[0]); self.x_in.copy_(keep[1]); self.step.copy_(keep[2])
        if keep[3] is not None:
            self.history.copy_(keep[3])
        if keep[4] is not None:
            self.x_step.copy_(keep[4])

    def run_steps(self, k: int) -> None:
        """Advance exactly k denoise steps from the current state (asynchronous)."""
        if self.mode == "eager":
            s = int(self.step.item())
            for i in range(k):
                self._step_const((s + i) % self.n_steps)
            self.step.fill_((s + k) % self.n_steps)
            return
        self.capture()
        if self.mode == "loop":
            if k % self.n_steps != 0:
                raise ValueError(f"mode='loop' runs whole {self.n_steps}-step loops; got k={k}")
            for _ in range(k // self.n_steps):
                self.graph.replay()
        else:
            for _ in range(k):
                self.graph.replay()

    def denoise(self, latent_unit: Optional[torch.Tensor] = None,
                seed: Optional[Union[int, Sequence[int]]] = None) -> torch.Tensor:
        """Full trajectory: unit noise (or a seed, set_noise) in, final fp32 latent (NCHW contiguous) out."""
        self.set_noise(latent_unit, seed)
        self.run_steps(self.n_steps)
        return self.latent.contiguous(memory_format=torch.contiguous_format).clone()
