"""Compile entry point: `model = optimize_model(model, cuda_graph)`.

Same surface as reference src/stabletriton/optimization.py:10-38 (README.md:5
calls it `compile`): trace the eager module with torch.fx, run the rewrite
passes in a fixed order (fused variants claim their nodes first), optionally
wrap `forward` in the shape-keyed hipGraph cache.  The returned GraphModule is
callable with the original forward signature; the caller re-attaches `.config`
(implementations/Diffusers/load_sdxl_pipeline.py:29-34) or uses
`stabletriton_amd.hooks`.
"""
from __future__ import annotations

from typing import Dict, Union

import torch
from torch import fx, nn

from . import _C, ops
from . import controlnet as _controlnet
from . import t2i_adapter as _t2i
from .ip_adapter import check_combination
from .optimizers import (dedupe_pure_calls, fuse_token_residual, fuse_attention, fuse_geglu, fuse_geglu_into_linear, fuse_groupnorm_stats, fuse_skip_cat, fuse_layernorm_into_linear, fuse_query_projection_into_attention, fuse_residual_adds,
                         fuse_shared_input_linears,
                         fuse_temb_add, fuse_timesteps, insert_controlnet, insert_freeu, insert_t2i_adapter, insert_ip_adapter, insert_pag, insert_reference, insert_regions, insert_seg, split_context, split_region, keep_channels_last, make_dynamic_graphed_callable, plan_fp8, remove_dropout,
                         replace_conv, replace_group_norm, replace_group_norm_activation, replace_layer_norm,
                         replace_linear, replace_linear_activ)


def replace_backend(gm: Union[fx.GraphModule, nn.Module], fuse: bool = True, fp8: bool = False, xattn_fusion: bool = True,
                    gn_stats: bool = True, freeu: bool = False, pag_layers=None, regions=None, region_tokens: int = 77,
                    ip_adapter=None, seg_layers=None, t2i_adapter: bool = False, controlnet: bool = False,
                    reference_layers=None) -> fx.GraphModule:
    """Pass pipeline over a traced module; an untraced nn.Module is traced here, after the flags were checked against each other
    (optimize_model relies on it: a bad combination raises before the trace).  The first eight passes and their order are the reference's
    (optimization.py:10-22); replace_linear is enabled (the MFMA GEMM is the
    product here), replace_conv / epilogue fusions / layout are additions.
    `xattn_fusion` / `gn_stats` switch two of the added fusions off (A/B measurements).  `freeu` (addition, off by default:
    the graph is then exactly the one without it) puts a FreeU site in front of the decoder concatenations of the first two
    stages and installs the neutral parameter state as `gm.freeu` (freeu.py).  `pag_layers` (addition, off by default, likewise):
    regular expressions selecting the self-attention sites that take perturbed batch entries (optimizers/insert_pag.py); the state,
    `gm.pag`, starts with chunks 0 = ordinary attention.  `regions=R` (addition, off by default, likewise): every cross-attention
    site runs R key/value segments of `region_tokens` keys with their own softmax, combined by the weights of `gm.regions`
    (optimizers/insert_regions.py, regions.py); those sites keep their query projection as a launch of its own.  `ip_adapter=N` or a
    tuple of up to 4 image token counts (addition, off by default, likewise): every cross-attention site adds a decoupled attention
    over the image tokens of each adapter slot under the live scales of `gm.ip_adapter` (optimizers/insert_ip_adapter.py,
    ip_adapter.py); the same cost per site as regions; not with `regions` or `fp8`.  `seg_layers` (addition, off by default,
    likewise): regular expressions selecting the self-attention sites whose perturbed batch entries take blurred queries (smoothed
    energy guidance; optimizers/insert_seg.py, seg.py); the state, `gm.seg`, starts with chunks 0 = ordinary attention; not with
    `pag_layers` (both claim the perturbed row block, and a site carries one leaf).  `t2i_adapter=True` (addition, off by default,
    likewise): a residual site behind every down block and the middle block (optimizers/insert_t2i_adapter.py, t2i_adapter.py); the
    state, `gm.t2i_adapter`, starts at scale 0 = the bits of the module without sites; not with `fp8`.  `controlnet=True` (addition,
    off by default, likewise): one leaf behind the middle block that adds a ControlNet's residuals to the skip tensors and the middle
    block's output, for the decoder's readers only (optimizers/insert_controlnet.py, controlnet.py); the state, `gm.controlnet`,
    starts at scale 0 = the bits of the module without sites; not with `t2i_adapter` or `fp8`.  `reference_layers` (addition, off by
    default, likewise): regular expressions selecting the self-attention sites whose leading batch entries also attend to the keys
    of the call's last B // chunks entries, the reference rows (reference-only control; optimizers/insert_reference.py,
    reference.py); the state, `gm.reference`, starts with chunks 0 = ordinary attention; not with `pag_layers` or `seg_layers` (a
    site carries one leaf)."""
    check_feature_combination(fp8, regions, ip_adapter, pag_layers, seg_layers, t2i_adapter, controlnet, reference_layers)
    if not isinstance(gm, fx.GraphModule):
        gm = fx.symbolic_trace(gm)
    stats: Dict[str, int] = {}
    if t2i_adapter:      # first of all: module paths are readable, and FreeU's sites then read skips that carry the residual
        stats["t2i_adapter_sites"] = insert_t2i_adapter(gm)
    if controlnet:       # likewise first (never both): FreeU's sites then read the leaf's outputs
        stats["controlnet_sites"] = insert_controlnet(gm)
    if freeu:      # first: the readers of a concatenation still carry their module paths
        stats["freeu_sites"] = insert_freeu(gm)
    stats["dropout"] = remove_dropout(gm)
    if fuse:
        stats["deduped_activations"] = dedupe_pure_calls(gm)
    stats["attention"] = fuse_attention(gm)
    if pag_layers is not None:      # directly after: the query projections still carry their module paths
        stats["pag_sites"] = insert_pag(gm, pag_layers)
    if seg_layers is not None:      # likewise (never both: check_feature_combination)
        stats["seg_sites"] = insert_seg(gm, seg_layers)
    if reference_layers is not None:      # likewise (never with either: check_feature_combination)
        stats["reference_sites"] = insert_reference(gm, reference_layers)
    if regions is not None:         # likewise
        stats["region_sites"] = insert_regions(gm, regions, region_tokens)
    if ip_adapter is not None:      # likewise
        stats["ip_adapter_sites"] = insert_ip_adapter(gm, ip_adapter)
    stats["geglu"] = fuse_geglu(gm)
    stats["linear_silu"] = replace_linear_activ(gm, nn.SiLU())
    stats["group_norm_silu"] = replace_group_norm_activation(gm, nn.SiLU())
    stats["group_norm"] = replace_group_norm(gm)
    stats["layer_norm"] = replace_layer_norm(gm)
    stats["linear"] = replace_linear(gm)
    stats["timesteps"] = fuse_timesteps(gm)
    stats["conv"] = replace_conv(gm)
    if fuse:
        stats["geglu_in_gemm"] = fuse_geglu_into_linear(gm)
        stats["temb_rowbias"] = fuse_temb_add(gm)
        stats["residual_adds"] = fuse_residual_adds(gm)
        stats["token_residuals"] = fuse_token_residual(gm)
        stats["shared_input_gemms"] = fuse_shared_input_linears(gm)
        stats["layer_norm_in_gemm"] = fuse_layernorm_into_linear(gm)
        stats["query_projection_in_attention"] = fuse_query_projection_into_attention(gm) if xattn_fusion else 0
        stats["group_norm_stats"] = fuse_groupnorm_stats(gm) if gn_stats else 0
        stats["skip_cats_removed"] = fuse_skip_cat(gm) if gn_stats else 0      # (the decoder's torch.cat: both readers take the two halves)
        if fp8:      # the three big projections of every transformer block on the fp8 matrix pipe, fed by e4m3 copies their
            stats["fp8_plan"] = plan_fp8(gm)      # producers' epilogues leave (no quantisation launches): optimizers/plan_fp8.py
    stats["channels_last_views"] = keep_channels_last(gm)
    gm.graph.eliminate_dead_code()
    gm.graph.lint()
    gm.recompile()
    gm.rewrite_stats = stats
    return gm


def check_feature_combination(fp8, regions, ip_adapter, pag_layers, seg_layers, t2i_adapter, controlnet=False, reference_layers=None) -> None:
    """The compile flags that exclude each other."""
    if reference_layers is not None and (pag_layers is not None or seg_layers is not None):
        raise ValueError("reference_layers cannot be combined with pag_layers or seg_layers: a self-attention site carries one leaf")
    if seg_layers is not None and pag_layers is not None:
        raise ValueError("seg_layers cannot be combined with pag_layers: smoothed energy guidance and perturbed-attention guidance both "
                         "claim the perturbed row block of a call, and a self-attention site carries one leaf")
    if regions is not None and fp8:
        raise ValueError("regions=R cannot be combined with fp8=True: the fp8 plan does not cover regional cross-attention sites")
    check_combination(ip_adapter, regions, fp8)
    _t2i.check_combination(t2i_adapter, fp8)
    _controlnet.check_combination(controlnet, t2i_adapter, fp8)


def run_compiler(gm: fx.GraphModule) -> fx.GraphModule:
    return replace_backend(gm)


def optimize_model(model: nn.Module, cuda_graph: bool = True, fuse: bool = True, fp8: bool = False, freeu: bool = False,
                   pag_layers=None, regions=None, region_tokens: int = 77, ip_adapter=None, seg_layers=None,
                   t2i_adapter: bool = False, controlnet: bool = False, reference_layers=None) -> fx.GraphModule:
    """`reference_layers=(".*",)` (addition): reference-only control (reference.py).  The selected self-attention sites can treat the
    last B // chunks batch entries of a call as reference rows: every other entry attends to its own tokens and to its reference
    row's tokens under one softmax (one launch, csrc/attention_joint.hip).  `gm.reference.using(chunks, step=..., table=...)` around the
    caller's own calls, `step` / `table` an optional device gate read at every launch; chunks 0, the initial state, is ordinary
    attention.  Not with `pag_layers` or `seg_layers`.
    `controlnet=True` (addition): ControlNet structural control (controlnet.py).  One launch behind the middle block adds the
    residuals of a ControlNet branch to the UNet's skip tensors and to the middle block's output, in place, for the decoder's readers
    only, and rewrites the producers' GroupNorm partials.  `gm.controlnet` - `bind(rows, latent_hw, device)` once, then
    `set(residuals, scale)`, `set_scale(scale)`, `set_site_weights(weights)`, `clear()` in place, no new capture;
    `using(step, table, residuals=...)` around the caller's own calls for per-step scales and residuals that are new every step;
    scale 0, the state after `bind`, writes nothing: the bits of the module compiled without sites.  `controlnet.ControlNetXL` is the
    branch network; `optimize_model(ControlNetXL(...), cuda_graph=False)` compiles it.  Not with `t2i_adapter=True` or `fp8=True`.
    `t2i_adapter=True` (addition): T2I-Adapter structural control (t2i_adapter.py).  The UNet adds `s * f_k` to its activation
    behind every down block and the middle block (diffusers' `down_intrablock_additional_residuals` places), in place, in one launch
    per site that also rewrites the producer's GroupNorm partials.  `gm.t2i_adapter` - `bind(rows, latent_hw, device)` once, then
    `set(features, scale)`, `set_scale(scale)`, `clear()` in place, no new capture; `using(step, table)` around the caller's own
    calls for per-step scales; scale 0, the state after `bind`, writes nothing: the bits of the module compiled without sites.
    `t2i_adapter.FullAdapterXL` turns a control image into the features.  Not with `fp8=True`.  (With `cuda_graph=True` a captured
    call keeps reading the table and counter it was captured with - the state's own, outside `using` -, and `bind` must precede the
    first call; DenoiseLoop and the hooks capture their own graphs over a `cuda_graph=False` module.)
    `seg_layers=("mid",)` (addition): smoothed energy guidance (seg.py).  The selected self-attention sites can treat the last
    B // chunks batch entries of a call as perturbed: their queries are Gaussian-blurred over the latent grid (sigma = infinity: the
    spatial mean).  `gm.seg.bind(latent_hw, device)` once per latent size, `gm.seg.using(chunks, latent_hw)` around the caller's own
    calls, `gm.seg.set_sigma(sigma)` in place, no new capture; chunks 0, the initial state, is ordinary attention.  Not with
    `pag_layers`.
    `ip_adapter=N` (addition; 4: base adapters, 16: plus; a tuple of up to 4 counts for several adapters): IP-Adapter image prompts
    (ip_adapter.py).  Every cross-attention adds s * Attn(q, K_img, V_img) per adapter slot, in the same launch.  `gm.ip_adapter` -
    `bind(rows, latent_hw, device)` once, then `load(state_dict, slot)`, `set_image(tokens, ...)`, `set_scale(scale, slot)`,
    `set_masks(masks, slot)`, `unload(slot)`, all in place, no new capture; a slot at scale 0 (the state after `bind`) is skipped:
    the bits of the module compiled without it.  Not with `regions` or `fp8=True`.
    `regions=R` (addition): regional prompts (regions.py).  The text context is R prompts of `region_tokens` tokens concatenated
    along the token axis; every cross-attention gives each its own softmax and combines them per latent cell with the weights of
    `gm.regions` - `bind(rows, latent_hw, device)` once, then `set(masks, positive_rows)` / `clear()` in place, no new capture;
    after `bind` the state is "off": the bits of the module compiled without it on the first prompt.  Not with `fp8=True`.
    `pag_layers=("mid",)` (addition): the selected self-attention sites can treat the last B // chunks batch entries of a call as
    perturbed (perturbed-attention guidance, pag.py): `gm.pag.using(chunks)` around the caller's own calls; chunks 0, the initial
    state, is ordinary attention.
    `freeu=True` (addition): the compiled module carries FreeU sites and `gm.freeu`, their parameter state, neutral until
    `gm.freeu.set(s1, s2, b1, b2, version)` (freeu.py; in-place, no new capture).
    `fp8=True` (addition, BASELINE config #5): the q|k|v, GEGLU and feed-forward output projections of a bf16 model's
    transformer blocks run with OCP e4m3 operands on the fp8 matrix pipe, fed by e4m3 copies their producers' epilogues
    leave under delayed per-tensor scales (optimizers/plan_fp8.py); everything else is unchanged."""
    # same preconditions as the reference (optimization.py:29-33), for ROCm
    assert torch.cuda.is_available(), "a ROCm GPU is required to use stabletriton_amd"
    major, _ = torch.cuda.get_device_capability()
    if major < 9:
        raise RuntimeError("a CDNA GPU (gfx9xx; built and tuned for gfx950 / MI355X) is required")
    p0 = next(model.parameters())
    assert p0.device.type == "cuda", "Model must be on GPU"
    # fp16 is what the reference's call site passes (load_sdxl_pipeline.py:17-28: `.half().cuda()`); bf16 has the same
    # matrix-pipe rate and fp32's exponent range; fp32 is the strict parity mode
    if p0.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise RuntimeError(f"model dtype {p0.dtype} not supported: use float16 / bfloat16 (fast) or float32 (strict parity)")
    _C.load()                                  # fail now, loudly, if the HIP library is missing
    model = model.eval().to(memory_format=torch.channels_last)      # conv weights -> (Cout,R,S,Cin) strides
    if fp8 and p0.dtype != torch.bfloat16:
        raise RuntimeError("fp8 projections need a bfloat16 model")
    gm = replace_backend(model, fuse=fuse, fp8=fp8, freeu=freeu, pag_layers=pag_layers, regions=regions,
                         region_tokens=region_tokens, ip_adapter=ip_adapter, seg_layers=seg_layers, t2i_adapter=t2i_adapter,
                         controlnet=controlnet, reference_layers=reference_layers)
    # the compiled module owns its mutable host state (split-K workspace, next-weights plan, derived weight buffers):
    # two compiled modules, or two streams each driving their own, never share any (ops.ExecContext)
    gm.exec_context = ops.ExecContext()
    gm.fp8_plan = bool(fp8 and fuse)
    if isinstance(model, _controlnet.ControlNetXL):
        # a ControlNet branch: its control-image embedding is no part of forward, so the trace drops it; the compiled module keeps the
        # eager module's bound method (DenoiseLoop.set_controlnet embeds an image through it).  Limitation: the embedding's weights stay
        # with the eager module - move / cast that module BEFORE compiling, a later .to() of the compiled branch leaves them behind
        gm.embed_condition = model.embed_condition
    # the host's tables of the sinusoidal timestep features (ops._timestep_table): built now, eagerly, so that no first call
    # inside somebody's stream capture has to compute them the other way
    from .optimizers.wrappers import timestep_embedding_wrapper
    for n in gm.graph.nodes:
        if n.op == "call_function" and n.target is timestep_embedding_wrapper and isinstance(n.args[1], int):
            ops._timestep_table(p0.device, n.args[1])
    if not (fuse and _install_context_split(gm)):
        plain = gm.forward

        def forward(*args, **kwargs):
            return _run_step(gm, lambda: plain(*args, **kwargs))

        gm.forward = forward
    if cuda_graph and (pag_layers is not None or seg_layers is not None):
        # the perturbed range - and for SEG the call's latent size, the sites' token grids - is host state the launches are captured
        # with: it is part of the graph cache's key
        state, inner = (gm.pag if pag_layers is not None else gm.seg), gm.forward

        def run_perturbed(*args, _chunks: int = 0, _latent=None, **kwargs):
            with state.using(_chunks, _latent):
                return inner(*args, **kwargs)

        graphed = make_dynamic_graphed_callable(run_perturbed, before_replay=gm.exec_context.refresh_derived)

        def perturbed_forward(*args, **kwargs):
            latent = state.latent_hw if seg_layers is not None and state.chunks else None
            if latent is not None:      # SEG's rows are allocated outside the capture the cache may start
                sample = args[0] if args else kwargs["sample"]
                state.bind(latent, sample.device)
            return graphed(*args, _chunks=state.chunks, _latent=latent, **kwargs)

        gm.forward = perturbed_forward
    elif cuda_graph and reference_layers is not None:
        # likewise: the reference range is host state of the captured launches; the gate is the state's own pair (the caller's
        # `using(chunks, step=, table=)` tensors would be captured by address: pass none with cuda_graph=True)
        ref_state, ref_inner = gm.reference, gm.forward

        def run_reference(*args, _chunks: int = 0, **kwargs):
            with ref_state.using(_chunks):
                return ref_inner(*args, **kwargs)

        ref_graphed = make_dynamic_graphed_callable(run_reference, before_replay=gm.exec_context.refresh_derived)

        def reference_forward(*args, **kwargs):
            if ref_state.gate is not None:
                raise ValueError("reference: a module compiled with cuda_graph=True runs under the state's own gate; compile with "
                                 "cuda_graph=False to pass step= / table= to using()")
            if ref_state.chunks:      # allocated outside the capture the cache may start
                sample = args[0] if args else kwargs["sample"]
                ref_state.own_gate(sample.device)
            return ref_graphed(*args, _chunks=ref_state.chunks, **kwargs)

        gm.forward = reference_forward
    elif cuda_graph:
        gm.forward = make_dynamic_graphed_callable(gm.forward, before_replay=gm.exec_context.refresh_derived)
    return gm


def _run_step(gm: fx.GraphModule, core):
    """One UNet evaluation inside the module's step scope.  With the fp8 plan: the launch that turns the previous step's
    maxima into this step's scales goes first; the very first evaluation runs twice (its first pass only measures)."""
    ectx = gm.exec_context
    with ectx.step():
        if not getattr(gm, "fp8_plan", False):
            return core()
        if ectx.fp8 is None or not ectx.fp8.calibrated:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("fp8 plan: run one eager step before capturing (DenoiseLoop.capture and the graph cache do)")
            out = core()                             # measuring pass: e4m3 copies under the initial scales, true maxima recorded
            if ectx.plan is not None:
                ectx.plan.reset()
            if ectx.fp8 is None:                     # nothing in this module qualified for the plan
                gm.fp8_plan = False
                return out
            ectx.fp8.calibrated = True
    with ectx.step():
        ectx.fp8.update()
        return core()


FP8_CALIBRATION_PASSES = 2      # measuring evaluations after a reset: the first runs under the initial scale (values beyond 28 clip,
                                # so what it records downstream of a clipped tensor is too small), the second under scales from the first


def recalibrate_fp8(gm, run_once) -> bool:
    """Start the delayed scales of `gm`'s fp8 plan over and measure them on the evaluation `run_once()` performs (eagerly,
    outside any capture; its result is discarded): after this the scales are a function of that evaluation's inputs alone,
    so two identical trajectories give identical results whatever ran before.  Returns False when there is nothing to do."""
    ectx = getattr(gm, "exec_context", None)
    if ectx is None or not getattr(gm, "fp8_plan", False) or ectx.fp8 is None:
        return False
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("fp8 plan: the scales cannot be re-measured inside a graph capture")
    ectx.fp8.reset()
    with torch.no_grad():
        for _ in range(FP8_CALIBRATION_PASSES):
            ectx.fp8.calibrated = False            # _run_step: one measuring pass, the scale update, one pass under the new scales
            run_once()
    return True


def _install_context_split(gm: fx.GraphModule) -> bool:
    """Hoist the text-context projections (step-invariant) out of the per-step graph.

    `gm(sample, timesteps, encoder_hidden_states, added_cond_kwargs)` keeps working and stays
    stateless (it evaluates the context part on every call).  Loops that reuse one prompt call
    `ctx = gm.precompute_context(ehs)` once and `gm.forward_with_context(sample, t, ctx, cond)`
    per step (stabletriton_amd/pipeline.py)."""
    names = [n.target for n in gm.graph.nodes if n.op == "placeholder"]
    if "encoder_hidden_states" not in names:
        return False
    context_module = split_context(gm, "encoder_hidden_states")
    if context_module is None:
        return False
    if getattr(gm, "exec_context", None) is None:
        gm.exec_context = ops.ExecContext()
    ectx = gm.exec_context
    gm.rewrite_stats["context_outputs"] = len(
        [n for n in context_module.graph.nodes if n.op == "output"][0].args[0])
    gm.context_module = context_module
    # The time path (sinusoidal features -> TimestepEmbedding MLPs -> the batched resnet time_emb_proj)
    # depends only on the timestep and the added conditioning: a loop evaluates it once per schedule
    # entry and feeds the per-step row back in (pipeline.DenoiseLoop).
    time_module = None
    cond_arg = "added_cond_kwargs" if "added_cond_kwargs" in names else ("y" if "y" in names else None)
    if "timesteps" in names and cond_arg is not None:
        time_module = split_region(gm, ("timesteps", cond_arg), "time_cache", meta_sources=("sample",),
                                   stop_at_slices=True, class_name="TimeModule")
    core = gm.forward     # generated: (sample, timesteps, ehs, context_cache, added_cond_kwargs[, time_cache], **kw)

    def precompute_context(encoder_hidden_states):
        with ectx:
            return context_module(encoder_hidden_states)

    if time_module is None:
        def forward_with_context(sample, timesteps, context_cache, added_cond_kwargs, **kwargs):
            return _run_step(gm, lambda: core(sample, timesteps, None, context_cache, added_cond_kwargs, **kwargs))
    else:
        gm.time_module = time_module
        gm.rewrite_stats["time_outputs"] = len([n for n in time_module.graph.nodes if n.op == "output"][0].args[0])

        def precompute_time(sample, timesteps, added_cond_kwargs):
            """Time-path tensors of one schedule entry (`sample` is read for its batch size and dtype only)."""
            with ectx:
                return time_module(sample, timesteps, added_cond_kwargs)

        def forward_with_context(sample, timesteps, context_cache, added_cond_kwargs, time_cache=None, **kwargs):
            if time_cache is None:
                time_cache = precompute_time(sample, timesteps, added_cond_kwargs)
            # one pass over the same GEMMs in the same order: each launch warms the next one's weights
            return _run_step(gm, lambda: core(sample, timesteps, None, context_cache, added_cond_kwargs, time_cache, **kwargs))

        gm.precompute_time = precompute_time

    def forward(sample, timesteps, encoder_hidden_states, added_cond_kwargs, **kwargs):
        ctx = precompute_context(encoder_hidden_states)      # (outside the per-step weight plan: a loop evaluates it once)
        return forward_with_context(sample, timesteps, ctx, added_cond_kwargs, **kwargs)

    gm.precompute_context = precompute_context
    gm.forward_with_context = forward_with_context
    gm.forward = forward
    return True


compile = optimize_model
