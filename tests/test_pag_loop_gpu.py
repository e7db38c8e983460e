"""Perturbed-attention guidance in the captured denoise loop and behind the hooks, on the TINY network, and one SDXL-base
strict step against the CPU fixture (tools/make_pag_golden.py).

The reference is the tests' own: the eager module in float64 on the CPU with forward hooks on the selected attn1 modules and a
float64 restatement of the three-way guidance around each sampler (tests/pag_util.py).  Euler 10 steps, g = 5, s = 3 unless
stated; rows [negative | positive | perturbed] from synth.denoise_inputs(2, 16, 1234): row 0 the negative prompt, row 1 the
prompt, row 0's noise."""
import functools

import pytest
import torch

from stabletriton_amd import hooks, pag, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import pag_util as PU
from tests.util import golden

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
G, S = 5.0, 3.0
LAYERS = ("mid",)


def _model(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


@functools.lru_cache(maxsize=None)
def _model64():
    """The same weights (synth.fill_module_ is a function of the names and the seed) in float64 on the CPU."""
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double()


@functools.lru_cache(maxsize=None)
def _inputs(rows=2):
    return synth.denoise_inputs(rows, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _compiled(dtype, fp8=False):
    return optimize_model(_model(dtype, torch.device("cuda:0")), cuda_graph=False, fp8=fp8, pag_layers=LAYERS)


TABLES = {"euler": lambda: euler_discrete_tables(10), "dpmpp_karras": lambda: dpmpp_2m_tables(10, karras=True),
          "dpmpp_sde": lambda: dpmpp_2m_sde_tables(10)}


@functools.lru_cache(maxsize=None)
def _ref(sampler="euler", s=S, g=G, phi=None, seed=None):
    """float64 hooked loop, computed once per configuration: (final latent, |e_pos - e_pert| max at step 0)."""
    return PU.loop64(_model64(), _inputs(), TABLES[sampler](), s, g=g, phi=phi, seed=seed, layers=LAYERS)


def _loop(gm, dtype, dev, mode="loop", tables=None, batch=1, x=None, pos=slice(1, 2), neg=slice(0, 1), **kw):
    x = x or _inputs()
    loop = DenoiseLoop(gm, batch, 16, dtype, dev, tables or TABLES["euler"](), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim,
                       mode=mode, **kw)
    rows = lambda k, r: x[k][r].to(dev, dtype)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    if kw.get("guidance_scale") is None:
        loop.set_conditioning(*(rows(k, pos) for k in keys))
    else:
        loop.set_conditioning(*(rows(k, pos) for k in keys), *(rows(k, neg) for k in keys))
    return loop


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ modes
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_modes_agree_and_fp32_matches_the_float64_hooked_loop(gpu, dtype):
    gm = _compiled(dtype)
    assert gm.rewrite_stats["pag_sites"] == 2
    noise = _inputs()["latent"][:1]
    finals = {}
    with torch.no_grad():
        for mode in ("eager", "step", "loop"):
            loop = _loop(gm, dtype, gpu, mode, guidance_scale=G, pag_scale=S)
            assert loop.x_in.shape[0] == 3 and loop.ehs.shape[0] == 3
            finals[mode] = loop.denoise(noise).cpu()
            assert torch.equal(finals[mode], loop.denoise(noise).cpu()), f"{mode}: a replay must repeat its bits"
            assert gm.pag.chunks == 0, "the loop names the perturbed block around its own calls only"
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    assert torch.isfinite(finals["loop"]).all()
    if dtype == torch.float32:
        ref, gap0 = _ref()
        plain, _ = _ref(s=None)
        moved = float((ref - plain).abs().max())
        err = _err(finals["loop"], ref)
        print(f"tiny CFG + PAG 10-step loop fp32: max abs err vs the float64 hooked loop {err:.2e}; PAG moves the float64 result by "
              f"{moved:.2f}; the perturbed prediction is {gap0:.2f} from the positive one at step 0")
        assert moved > 100 * ABS_TOL_STRICT, "PAG must matter for this check to mean anything"
        assert err <= ABS_TOL_STRICT


@pytest.mark.parametrize("config", ["pag_alone", "cfg_rescale", "dpmpp_karras", "dpmpp_sde"])
def test_fp32_configurations_match_the_float64_hooked_loop(gpu, config):
    gm = _compiled(torch.float32)
    noise = _inputs()["latent"][:1]
    sampler, kw, ref_kw, seed = "euler", dict(guidance_scale=G, pag_scale=S), {}, None
    if config == "pag_alone":
        kw, ref_kw = dict(pag_scale=S), dict(g=None)
    elif config == "cfg_rescale":
        kw["guidance_rescale"] = 0.7
        ref_kw = dict(phi=0.7)
    elif config == "dpmpp_karras":
        sampler = config
    else:
        sampler, seed = config, 77
        ref_kw = dict(seed=seed)
    with torch.no_grad():
        loop = _loop(gm, torch.float32, gpu, "loop", TABLES[sampler](), **kw)
        assert loop.x_in.shape[0] == (2 if config == "pag_alone" else 3)
        if seed is not None:
            loop.set_seed(seed)
        out = loop.denoise(noise).cpu()
        assert torch.equal(out, loop.denoise(noise).cpu())
    ref, _ = _ref(sampler, **ref_kw)
    err = _err(out, ref)
    print(f"tiny PAG {config} fp32: max abs err vs the float64 hooked loop {err:.2e}")
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ set_pag
def test_set_pag_needs_no_recapture(gpu):
    dtype = torch.float32
    gm = _compiled(dtype)
    noise = _inputs()["latent"][:1]
    tables = TABLES["euler"]()
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", guidance_scale=G, pag_scale=S)
        at3 = loop.denoise(noise).cpu()
        graph = loop.graph
        assert graph is not None
        loop.set_pag(1.0)
        at1 = loop.denoise(noise).cpu()
        assert loop.graph is graph and not torch.equal(at1, at3)
        loop.set_pag(S)
        assert torch.equal(loop.denoise(noise).cpu(), at3) and loop.graph is graph, "restoring the scale restores the bits"
        # a per-step table: diffusers' adaptive scale; 3 - 0.004 (1000 - t) reaches the clamp inside the schedule
        table = pag.adaptive_scales(tables.timesteps, S, 0.004)
        assert table[0] > 0.0 and table[-1] == 0.0 and len(set(table)) > 2
        loop.set_pag(table)
        adaptive = loop.denoise(noise).cpu()
        assert loop.graph is graph
    ref, _ = PU.loop64(_model64(), _inputs(), tables, [max(0.0, S - 0.004 * (1000.0 - float(t))) for t in tables.timesteps], g=G)
    err = _err(adaptive, ref)
    print(f"tiny CFG + adaptive PAG table fp32: max abs err vs the float64 hooked loop {err:.2e}")
    assert err <= ABS_TOL_STRICT
    with pytest.raises(ValueError, match="set_pag"):
        loop.set_pag([1.0, 2.0])


def test_pag_scale_zero_is_the_cfg_loop(gpu):
    """pag_scale = 0 keeps the 3B rows and gives the CFG value of e.  Against a 2B CFG loop of the same g it is within the strict
    gate, NOT bit-equal: the UNet's GEMM dispatch (tile configuration, split-K) depends on the row count, so the two
    loops' predictions differ in the last bits."""
    dtype = torch.float32
    gm = _compiled(dtype)
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        zero = _loop(gm, dtype, gpu, "loop", guidance_scale=G, pag_scale=0.0).denoise(noise).cpu()
        cfg = _loop(gm, dtype, gpu, "loop", guidance_scale=G).denoise(noise).cpu()
    diff = float((zero - cfg).abs().max())
    print(f"tiny pag_scale 0 (3B rows) vs the CFG loop (2B rows): max abs diff {diff:.2e}")
    assert diff <= ABS_TOL_STRICT
    assert _err(zero, _ref(s=None)[0]) <= ABS_TOL_STRICT


def test_batch_rows_match_their_single_runs(gpu):
    """B = 2, two prompts (negatives rows 0, 1; positives rows 2, 3): each row is its own B = 1 run."""
    dtype = torch.float32
    gm = _compiled(dtype)
    x = _inputs(4)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", batch=2, x=x, pos=slice(2, 4), neg=slice(0, 2), guidance_scale=G, pag_scale=S)
        assert loop.x_in.shape[0] == 6
        both = loop.denoise(x["latent"][:2]).cpu()
        for k in range(2):
            one = _loop(gm, dtype, gpu, "loop", x=x, pos=slice(2 + k, 3 + k), neg=slice(k, k + 1), guidance_scale=G, pag_scale=S)
            single = one.denoise(x["latent"][k:k + 1]).cpu()
            err = float((both[k:k + 1] - single).abs().max())
            print(f"tiny CFG + PAG B=2 row {k} vs its B=1 run: max abs diff {err:.2e}")
            assert err <= ABS_TOL_STRICT
    assert not torch.equal(both[0], both[1])


def test_error_cases(gpu):
    dtype = torch.float32
    gm = _compiled(dtype)
    with pytest.raises(ValueError, match="pag_scale"):
        _loop(gm, dtype, gpu, "eager", guidance_scale=G).set_pag(1.0)
    plain = optimize_model(_model(dtype, gpu), cuda_graph=False)
    with pytest.raises(ValueError, match="pag_layers"):
        _loop(plain, dtype, gpu, "eager", guidance_scale=G, pag_scale=S)
    with pytest.raises(ValueError, match="guidance_rescale needs guidance_scale"):
        _loop(gm, dtype, gpu, "eager", pag_scale=S, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="negative conditioning"):
        _loop(gm, dtype, gpu, "eager", pag_scale=S).set_conditioning(*(_inputs()[k][1:2].to(gpu) for k in ("encoder_hidden_states", "text_embeds", "time_ids")),
                                                                     negative_text_embeds=_inputs()["text_embeds"][:1].to(gpu))
    with pytest.raises(ValueError, match="pag_layers"):
        optimize_model(_model(dtype, gpu), cuda_graph=False, pag_layers=("nowhere",))


def test_set_image_lora_and_freeu_keep_working(gpu):
    """PAG touches none of their state: img2img start in mode step, a LoRA-free weight refresh, FreeU sites beside PAG sites."""
    dtype = torch.bfloat16
    gm = optimize_model(_model(dtype, gpu), cuda_graph=False, pag_layers=LAYERS, freeu=True)
    assert gm.rewrite_stats["pag_sites"] == 2 and gm.rewrite_stats["freeu_sites"] == 6
    x = _inputs()
    noise = x["latent"][:1]
    init = synth.normal("img2img.init", (1, 4, 16, 16), 77) * 0.8
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "step", guidance_scale=G, pag_scale=S)
        left = loop.set_image(init, noise, 0.5)
        assert left == 5
        loop.run_steps(left)
        a = loop.latent.clone()
        eager = _loop(gm, dtype, gpu, "eager", guidance_scale=G, pag_scale=S)
        eager.run_steps(eager.set_image(init, noise, 0.5))
        assert torch.equal(a, eager.latent) and torch.isfinite(a).all()
        base = loop.denoise(noise)
        loop.set_freeu(0.9, 0.2, 1.3, 1.4)
        on = loop.denoise(noise)
        assert not torch.equal(on, base) and torch.isfinite(on).all()
        loop.set_freeu(None)
        assert loop.refresh_weights() >= 0
        assert torch.equal(loop.denoise(noise), base)


def test_fp8_plan_with_pag_runs_and_repeats(gpu):
    """A smoke check: the fp8 plan fires on the perturbed sites' projections as everywhere else; finite, and a replay repeats."""
    dtype = torch.bfloat16
    gm = _compiled(dtype, fp8=True)
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "step", euler_discrete_tables(8), guidance_scale=G, pag_scale=S)
        first = loop.denoise(noise).cpu()
        again = loop.denoise(noise).cpu()
    assert gm.exec_context.fp8 is not None and gm.exec_context.fp8.sites
    assert torch.isfinite(first).all() and torch.equal(first, again)


# ------------------------------------------------------------------------------------------------ hooks
def test_diffusers_hook_enable_and_disable(gpu):
    dtype = torch.float32
    m = _model(dtype, gpu)
    x = PU.three_rows(16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], cross_attention_kwargs=None,
                       added_cond_kwargs=cond, return_dict=False)[0].clone()
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu, pag_layers=LAYERS)
    base = call(unet)
    assert torch.equal(base, call(unet))                       # (the second call replays the captured graph)
    step_fn = next(iter(unet._steps.values()))
    assert len(step_fn._cached) == 1
    unet.enable_pag(3)
    on = call(unet)
    assert len(step_fn._cached) == 2, "another chunks value is another cache entry, not a replay of the wrong graph"
    assert torch.equal(on, call(unet)) and len(step_fn._cached) == 2
    # (the unperturbed rows: the attention launch of a site now sees a sub-batch, so the strict gate, not bits)
    assert float((on[:2] - base[:2]).abs().max()) <= ABS_TOL_STRICT and float((on[2] - base[2]).abs().max()) > 10 * ABS_TOL_STRICT
    m64 = _model64()
    xi = {k: v.double() for k, v in x.items()}

    def ref(chunks):
        with torch.no_grad(), PU.hooked(m64, LAYERS, chunks):
            return m64(xi["latent"], torch.tensor(300.0), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]

    err = _err(on, ref(3))
    print(f"diffusers hook, tiny fp32, enable_pag(3): max abs err vs the hooked float64 module {err:.2e}")
    assert err <= ABS_TOL_STRICT
    unet.enable_pag(1)                                          # a fully perturbed call (ComfyUI's node makes one)
    assert _err(call(unet), ref(1)) <= ABS_TOL_STRICT and len(step_fn._cached) == 3
    unet.disable_pag()
    off = call(unet)
    assert torch.equal(off, base) and len(step_fn._cached) == 3
    assert _err(off, ref(0)) <= ABS_TOL_STRICT
    with pytest.raises(ValueError, match="chunks"):
        unet.enable_pag(0)
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    with pytest.raises(ValueError, match="pag_layers"):
        plain.enable_pag(3)
    with pytest.raises(ValueError, match="pag_layers"):
        plain.disable_pag()


def test_comfy_hook_fully_perturbed_call(gpu):
    dtype = torch.float32
    m = _model(dtype, gpu)
    adapter = hooks.compile_comfy_unet(m, pag_layers=LAYERS)
    assert adapter.compiled.rewrite_stats["pag_sites"] == 2
    x = _inputs()
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    with torch.no_grad():
        y = torch.cat([xg["text_embeds"], m.add_time_proj(xg["time_ids"].flatten()).reshape(2, -1).to(dtype)], dim=-1)
    call = lambda a: a(xg["latent"], timesteps=torch.full((2,), 300.0, device=gpu), context=xg["encoder_hidden_states"], y=y).clone()
    base = call(adapter)
    adapter.enable_pag(1)
    on = call(adapter)
    assert not torch.equal(on, base) and torch.equal(on, call(adapter))
    m64 = _model64()
    xi = {k: v.double() for k, v in x.items()}
    with torch.no_grad(), PU.hooked(m64, LAYERS, 1):
        ref = m64(xi["latent"], torch.tensor(300.0), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]
    assert _err(on, ref) <= ABS_TOL_STRICT
    adapter.disable_pag()
    assert torch.equal(call(adapter), base)


def test_graphed_module_keys_its_cache_on_chunks(gpu):
    """optimize_model(cuda_graph=True): the module's own graph cache takes `chunks` into its key."""
    dtype = torch.float32
    gm = optimize_model(_model(dtype, gpu), cuda_graph=True, pag_layers=LAYERS)
    x = PU.three_rows(16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    args = (x["latent"].to(gpu), torch.tensor(500.0, device=gpu), x["encoder_hidden_states"].to(gpu),
            {"text_embeds": x["text_embeds"].to(gpu), "time_ids": x["time_ids"].to(gpu)})
    with torch.no_grad():
        base = gm(*args)[0].clone()
        with gm.pag.using(3):
            on = gm(*args)[0].clone()
            assert torch.equal(on, gm(*args)[0])
        assert torch.equal(gm(*args)[0], base)
    assert float((on[:2] - base[:2]).abs().max()) <= ABS_TOL_STRICT and float((on[2] - base[2]).abs().max()) > 10 * ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ SDXL-base, one strict step
def test_sdxl_strict_step_with_pag_vs_cpu_fixture(gpu, sdxl_fp32_pair):
    """SDXL-base fp32 at latent 64, rows [negative | positive | perturbed], sites ("mid",), against
    tests/golden/f1_unet_step_latent64_pag.npz (the eager fp32 module with the tests' hooks on the CPU, tools/make_pag_golden.py;
    its own deviation from a float64 run is in the file)."""
    g = golden("f1_unet_step_latent64_pag")
    ref = torch.from_numpy(g["out"])
    gm = optimize_model(sdxl_fp32_pair[0], cuda_graph=False, pag_layers=LAYERS)
    assert gm.rewrite_stats["pag_sites"] == 10 == int(g["sites"])
    x = PU.three_rows(int(g["latent_hw"]), 1234)
    xg = {k: v.to(gpu) for k, v in x.items()}
    with torch.no_grad(), gm.pag.using(int(g["chunks"])):
        out = gm(xg["latent"], torch.tensor(float(g["timestep"]), device=gpu), xg["encoder_hidden_states"],
                 {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0].float().cpu()
    err = float((out - ref).abs().max())
    gap = float(g["pert_vs_pos_max_abs"])
    print(f"SDXL strict step with PAG: max abs err {err:.2e} (|ref| max {float(ref.abs().max()):.2f}; the perturbed row is {gap:.2e} from "
          f"the positive one; fixture vs float64 {float(g['f64_max_abs_dev']) if 'f64_max_abs_dev' in g.files else float('nan'):.2e})")
    assert gap > 100 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT
