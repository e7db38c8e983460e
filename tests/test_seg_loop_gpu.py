"""Smoothed energy guidance in the captured denoise loop and behind the hooks, on the TINY network, and one SDXL-base strict step
against the CPU fixture (tools/make_seg_golden.py).

The reference is the tests' own: the eager module in float64 on the CPU with forward hooks on the selected attn1 modules that
recompute the perturbed rows with blurred queries, and a float64 restatement of the three-way guidance around each sampler
(tests/seg_util.py on tests/pag_util.py's sampler rows).  Euler 10 steps, g = 5, s = 3 unless stated; rows
[negative | positive | perturbed] from synth.denoise_inputs(2, hw, 1234): row 0 the negative prompt, row 1 the prompt, row 0's noise.
Latent 16 and 24 x 16, sites ("mid",) and ("down_blocks.1", "mid"), sigma 1 and infinity: all eight with CFG under Euler in the three
modes; without CFG, with rescale and under the two DPM++ samplers on the two opposite corners of that cube."""
import functools
import itertools

import pytest
import torch

from stabletriton_amd import hooks, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import pag_util as PU
from tests import seg_util as SU
from tests.util import golden

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
G, S = 5.0, 3.0
INF = float("inf")
MID, BOTH = ("mid",), ("down_blocks.1", "mid")
CUBE = list(itertools.product([(16, 16), (24, 16)], [MID, BOTH], [1.0, INF]))
CORNERS = [((16, 16), MID, INF), ((24, 16), BOTH, 1.0)]
_id = lambda c: f"{c[0][0]}x{c[0][1]}-{'+'.join(c[1])}-sigma{c[2]}"


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
def _inputs(rows=2, hw=(16, 16)):
    return synth.denoise_inputs(rows, hw, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _compiled(dtype, layers=MID, fp8=False):
    return optimize_model(_model(dtype, torch.device("cuda:0")), cuda_graph=False, fp8=fp8, seg_layers=layers)


TABLES = {"euler": lambda: euler_discrete_tables(10), "dpmpp_karras": lambda: dpmpp_2m_tables(10, karras=True),
          "dpmpp_sde": lambda: dpmpp_2m_sde_tables(10)}


@functools.lru_cache(maxsize=None)
def _ref(hw=(16, 16), layers=MID, sigma=INF, sampler="euler", s=S, g=G, phi=None, seed=None):
    """float64 hooked loop, computed once per configuration: (final latent, |e_pos - e_pert| max at step 0)."""
    if s is None:
        return PU.loop64(_model64(), _inputs(2, hw), TABLES[sampler](), None, g=g, phi=phi, seed=seed)
    return SU.loop64(_model64(), _inputs(2, hw), TABLES[sampler](), s, sigma, hw, g=g, phi=phi, seed=seed, layers=layers)


def _loop(gm, dtype, dev, mode="loop", tables=None, batch=1, x=None, hw=(16, 16), pos=slice(1, 2), neg=slice(0, 1), **kw):
    x = x or _inputs(2, hw)
    loop = DenoiseLoop(gm, batch, hw, dtype, dev, tables or TABLES["euler"](), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim,
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
@pytest.mark.parametrize("case", CUBE, ids=_id)
def test_fp32_modes_agree_and_match_the_float64_hooked_loop(gpu, case):
    hw, layers, sigma = case
    gm = _compiled(torch.float32, layers)
    assert gm.rewrite_stats["seg_sites"] == len(layers) * 2
    noise = _inputs(2, hw)["latent"][:1]
    finals = {}
    with torch.no_grad():
        for mode in ("eager", "step", "loop"):
            loop = _loop(gm, torch.float32, gpu, mode, hw=hw, guidance_scale=G, seg_scale=S, seg_sigma=sigma)
            assert loop.x_in.shape[0] == 3 and loop.ehs.shape[0] == 3
            finals[mode] = loop.denoise(noise).cpu()
            assert torch.equal(finals[mode], loop.denoise(noise).cpu()), f"{mode}: a replay must repeat its bits"
            assert gm.seg.chunks == 0 and gm.seg.latent_hw is None, "the loop names the perturbed block around its own calls only"
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    ref, gap0 = _ref(hw, layers, sigma)
    plain, _ = _ref(hw, s=None)
    moved = float((ref - plain).abs().max())
    err = _err(finals["loop"], ref)
    print(f"tiny CFG + SEG {_id(case)} fp32: max abs err vs the float64 hooked loop {err:.2e}; SEG moves the float64 result by "
          f"{moved:.2f}; the perturbed prediction is {gap0:.3f} from the positive one at step 0")
    assert moved > 100 * ABS_TOL_STRICT, "SEG must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


@pytest.mark.parametrize("case", CORNERS, ids=_id)
@pytest.mark.parametrize("config", ["seg_alone", "cfg_rescale", "dpmpp_karras", "dpmpp_sde"])
def test_fp32_configurations_match_the_float64_hooked_loop(gpu, config, case):
    hw, layers, sigma = case
    gm = _compiled(torch.float32, layers)
    noise = _inputs(2, hw)["latent"][:1]
    sampler, kw, ref_kw, seed = "euler", dict(guidance_scale=G, seg_scale=S, seg_sigma=sigma), {}, None
    if config == "seg_alone":
        kw, ref_kw = dict(seg_scale=S, seg_sigma=sigma), dict(g=None)
    elif config == "cfg_rescale":
        kw["guidance_rescale"] = 0.7
        ref_kw = dict(phi=0.7)
    elif config == "dpmpp_karras":
        sampler = config
    else:
        sampler, seed = config, 77
        ref_kw = dict(seed=seed)
    with torch.no_grad():
        loop = _loop(gm, torch.float32, gpu, "loop", TABLES[sampler](), hw=hw, **kw)
        assert loop.x_in.shape[0] == (2 if config == "seg_alone" else 3)
        if seed is not None:
            loop.set_seed(seed)
        out = loop.denoise(noise).cpu()
        assert torch.equal(out, loop.denoise(noise).cpu())
    ref, _ = _ref(hw, layers, sigma, sampler, **ref_kw)
    err = _err(out, ref)
    print(f"tiny SEG {config} {_id(case)} fp32: max abs err vs the float64 hooked loop {err:.2e}")
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ set_seg
def test_set_seg_needs_no_recapture(gpu):
    dtype = torch.float32
    gm = _compiled(dtype)
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", guidance_scale=G, seg_scale=S, seg_sigma=1.0)
        rows = {k: r.data_ptr() for k, r in gm.seg._rows.items()}
        at1 = loop.denoise(noise).cpu()
        graph = loop.graph
        assert graph is not None
        loop.set_seg(sigma=INF)                                   # finite -> infinity: the same launches take the mean
        at_inf = loop.denoise(noise).cpu()
        assert loop.graph is graph and {k: r.data_ptr() for k, r in gm.seg._rows.items()} == rows
        table = [S - 0.25 * i for i in range(10)]
        loop.set_seg(table, 1.0)                                  # another scale table, infinity -> finite
        tabled = loop.denoise(noise).cpu()
        assert loop.graph is graph
        loop.set_seg(S)
        assert torch.equal(loop.denoise(noise).cpu(), at1) and loop.graph is graph, "restoring the setting restores the bits"
    for name, out, ref in (("sigma 1", at1, _ref(sigma=1.0)[0]), ("sigma inf", at_inf, _ref(sigma=INF)[0]),
                           ("sigma 1, scale table", tabled, SU.loop64(_model64(), _inputs(), TABLES["euler"](), table, 1.0, (16, 16), g=G)[0])):
        err = _err(out, ref)
        print(f"tiny CFG + SEG after set_seg, {name}: max abs err vs the float64 hooked loop {err:.2e}")
        assert err <= ABS_TOL_STRICT
    apart = float((at1 - at_inf).abs().max())
    print(f"sigma 1 and sigma infinity end {apart:.3f} apart")
    assert apart > 10 * ABS_TOL_STRICT
    with pytest.raises(ValueError, match="set_seg"):
        loop.set_seg([1.0, 2.0])
    with pytest.raises(ValueError, match="sigma"):
        loop.set_seg(sigma=0.0)


def test_seg_scale_zero_is_the_cfg_loop(gpu):
    """seg_scale = 0 keeps the 3B rows and gives the CFG value of e: within the strict gate of a 2B CFG loop of the same g (not
    bit-equal: the UNet's GEMM dispatch depends on the row count)."""
    dtype = torch.float32
    gm = _compiled(dtype)
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        zero = _loop(gm, dtype, gpu, "loop", guidance_scale=G, seg_scale=0.0).denoise(noise).cpu()
        cfg = _loop(gm, dtype, gpu, "loop", guidance_scale=G).denoise(noise).cpu()
    diff = float((zero - cfg).abs().max())
    print(f"tiny seg_scale 0 (3B rows) vs the CFG loop (2B rows): max abs diff {diff:.2e}")
    assert diff <= ABS_TOL_STRICT
    assert _err(zero, _ref(s=None)[0]) <= ABS_TOL_STRICT


def test_batch_rows_match_their_single_runs(gpu):
    """B = 2, two prompts (negatives rows 0, 1; positives rows 2, 3): each row is its own B = 1 run."""
    dtype = torch.float32
    gm = _compiled(dtype)
    x = _inputs(4)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", batch=2, x=x, pos=slice(2, 4), neg=slice(0, 2), guidance_scale=G, seg_scale=S, seg_sigma=1.0)
        assert loop.x_in.shape[0] == 6
        both = loop.denoise(x["latent"][:2]).cpu()
        for k in range(2):
            one = _loop(gm, dtype, gpu, "loop", x=x, pos=slice(2 + k, 3 + k), neg=slice(k, k + 1), guidance_scale=G, seg_scale=S, seg_sigma=1.0)
            single = one.denoise(x["latent"][k:k + 1]).cpu()
            err = float((both[k:k + 1] - single).abs().max())
            print(f"tiny CFG + SEG B=2 row {k} vs its B=1 run: max abs diff {err:.2e}")
            assert err <= ABS_TOL_STRICT
    assert not torch.equal(both[0], both[1])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_16_bit_loops_run_repeat_and_are_finite(gpu, dtype):
    gm = _compiled(dtype, BOTH)
    noise = _inputs()["latent"][:1]
    finals = {}
    with torch.no_grad():
        for mode in ("eager", "loop"):
            loop = _loop(gm, dtype, gpu, mode, guidance_scale=G, seg_scale=S, seg_sigma=1.0)
            finals[mode] = loop.denoise(noise).cpu()
            assert torch.equal(finals[mode], loop.denoise(noise).cpu()), f"{mode}: a replay must repeat its bits"
        loop.set_seg(sigma=INF)
        other = loop.denoise(noise).cpu()
    assert torch.equal(finals["eager"], finals["loop"]) and torch.isfinite(finals["loop"]).all()
    assert torch.isfinite(other).all() and not torch.equal(other, finals["loop"])


def test_fp8_plan_with_seg_runs_and_repeats(gpu):
    dtype = torch.bfloat16
    gm = _compiled(dtype, MID, fp8=True)
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "step", euler_discrete_tables(8), guidance_scale=G, seg_scale=S)
        first = loop.denoise(noise).cpu()
        again = loop.denoise(noise).cpu()
    assert gm.exec_context.fp8 is not None and gm.exec_context.fp8.sites
    assert torch.isfinite(first).all() and torch.equal(first, again)


def test_set_image_lora_and_freeu_keep_working(gpu):
    """SEG touches none of their state: img2img start in mode step, a LoRA-free weight refresh, FreeU sites beside SEG sites."""
    dtype = torch.bfloat16
    m = _model(dtype, gpu)
    targets = {n: tuple(mod.weight.shape) for n, mod in m.named_modules() if n.startswith("mid_block") and n.endswith("attn1.to_q")}
    gm = optimize_model(m, cuda_graph=False, seg_layers=MID, freeu=True)
    assert gm.rewrite_stats["seg_sites"] == 2 == len(targets) and gm.rewrite_stats["freeu_sites"] == 6
    x = _inputs()
    noise = x["latent"][:1]
    init = synth.normal("img2img.init", (1, 4, 16, 16), 77) * 0.8
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "step", guidance_scale=G, seg_scale=S)
        left = loop.set_image(init, noise, 0.5)
        assert left == 5
        loop.run_steps(left)
        a = loop.latent.clone()
        eager = _loop(gm, dtype, gpu, "eager", guidance_scale=G, seg_scale=S)
        eager.run_steps(eager.set_image(init, noise, 0.5))
        assert torch.equal(a, eager.latent) and torch.isfinite(a).all()
        base = loop.denoise(noise)
        loop.set_freeu(0.9, 0.2, 1.3, 1.4)
        on = loop.denoise(noise)
        assert not torch.equal(on, base) and torch.isfinite(on).all()
        loop.set_freeu(None)
        assert loop.refresh_weights() >= 0
        assert torch.equal(loop.denoise(noise), base)
        # a LoRA on the sites' own projections: load moves the result, unload restores the bits, the graph stays
        graph = loop.graph
        sd = {}
        for name, (n_out, n_in) in targets.items():
            sd[f"unet.{name}.lora_A.weight"] = synth.normal(name + ".A", (4, n_in), 5) * 0.1
            sd[f"unet.{name}.lora_B.weight"] = synth.normal(name + ".B", (n_out, 4), 5) * 0.1
        assert not loop.load_lora("a", sd, 1.0)
        with_lora = loop.denoise(noise)
        assert not torch.equal(with_lora, base) and torch.isfinite(with_lora).all()
        loop.unload_lora("a")
        assert torch.equal(loop.denoise(noise), base) and loop.graph is graph


def test_error_cases(gpu):
    dtype = torch.float32
    gm = _compiled(dtype)
    with pytest.raises(ValueError, match="seg_scale"):
        _loop(gm, dtype, gpu, "eager", guidance_scale=G).set_seg(1.0)
    plain = optimize_model(_model(dtype, gpu), cuda_graph=False)
    with pytest.raises(ValueError, match="seg_layers"):
        _loop(plain, dtype, gpu, "eager", guidance_scale=G, seg_scale=S)
    with pytest.raises(ValueError, match="seg_scale cannot be combined with pag_scale"):
        _loop(gm, dtype, gpu, "eager", guidance_scale=G, seg_scale=S, pag_scale=S)
    with pytest.raises(ValueError, match="set_seg"):
        _loop(gm, dtype, gpu, "eager", guidance_scale=G, seg_scale=[1.0] * 9)
    with pytest.raises(ValueError, match="guidance_rescale needs guidance_scale"):
        _loop(gm, dtype, gpu, "eager", seg_scale=S, guidance_rescale=0.7)
    with pytest.raises(ValueError, match="seg_layers"):
        optimize_model(_model(dtype, gpu), cuda_graph=False, seg_layers=("nowhere",))
    with pytest.raises(ValueError, match="seg_layers cannot be combined with pag_layers"):
        optimize_model(_model(dtype, gpu), cuda_graph=False, seg_layers=MID, pag_layers=MID)


# ------------------------------------------------------------------------------------------------ hooks
def _ref_step(chunks, x, layers=MID, sigma=INF, t=300.0):
    m64 = _model64()
    xi = {k: v.double() for k, v in x.items()}
    hw = tuple(x["latent"].shape[-2:])
    with torch.no_grad(), SU.hooked(m64, layers, chunks, hw, sigma):
        return m64(xi["latent"], torch.tensor(t), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]


def test_diffusers_hook_enable_and_disable(gpu):
    dtype = torch.float32
    m = _model(dtype, gpu)
    x = PU.three_rows(16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], cross_attention_kwargs=None,
                       added_cond_kwargs=cond, return_dict=False)[0].clone()
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu, seg_layers=MID)
    base = call(unet)
    assert torch.equal(base, call(unet))                       # (the second call replays the captured graph)
    step_fn = next(iter(unet._steps.values()))
    assert len(step_fn._cached) == 1
    unet.enable_seg(3)
    on = call(unet)
    assert len(step_fn._cached) == 2, "another chunks value is another cache entry, not a replay of the wrong graph"
    assert torch.equal(on, call(unet)) and len(step_fn._cached) == 2
    # (the unperturbed rows: the attention launch of a site now sees a sub-batch, so the strict gate, not bits)
    assert float((on[:2] - base[:2]).abs().max()) <= ABS_TOL_STRICT and float((on[2] - base[2]).abs().max()) > 10 * ABS_TOL_STRICT
    err = _err(on, _ref_step(3, x))
    print(f"diffusers hook, tiny fp32, enable_seg(3): max abs err vs the hooked float64 module {err:.2e}")
    assert err <= ABS_TOL_STRICT
    unet.set_seg_sigma(1.0)                                     # an in-place write: the same graph, another result
    at1 = call(unet)
    assert len(step_fn._cached) == 2 and not torch.equal(at1, on)
    assert _err(at1, _ref_step(3, x, sigma=1.0)) <= ABS_TOL_STRICT
    unet.enable_seg(2, sigma=3.0)
    with pytest.raises(ValueError, match="chunks"):
        call(unet)                                              # 3 rows do not divide into 2 chunks
    unet.disable_seg()
    off = call(unet)
    assert torch.equal(off, base) and len(step_fn._cached) == 2
    assert _err(off, _ref_step(0, x)) <= ABS_TOL_STRICT
    with pytest.raises(ValueError, match="chunks"):
        unet.enable_seg(0)
    with pytest.raises(ValueError, match="sigma"):
        unet.enable_seg(3, sigma=-2.0)
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    for use in (lambda: plain.enable_seg(3), lambda: plain.set_seg_sigma(1.0), lambda: plain.disable_seg()):
        with pytest.raises(ValueError, match="seg_layers"):
            use()


def test_comfy_hook_fully_perturbed_call(gpu):
    dtype = torch.float32
    m = _model(dtype, gpu)
    adapter = hooks.compile_comfy_unet(m, seg_layers=MID)
    assert adapter.compiled.rewrite_stats["seg_sites"] == 2
    x = _inputs()
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    with torch.no_grad():
        y = torch.cat([xg["text_embeds"], m.add_time_proj(xg["time_ids"].flatten()).reshape(2, -1).to(dtype)], dim=-1)
    call = lambda a: a(xg["latent"], timesteps=torch.full((2,), 300.0, device=gpu), context=xg["encoder_hidden_states"], y=y).clone()
    base = call(adapter)
    adapter.enable_seg(1)
    on = call(adapter)
    assert not torch.equal(on, base) and torch.equal(on, call(adapter))
    assert _err(on, _ref_step(1, x)) <= ABS_TOL_STRICT
    adapter.disable_seg()
    assert torch.equal(call(adapter), base)


def test_graphed_module_keys_its_cache_on_chunks(gpu):
    """optimize_model(cuda_graph=True): the module's own graph cache takes `chunks` (and the latent size) into its key."""
    dtype = torch.float32
    gm = optimize_model(_model(dtype, gpu), cuda_graph=True, seg_layers=MID)
    x = PU.three_rows(16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    args = (x["latent"].to(gpu), torch.tensor(500.0, device=gpu), x["encoder_hidden_states"].to(gpu),
            {"text_embeds": x["text_embeds"].to(gpu), "time_ids": x["time_ids"].to(gpu)})
    with torch.no_grad():
        base = gm(*args)[0].clone()
        with gm.seg.using(3, (16, 16)):
            on = gm(*args)[0].clone()
            assert torch.equal(on, gm(*args)[0])
        assert torch.equal(gm(*args)[0], base)
    assert float((on[:2] - base[:2]).abs().max()) <= ABS_TOL_STRICT and float((on[2] - base[2]).abs().max()) > 10 * ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ SDXL-base, one strict step
def test_sdxl_strict_step_with_seg_vs_cpu_fixture(gpu, sdxl_fp32_pair):
    """SDXL-base fp32 at latent 64, rows [negative | positive | perturbed], sigma = infinity, against
    tests/golden/f1_unet_step_latent64_seg.npz (the eager fp32 module with the tests' hooks on the CPU, tools/make_seg_golden.py;
    its own deviation from a float64 run is in the file).  The fixture's sites are all seventy self-attentions: with ("mid",), ten
    sites, the perturbed row is 8.5e-3 from the positive one at timestep 999 and with ("down_blocks.2", "mid") 5.1e-2, both below
    the hundred gates this check asks for; with every site it is 0.157."""
    g = golden("f1_unet_step_latent64_seg")
    ref = torch.from_numpy(g["out"])
    layers = tuple(str(s) for s in g["layers"])
    gm = optimize_model(sdxl_fp32_pair[0], cuda_graph=False, seg_layers=layers)
    assert layers == ("down_blocks", "mid", "up_blocks") and gm.rewrite_stats["seg_sites"] == 70 == int(g["sites"])
    hw = int(g["latent_hw"])
    x = PU.three_rows(hw, 1234)
    xg = {k: v.to(gpu) for k, v in x.items()}
    gm.seg.bind((hw, hw), gpu)
    gm.seg.set_sigma(float(g["sigma"]))
    with torch.no_grad(), gm.seg.using(int(g["chunks"]), (hw, hw)):
        out = gm(xg["latent"], torch.tensor(float(g["timestep"]), device=gpu), xg["encoder_hidden_states"],
                 {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0].float().cpu()
    err = float((out - ref).abs().max())
    gap = float(g["pert_vs_pos_max_abs"])
    print(f"SDXL strict step with SEG: max abs err {err:.2e} (|ref| max {float(ref.abs().max()):.2f}; the perturbed row is {gap:.2e} from "
          f"the positive one; fixture vs float64 {float(g['f64_max_abs_dev']) if 'f64_max_abs_dev' in g.files else float('nan'):.2e})")
    assert gap > 100 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT
