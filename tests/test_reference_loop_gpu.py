"""Reference-only control in the captured denoise loop and behind the hooks, on the TINY network at LATENT 32: the 128-channel level
then has 256 tokens, so bf16 takes the joint-attention kernel there, while the 64-token level (and everything in fp32) takes
ops.attention_joint's slow path.

The reference is the tests' own: the eager module in float64 on the CPU with forward hooks on every attn1 module and a float64
restatement of each sampler (tests/reference_util.py, tests/pag_util.py).  10 steps, g = 5 unless stated; rows [negative | positive |
reference] from synth.denoise_inputs(2, 32, 1234): row 0 the negative prompt, row 1 the prompt, row 0's noise."""
import functools
import types

import pytest
import torch

from stabletriton_amd import hooks, ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import pag_util as PU
from tests import reference_util as RU

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
Z_TOL = 4e-6                    # the generator against its float64 restatement, relative to max(1, |z|) (tests/test_sde_loop_gpu.py)
G = 5.0
HW = 32
LAYERS = (".*",)


def _model(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


@functools.lru_cache(maxsize=None)
def _model64():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double()


@functools.lru_cache(maxsize=None)
def _inputs():
    return synth.denoise_inputs(2, HW, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _reference():
    """(the reference image's latent, its unit noise)"""
    return synth.normal("reference.init", (1, 4, HW, HW), 77) * 0.8, synth.normal("reference.noise", (1, 4, HW, HW), 78)


@functools.lru_cache(maxsize=None)
def _compiled(dtype):
    return optimize_model(_model(dtype, torch.device("cuda:0")), cuda_graph=False, reference_layers=LAYERS)


TABLES = {"euler": lambda: euler_discrete_tables(10), "dpmpp_karras": lambda: dpmpp_2m_tables(10, karras=True),
          "dpmpp_sde": lambda: dpmpp_2m_sde_tables(10)}


@functools.lru_cache(maxsize=None)
def _ref(sampler="euler", with_reference=True, g=G, phi=None, seed=None):
    """float64 hooked loop, computed once per configuration."""
    init, noise = _reference() if with_reference else (None, None)
    return RU.loop64(_model64(), _inputs(), TABLES[sampler](), init, noise, g=g, phi=phi, seed=seed, layers=LAYERS)


def _loop(gm, dtype, dev, mode="loop", tables=None, **kw):
    x = _inputs()
    loop = DenoiseLoop(gm, 1, HW, dtype, dev, tables or TABLES["euler"](), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim,
                       mode=mode, reference=True, **kw)
    rows = lambda k, r: x[k][r].to(dev, dtype)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    if kw.get("guidance_scale") is None:
        loop.set_conditioning(*(rows(k, slice(1, 2)) for k in keys))
    else:
        loop.set_conditioning(*(rows(k, slice(1, 2)) for k in keys), *(rows(k, slice(0, 1)) for k in keys))
    loop.set_reference(*_reference())
    return loop


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ modes
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_modes_agree_and_fp32_matches_the_float64_hooked_loop(gpu, dtype):
    gm = _compiled(dtype)
    assert gm.rewrite_stats["reference_sites"] == 17
    noise = _inputs()["latent"][:1]
    finals = {}
    with torch.no_grad():
        for mode in ("eager", "step", "loop"):
            loop = _loop(gm, dtype, gpu, mode, guidance_scale=G)
            assert loop.x_in.shape[0] == 3 and loop.ehs.shape[0] == 3
            finals[mode] = loop.denoise(noise).cpu()
            assert torch.equal(finals[mode], loop.denoise(noise).cpu()), f"{mode}: a replay must repeat its bits"
            assert gm.reference.chunks == 0 and gm.reference.gate is None, "the loop names the reference block around its own calls only"
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    assert torch.isfinite(finals["loop"]).all()
    if dtype == torch.float32:
        ref, plain = _ref(), _ref(with_reference=False)
        moved = float((ref - plain).abs().max())
        err = _err(finals["loop"], ref)
        print(f"tiny CFG + reference 10-step loop fp32: max abs err vs the float64 hooked loop {err:.2e}; the reference moves the float64 "
              f"result by {moved:.2f}")
        assert moved > 100 * ABS_TOL_STRICT, "the reference must matter for this check to mean anything"
        assert err <= ABS_TOL_STRICT


@pytest.mark.parametrize("config", ["no_guidance", "cfg_rescale", "dpmpp_karras", "dpmpp_sde"])
def test_fp32_configurations_match_the_float64_hooked_loop(gpu, config):
    gm = _compiled(torch.float32)
    noise = _inputs()["latent"][:1]
    sampler, kw, ref_kw, seed = "euler", dict(guidance_scale=G), {}, None
    if config == "no_guidance":
        kw, ref_kw = {}, dict(g=None)
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
        assert loop.x_in.shape[0] == (2 if config == "no_guidance" else 3)
        if seed is not None:
            loop.set_seed(seed)
        out = loop.denoise(noise).cpu()
        assert torch.equal(out, loop.denoise(noise).cpu())
    ref = _ref(sampler, **ref_kw)
    moved = float((ref - _ref(sampler, with_reference=False, **ref_kw)).abs().max())
    err = _err(out, ref)
    print(f"tiny reference {config} fp32: max abs err vs the float64 hooked loop {err:.2e}; the reference moves the float64 result by {moved:.2f}")
    assert moved > 100 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ the kernel adds nothing of its own
def test_bf16_loop_with_the_kernel_equals_the_slow_path_loop(gpu, monkeypatch):
    dtype = torch.bfloat16
    gm = _compiled(dtype)
    noise = _inputs()["latent"][:1]
    calls = {"fused": 0, "slow": 0}
    real = ops.attention_joint

    def counting(q, k, v, k2, v2, num_heads, scale, lead=None, gate=None, fused=None):
        applies = q.dtype in (torch.bfloat16, torch.float16) and q.shape[-1] // num_heads == 64 and k.shape[1] >= 256
        calls["fused" if applies else "slow"] += 1
        return real(q, k, v, k2, v2, num_heads, scale, lead=lead, gate=gate, fused=fused)

    with torch.no_grad():
        monkeypatch.setattr(ops, "attention_joint", counting)
        with_kernel = _loop(gm, dtype, gpu, "eager", guidance_scale=G).denoise(noise).cpu()
        assert calls["fused"] > 0 and calls["slow"] > 0, "latent 32: the 256-token level takes the kernel, the 64-token level the slow path"
        monkeypatch.setattr(ops, "attention_joint", lambda *a, **kw: real(*a, **{**kw, "fused": False}))
        slow = _loop(gm, dtype, gpu, "eager", guidance_scale=G).denoise(noise).cpu()
    assert torch.isfinite(with_kernel).all()
    assert torch.equal(with_kernel, slow), "one launch per site gives the bits of the concatenate-and-attend route"


# ------------------------------------------------------------------------------------------------ the gate
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_set_reference_needs_no_recapture_and_off_ignores_the_reference(gpu, dtype):
    gm = _compiled(dtype)
    noise = _inputs()["latent"][:1]
    init, rnoise = _reference()
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", guidance_scale=G)
        on = loop.denoise(noise).cpu()
        graph = loop.graph
        assert graph is not None
        loop.set_reference(None)
        off = loop.denoise(noise).cpu()
        assert loop.graph is graph and torch.isfinite(off).all() and not torch.equal(off, on)
        loop.reference_init.fill_(float("nan"))             # gated off, the reference rows' keys are never read
        again = loop.denoise(noise).cpu()
        assert loop.graph is graph and torch.isfinite(again).all() and torch.equal(again, off)
        loop.set_reference(init, rnoise, end=0.5)
        first = loop.denoise(noise).cpu()
        loop.set_reference(init, rnoise, start=0.5)
        second = loop.denoise(noise).cpu()
        assert loop.graph is graph
        for half in (first, second):
            assert torch.isfinite(half).all() and not torch.equal(half, on) and not torch.equal(half, off)
        assert not torch.equal(first, second)
        loop.set_reference(init, rnoise)
        assert torch.equal(loop.denoise(noise).cpu(), on) and loop.graph is graph, "restoring the reference restores the bits"
    if dtype == torch.float32:
        plain = _ref(with_reference=False)
        assert _err(off, plain) <= ABS_TOL_STRICT, "gated off: the CFG loop's value (its rows are evaluated in a batch of three)"
        half = RU.loop64(_model64(), _inputs(), TABLES["euler"](), init, rnoise, g=G, layers=LAYERS, on=[i < 5 for i in range(10)])
        assert _err(first, half) <= ABS_TOL_STRICT


def test_seeded_reference_noise_is_rng_stream_at_its_own_counter_word(gpu):
    from stabletriton_amd import pipeline
    dtype = torch.float32
    loop = _loop(_compiled(dtype), dtype, gpu, "eager", guidance_scale=G)
    init, _ = _reference()
    loop.set_seed(5)
    loop.set_reference(init, seed=1234)
    want = PU.unit64(1234, pipeline.REFERENCE_COUNTER_WORD, (1, 4, HW, HW))
    err = (loop.reference_noise.double().cpu() - want).abs() / want.abs().clamp(min=1.0)
    assert float(err.max()) <= Z_TOL
    assert int(loop.seeds[0]) == 5, "the call's seed leaves set_seed's table alone"
    assert pipeline.REFERENCE_COUNTER_WORD > loop.n_steps


# ------------------------------------------------------------------------------------------------ with inpainting
def test_inpaint_with_reference_keeps_the_kept_pixels(gpu):
    dtype = torch.bfloat16
    gm = _compiled(dtype)
    noise = _inputs()["latent"][:1]
    keep = synth.normal("inpaint.init", (1, 4, HW, HW), 79) * 0.8
    mask = torch.ones(HW, HW)
    mask[4:20, 6:18] = 0.0
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", guidance_scale=G, inpaint=True)
        loop.set_inpaint(keep, mask)
        out = loop.denoise(noise).cpu()
        assert torch.equal(out, loop.denoise(noise).cpu())
        kept = (mask == 0).expand(1, 4, HW, HW)
        assert torch.equal(out[kept], keep[kept]), "a kept pixel ends on the init latent bit for bit"
        assert torch.isfinite(out).all() and not torch.equal(out[~kept], keep[~kept])
        loop.set_reference(None)
        off = loop.denoise(noise).cpu()
        assert torch.equal(off[kept], keep[kept]) and not torch.equal(off, out)


# ------------------------------------------------------------------------------------------------ hooks
def _three_rows(dev, dtype):
    """[negative | positive | reference] rows of one UNet call: row 0's latent twice, then the noised reference latent."""
    x = _inputs()
    init, rnoise = _reference()
    out = {k: x[k][[0, 1, 1]].clone() for k in ("encoder_hidden_states", "text_embeds", "time_ids")}
    out["latent"] = torch.cat([x["latent"][[0, 0]], init + 2.0 * rnoise])
    return out, {k: v.to(dev, dtype) for k, v in out.items()}


def test_diffusers_hook_enable_and_disable(gpu):
    dtype = torch.float32
    m = _model(dtype, gpu)
    x, xg = _three_rows(gpu, dtype)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], cross_attention_kwargs=None,
                       added_cond_kwargs=cond, return_dict=False)[0].clone()
    pipe = hooks.attach_to_diffusers(types.SimpleNamespace(unet=m), TINY, dtype, reference_layers=LAYERS)
    unet = pipe.unet
    base = call(unet)
    unet.enable_reference(3)
    on = call(unet)
    assert torch.equal(on, call(unet)), "the second call replays the captured graph"
    step_fn = next(iter(unet._steps.values()))
    assert len(step_fn._cached) == 2, "another chunks value is another cache entry"
    direct = optimize_model(m, cuda_graph=False, reference_layers=LAYERS)
    with torch.no_grad(), direct.reference.using(3):
        want = direct(xg["latent"], torch.tensor(300.0, device=gpu), xg["encoder_hidden_states"], cond)[0]
    assert torch.equal(on, want), "the hook's call is the module's call"
    assert float((on[2] - base[2]).abs().max()) <= ABS_TOL_STRICT and float((on[:2] - base[:2]).abs().max()) > 10 * ABS_TOL_STRICT
    m64 = _model64()
    xi = {k: v.double() for k, v in x.items()}
    with torch.no_grad(), RU.hooked(m64, LAYERS, 3):
        ref = m64(xi["latent"], torch.tensor(300.0), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]
    err = _err(on, ref)
    print(f"diffusers hook, tiny fp32, enable_reference(3): max abs err vs the hooked float64 module {err:.2e}")
    assert err <= ABS_TOL_STRICT
    unet.disable_reference()
    assert torch.equal(call(unet), base)
    with pytest.raises(ValueError, match="chunks"):
        unet.enable_reference(1)
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    with pytest.raises(ValueError, match="reference_layers"):
        plain.enable_reference(3)
    with pytest.raises(ValueError, match="reference_layers"):
        plain.disable_reference()


def test_comfy_hook_and_graphed_module_key_their_caches_on_chunks(gpu):
    dtype = torch.bfloat16
    m = _model(dtype, gpu)
    adapter = hooks.compile_comfy_unet(m, reference_layers=LAYERS)
    assert adapter.compiled.rewrite_stats["reference_sites"] == 17
    _, xg = _three_rows(gpu, dtype)
    with torch.no_grad():
        y = torch.cat([xg["text_embeds"], m.add_time_proj(xg["time_ids"].flatten()).reshape(3, -1).to(dtype)], dim=-1)
    call = lambda a: a(xg["latent"], timesteps=torch.full((3,), 300.0, device=gpu), context=xg["encoder_hidden_states"], y=y).clone()
    base = call(adapter)
    adapter.enable_reference(3)
    on = call(adapter)
    assert torch.isfinite(on).all() and not torch.equal(on[:2], base[:2]) and torch.equal(on, call(adapter))
    adapter.disable_reference()
    assert torch.equal(call(adapter), base)
    gm = optimize_model(_model(dtype, gpu), cuda_graph=True, reference_layers=LAYERS)
    args = (xg["latent"], torch.tensor(300.0, device=gpu), xg["encoder_hidden_states"], {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})
    with torch.no_grad():
        plain = gm(*args)[0].clone()
        with gm.reference.using(3):
            graphed = gm(*args)[0].clone()
            assert torch.equal(graphed, gm(*args)[0])
        assert torch.equal(gm(*args)[0], plain)
    assert not torch.equal(graphed[:2], plain[:2]) and torch.isfinite(graphed).all()


def test_error_cases(gpu):
    dtype = torch.float32
    plain = optimize_model(_model(dtype, gpu), cuda_graph=False)
    with pytest.raises(ValueError, match="reference_layers"):
        DenoiseLoop(plain, 1, HW, dtype, gpu, TABLES["euler"](), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, reference=True)
    with pytest.raises(ValueError, match="reference_layers"):
        optimize_model(_model(dtype, gpu), cuda_graph=False, reference_layers=("nowhere",))
    with pytest.raises(ValueError, match="cannot be combined"):
        optimize_model(_model(dtype, gpu), cuda_graph=False, reference_layers=LAYERS, pag_layers=("mid",))
