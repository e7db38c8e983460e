"""LoRA adapters end to end on the TINY network: DenoiseLoop.load_lora / set_lora_scale / unload_lora, lora.attach on an
optimize_model result, and the Diffusers hook.

Plumbing is checked with no tolerance: a compiled module with an adapter loaded must give the bits of a FRESHLY compiled
module whose state dict already holds the merged weights the first one produced - a missed derived buffer, stale hoisted
K/V or time tables, or a missed fp8 recalibration shows as a difference.  Numerics are checked against the oracle run on a
state dict merged in float64."""
import pytest
import torch
from torch import nn

from oracle import unet_oracle as orc
from stabletriton_amd import hooks, lora, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
G = 5.0


def _model(dtype, dev, sd=None):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    if sd is None:
        synth.fill_module_(m, 0)
    else:
        m.load_state_dict(sd)
    return m


def _own_state(compiled, like):
    """The compiled module's weights under the model's own keys (its hoisted sub-graphs list the same tensors again)."""
    sd = compiled.state_dict()
    return {k: sd[k].detach().clone() for k in like.state_dict()}


def _adapter(m, rank, seed, names=None, std=0.08):
    """A seeded synthetic adapter on the Linear modules of `m` (all of them, the time path included, or those in `names`):
    (kohya-keyed state dict, {module: (down, up)})."""
    g = torch.Generator().manual_seed(seed)
    sd, facs = {}, {}
    for n, l in m.named_modules():
        if not isinstance(l, nn.Linear) or (names is not None and not names(n)):
            continue
        N, K = l.weight.shape
        down, up = torch.randn(rank, K, generator=g) * std, torch.randn(N, rank, generator=g) * std
        stem = "lora_unet_" + n.replace(".", "_")
        sd[stem + ".lora_down.weight"], sd[stem + ".lora_up.weight"], sd[stem + ".alpha"] = down, up, torch.tensor(float(rank))
        facs[n] = (down, up)
    return sd, facs


def _inputs(dev, dtype):
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    return x, {k: v.to(dev, dtype) for k, v in x.items()}


def _loop(gm, dtype, dev, mode, x, steps=6):
    loop = DenoiseLoop(gm, 1, 16, dtype, dev, euler_discrete_tables(steps), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim,
                       guidance_scale=G, mode=mode)
    rows = lambda k, r: x[k][r].to(dev, dtype)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    loop.set_conditioning(*(rows(k, slice(1, 2)) for k in keys), *(rows(k, slice(0, 1)) for k in keys))
    return loop


# ------------------------------------------------------------------------------------------------ plumbing, bit exact
@pytest.mark.parametrize("dtype", DTYPES)
def test_graphed_module_with_adapter_equals_fresh_module_with_merged_weights(gpu, dtype):
    x, xg = _inputs(gpu, dtype)
    t = torch.tensor(500.0, device=gpu)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda gm: gm(xg["latent"], t, xg["encoder_hidden_states"], cond)[0].clone()
    m1 = _model(dtype, gpu)
    gm1 = optimize_model(m1, cuda_graph=True)
    sd_a, _ = _adapter(m1, 8, 11)
    sd_b, _ = _adapter(m1, 32, 12, names=lambda n: ".attn" in n)
    with torch.no_grad():
        base_out = call(gm1)
        assert torch.equal(base_out, call(gm1))                   # (the second call replays the captured graph)
        ls = lora.attach(gm1)
        ls.load("a", sd_a, 0.8)
        ls.load("b", sd_b, -0.5)
        out1 = call(gm1)
        assert not torch.equal(out1, base_out)
        gm2 = optimize_model(_model(dtype, gpu, _own_state(gm1, m1)), cuda_graph=True)
        call(gm2)
        out2 = call(gm2)
        assert torch.equal(out1, out2), f"{dtype}: adapter loaded vs merged weights compiled afresh differ by {float((out1.float() - out2.float()).abs().max()):.3e}"
        ls.unload_all()
        assert torch.equal(call(gm1), base_out), "unload must restore the output bit for bit"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["loop", "step", "eager"])
def test_loop_with_adapter_equals_fresh_loop_with_merged_weights(gpu, dtype, mode):
    x, _ = _inputs(gpu, dtype)
    m1 = _model(dtype, gpu)
    gm1 = optimize_model(m1, cuda_graph=False)
    sd_a, _ = _adapter(m1, 8, 21)
    with torch.no_grad():
        loop1 = _loop(gm1, dtype, gpu, mode, x)
        base_out = loop1.denoise(x["latent"][:1])                  # captured with the base weights
        graph = loop1.graph
        assert loop1.load_lora("a", sd_a, 0.7) == []
        out1 = loop1.denoise(x["latent"][:1])
        assert loop1.graph is graph, "a LoRA load must not recapture"
        assert not torch.equal(out1, base_out) and torch.isfinite(out1).all()
        gm2 = optimize_model(_model(dtype, gpu, _own_state(gm1, m1)), cuda_graph=False)
        out2 = _loop(gm2, dtype, gpu, mode, x).denoise(x["latent"][:1])
    assert torch.equal(out1, out2), f"{dtype} {mode}: differ by {float((out1 - out2).abs().max()):.3e}"


@pytest.mark.parametrize("mode", ["loop", "step"])
def test_fp8_loop_with_adapter_equals_fresh_loop_with_merged_weights(gpu, mode):
    """fp8 plan: the derived e4m3 weights follow the merge and every trajectory re-measures its scales (set_noise)."""
    dtype = torch.bfloat16
    x, _ = _inputs(gpu, dtype)
    m1 = _model(dtype, gpu)
    gm1 = optimize_model(m1, cuda_graph=False, fp8=True)
    sd_a, _ = _adapter(m1, 16, 31)
    with torch.no_grad():
        loop1 = _loop(gm1, dtype, gpu, mode, x)
        base_out = loop1.denoise(x["latent"][:1])
        assert gm1.exec_context.fp8 is not None and gm1.exec_context.fp8.sites
        graph = loop1.graph
        loop1.load_lora("a", sd_a, 0.7)
        out1 = loop1.denoise(x["latent"][:1])
        assert loop1.graph is graph and not torch.equal(out1, base_out)
        gm2 = optimize_model(_model(dtype, gpu, _own_state(gm1, m1)), cuda_graph=False, fp8=True)
        out2 = _loop(gm2, dtype, gpu, mode, x).denoise(x["latent"][:1])
        assert torch.equal(out1, out2), f"fp8 {mode}: differ by {float((out1 - out2).abs().max()):.3e}"
        loop1.unload_lora("a")
        assert torch.equal(loop1.denoise(x["latent"][:1]), base_out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_diffusers_hook_with_adapter_equals_fresh_hook_with_merged_weights(gpu, dtype):
    x, xg = _inputs(gpu, dtype)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u, **kw: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], added_cond_kwargs=cond, **kw)[0].clone()
    m = _model(dtype, gpu)
    unet1 = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    sd_a, _ = _adapter(m, 8, 41)
    base_out = call(unet1)
    assert torch.equal(base_out, call(unet1))
    unet1.load_lora("a", sd_a, 0.9)
    out1 = call(unet1)
    assert not torch.equal(out1, base_out)
    unet2 = hooks.compile_unet_from_state_dict(_own_state(unet1.compiled, m), TINY, dtype, gpu)
    call(unet2)
    out2 = call(unet2)
    assert torch.equal(out1, out2), f"{dtype}: differ by {float((out1.float() - out2.float()).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ numerics
def test_fp32_loop_with_adapters_on_every_linear_vs_float64_merged_oracle(gpu):
    """Adapters on every Linear (time-path Linears included), two at once, against the oracle on weights merged in float64.
    Measured worst case on one MI355X: 7.9e-5 against the gate of 1e-3 (|ref| max 32.8; the adapters move the result by 18.8)."""
    dtype = torch.float32
    x, _ = _inputs(gpu, dtype)
    m = _model(dtype, gpu)
    base = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    gm = optimize_model(m, cuda_graph=False)
    sd_a, facs_a = _adapter(m, 8, 51)
    sd_b, facs_b = _adapter(m, 4, 52, names=lambda n: "attn2" in n or "time_emb" in n or "embedding" in n)
    assert "time_embedding.linear_1" in facs_a and "down_blocks.0.resnets.0.time_emb_proj" in facs_b
    tables = euler_discrete_tables(10)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", x, steps=10)
        loop.load_lora("a", sd_a, 0.8)
        loop.load_lora("b", sd_b, -0.6)
        out = loop.denoise(x["latent"][:1]).cpu()
    merged = dict(base)
    for facs, s in ((facs_a, 0.8), (facs_b, -0.6)):
        for n, (down, up) in facs.items():
            merged[n + ".weight"] = merged[n + ".weight"] + s * (up.double() @ down.double())      # alpha = rank
    sd = {k: v.float() for k, v in merged.items()}
    ehs, te, ti = (x[k][[0, 1]] for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    ref = orc.euler_denoise_cfg(lambda xi, t: orc.unet_forward(sd, xi, t, ehs, te, ti), x["latent"][:1], tables, G)
    sd0 = {k: v.float() for k, v in base.items()}
    ref0 = orc.euler_denoise_cfg(lambda xi, t: orc.unet_forward(sd0, xi, t, ehs, te, ti), x["latent"][:1], tables, G)
    err = float((out - ref).abs().max())
    print(f"tiny fp32 10-step CFG loop, adapters on every Linear: max abs err vs float64-merged oracle {err:.2e} "
          f"(|ref| max {float(ref.abs().max()):.2f}; the adapters move the result by {float((ref - ref0).abs().max()):.2e})")
    assert float((ref - ref0).abs().max()) > 100 * ABS_TOL_STRICT, "the adapters must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ lifecycle
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scale_changes_and_unload_are_bit_exact_and_never_recapture(gpu, dtype):
    x, _ = _inputs(gpu, dtype)
    m = _model(dtype, gpu)
    gm = optimize_model(m, cuda_graph=False)
    sd_a, _ = _adapter(m, 8, 61)
    sd_b, _ = _adapter(m, 64, 62, names=lambda n: "ff.net" in n)
    noise = x["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", x)
        before = loop.denoise(noise)
        graph = loop.graph
        assert graph is not None
        weights = _own_state(gm, m)
        loop.load_lora("a", sd_a, 0.6)
        at_06 = loop.denoise(noise)
        loop.set_lora_scale("a", 1.4)
        at_14 = loop.denoise(noise)
        assert not torch.equal(at_06, before) and not torch.equal(at_14, at_06)
        loop.set_lora_scale("a", 0.6)
        assert torch.equal(loop.denoise(noise), at_06), "returning to a scale must return the output"
        loop.load_lora("b", sd_b, -1.0)
        assert not torch.equal(loop.denoise(noise), at_06)
        loop.unload_lora("b")
        assert torch.equal(loop.denoise(noise), at_06)
        loop.set_lora_scale("a", 0.0)
        assert torch.equal(loop.denoise(noise), before), "scale 0 is the base"
        loop.set_lora_scale("a", 0.6)
        loop.unload_lora("a")
        assert torch.equal(loop.denoise(noise), before), "unload must restore the pre-load output"
        after = _own_state(gm, m)
        assert all(torch.equal(after[k], weights[k]) for k in weights), "unload must restore every weight bit for bit"
        assert loop.graph is graph, "no recapture at any point"
        with pytest.raises(KeyError):
            loop.set_lora_scale("a", 1.0)


def test_load_before_conditioning_and_two_loops_do_not_disturb_each_other(gpu):
    dtype = torch.float32
    x, _ = _inputs(gpu, dtype)
    m1, m2 = _model(dtype, gpu), _model(dtype, gpu)
    gm1, gm2 = optimize_model(m1, cuda_graph=False), optimize_model(m2, cuda_graph=False)
    sd_a, _ = _adapter(m1, 8, 71)
    noise = x["latent"][:1]
    with torch.no_grad():
        l1, l2 = _loop(gm1, dtype, gpu, "step", x), _loop(gm2, dtype, gpu, "step", x)
        base1, base2 = l1.denoise(noise), l2.denoise(noise)
        assert torch.equal(base1, base2)
        l1.load_lora("a", sd_a, 1.0)
        with_a = l1.denoise(noise)
        assert not torch.equal(with_a, base1)
        assert torch.equal(l2.denoise(noise), base2), "a loop that shares no module is not disturbed"
        assert lora.attach(gm2).names() == [] and lora.attach(gm1).names() == ["a"]
        # an adapter loaded before the loop has any conditioning: the first set_conditioning derives everything from merged weights
        m3 = _model(dtype, gpu)
        gm3 = optimize_model(m3, cuda_graph=False)
        l3 = DenoiseLoop(gm3, 1, 16, dtype, gpu, euler_discrete_tables(6), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim,
                         guidance_scale=G, mode="step")
        l3.load_lora("a", sd_a, 1.0)
        rows = lambda k, r: x[k][r].to(gpu, dtype)
        keys = ("encoder_hidden_states", "text_embeds", "time_ids")
        l3.set_conditioning(*(rows(k, slice(1, 2)) for k in keys), *(rows(k, slice(0, 1)) for k in keys))
        assert torch.equal(l3.denoise(noise), with_a)


# ------------------------------------------------------------------------------------------------ hooks
def test_hook_scale_keyword_is_the_global_multiplier(gpu):
    dtype = torch.float16
    x, xg = _inputs(gpu, dtype)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u, **kw: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], added_cond_kwargs=cond, **kw)[0].clone()
    m = _model(dtype, gpu)
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    sd_a, _ = _adapter(m, 8, 81)
    base_out = call(unet)
    with pytest.raises(NotImplementedError):                       # no adapter loaded: exactly the earlier behaviour
        call(unet, cross_attention_kwargs={"scale": 0.5})
    unet.load_lora("a", sd_a, 1.0)
    full = call(unet)
    half_kw = call(unet, cross_attention_kwargs={"scale": 0.5})
    assert torch.equal(half_kw, call(unet, cross_attention_kwargs={"scale": 0.5}))
    assert torch.equal(call(unet), full) and torch.equal(call(unet, cross_attention_kwargs={"scale": 1.0}), full)
    unet.set_lora_scale("a", 0.5)
    assert torch.equal(call(unet), half_kw), "scale keyword 0.5 must equal set_lora_scale(0.5)"
    assert not torch.equal(half_kw, full) and not torch.equal(half_kw, base_out)
    with pytest.raises(NotImplementedError):
        call(unet, cross_attention_kwargs={"scale": 1.0, "gligen": {}})
    unet.unload_lora("a")
    assert torch.equal(call(unet), base_out)
    with pytest.raises(NotImplementedError):
        call(unet, cross_attention_kwargs={"scale": 0.5})


def test_comfy_hook_loads_adapters_under_the_models_own_names(gpu):
    dtype = torch.bfloat16
    m = _model(dtype, gpu)
    adapter = hooks.compile_comfy_unet(m)
    sd_a, facs = _adapter(m, 8, 91)
    x, xg = _inputs(gpu, dtype)
    y = torch.randn(2, TINY.add_in_dim, generator=torch.Generator().manual_seed(3)).to(gpu, dtype)
    call = lambda: adapter(xg["latent"], timesteps=torch.full((2,), 300.0, device=gpu), context=xg["encoder_hidden_states"], y=y).clone()
    base_out = call()
    assert adapter.load_lora("a", sd_a, 0.8) == []
    assert sorted(lora.attach(adapter.compiled).adapted_modules()) == sorted(facs)
    assert not torch.equal(call(), base_out)
    adapter.unload_lora("a")
    assert torch.equal(call(), base_out)
