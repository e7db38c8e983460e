"""LoCon conv adapters and DoRA end to end on the TINY network: a DoRA adapter on every Conv2d and Linear plus a plain
conv-only adapter, through lora.attach on a graphed optimize_model result, DenoiseLoop.load_lora(convs=True) and the
Diffusers hook.

Plumbing is checked with no tolerance, as in test_lora_loop_gpu.py: a compiled module with the adapters loaded must give the
bits of a FRESHLY compiled module whose state dict already holds the merged weights - a conv that reads a copy of its
weight, or a strict-mode split image that was not re-derived, shows as a difference.  Numerics are checked against the
oracle run on a state dict merged in float64 by the DoRA formula

    V_j = B + s_j up_j down_j,   g_j[n] = m_j[n] / ||V_j[n]||  (1 for the plain adapter),   W = B + sum_j (g_j V_j - B)."""
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


def _adapter(m, rank, seed, dora, convs_only=False, std=0.08):
    """A seeded synthetic adapter on every Conv2d and Linear of `m` (or on the Conv2d alone), kohya-keyed; with `dora` every
    module also gets a magnitude ||B[n]|| * U(0.8, 1.2).  Returns (state dict, {module: (down, up, magnitude or None)})."""
    g = torch.Generator().manual_seed(seed)
    sd, facs = {}, {}
    for n, l in m.named_modules():
        if not isinstance(l, (nn.Conv2d,) if convs_only else (nn.Conv2d, nn.Linear)):
            continue
        shape = tuple(l.weight.shape)
        if len(shape) == 4:
            down, up = torch.randn(rank, *shape[1:], generator=g) * std, torch.randn(shape[0], rank, 1, 1, generator=g) * std
        else:
            down, up = torch.randn(rank, shape[1], generator=g) * std, torch.randn(shape[0], rank, generator=g) * std
        stem = "lora_unet_" + n.replace(".", "_")
        sd[stem + ".lora_down.weight"], sd[stem + ".lora_up.weight"], sd[stem + ".alpha"] = down, up, torch.tensor(float(rank))
        mag = None
        if dora:
            mag = l.weight.detach().float().cpu().reshape(shape[0], -1).norm(dim=1) * (0.8 + 0.4 * torch.rand(shape[0], generator=g))
            sd[stem + ".dora_scale"] = mag.reshape(-1, *([1] * (len(shape) - 1)))
        facs[n] = (down, up, mag)
    return sd, facs


def _merge64(base, adapters):
    """The formula above in float64 on the state dict `base` (float64, the weights' own 4-D / 2-D shapes); alpha = rank."""
    merged = dict(base)
    for n in {n for facs, _ in adapters for n in facs}:
        b = base[n + ".weight"]
        rows = b.reshape(b.shape[0], -1)
        w = rows.clone()
        for facs, s in adapters:
            if n not in facs:
                continue
            down, up, mag = facs[n]
            r = down.shape[0]
            v = rows + s * (up.double().reshape(-1, r) @ down.double().reshape(r, -1))
            w = w + ((mag.double() / v.norm(dim=1))[:, None] if mag is not None else 1.0) * v - rows
        merged[n + ".weight"] = w.reshape(b.shape)
    return merged


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


def _all_targets(m):
    return sorted(n for n, l in m.named_modules() if isinstance(l, (nn.Conv2d, nn.Linear)))


# ------------------------------------------------------------------------------------------------ plumbing, bit exact
@pytest.mark.parametrize("dtype", DTYPES)
def test_graphed_module_with_conv_dora_adapters_equals_fresh_module_with_merged_weights(gpu, dtype):
    x, xg = _inputs(gpu, dtype)
    t = torch.tensor(500.0, device=gpu)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda gm: gm(xg["latent"], t, xg["encoder_hidden_states"], cond)[0].clone()
    m1 = _model(dtype, gpu)
    gm1 = optimize_model(m1, cuda_graph=True)
    sd_d, _ = _adapter(m1, 8, 111, dora=True)
    sd_p, _ = _adapter(m1, 4, 112, dora=False, convs_only=True)
    with torch.no_grad():
        base_out = call(gm1)
        assert torch.equal(base_out, call(gm1))                   # (the second call replays the captured graph)
        graphs = {k: e.graph for k, e in gm1.forward._cached.items()}
        assert graphs
        ls = lora.attach(gm1)
        assert ls.load("d", sd_d, 0.8, convs=True) == []
        assert ls.load("p", sd_p, -0.5, convs=True) == []
        assert sorted(ls.adapted_modules()) == _all_targets(m1)
        out1 = call(gm1)
        assert not torch.equal(out1, base_out) and torch.isfinite(out1).all()
        gm2 = optimize_model(_model(dtype, gpu, _own_state(gm1, m1)), cuda_graph=True)
        call(gm2)
        out2 = call(gm2)
        assert torch.equal(out1, out2), f"{dtype}: adapters loaded vs merged weights compiled afresh differ by {float((out1.float() - out2.float()).abs().max()):.3e}"
        ls.set_scale("d", 0.3)
        assert not torch.equal(call(gm1), out1)
        ls.set_scale("d", 0.8)
        assert torch.equal(call(gm1), out1), "returning to a scale must return the output"
        ls.unload_all()
        assert torch.equal(call(gm1), base_out), "unload must restore the output bit for bit"
        now = {k: e.graph for k, e in gm1.forward._cached.items()}
        assert now.keys() == graphs.keys() and all(now[k] is graphs[k] for k in graphs), "load, scale change and unload must not recapture"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["loop", "step", "eager"])
def test_loop_with_conv_dora_adapters_equals_fresh_loop_with_merged_weights(gpu, dtype, mode):
    x, _ = _inputs(gpu, dtype)
    m1 = _model(dtype, gpu)
    gm1 = optimize_model(m1, cuda_graph=False)
    sd_d, _ = _adapter(m1, 8, 121, dora=True)
    sd_p, _ = _adapter(m1, 4, 122, dora=False, convs_only=True)
    noise = x["latent"][:1]
    with torch.no_grad():
        loop1 = _loop(gm1, dtype, gpu, mode, x)
        base_out = loop1.denoise(noise)                            # captured with the base weights
        graph = loop1.graph
        assert loop1.load_lora("d", sd_d, 0.7, convs=True) == []
        assert loop1.load_lora("p", sd_p, -0.6, convs=True) == []
        out1 = loop1.denoise(noise)
        assert not torch.equal(out1, base_out) and torch.isfinite(out1).all()
        gm2 = optimize_model(_model(dtype, gpu, _own_state(gm1, m1)), cuda_graph=False)
        out2 = _loop(gm2, dtype, gpu, mode, x).denoise(noise)
        assert torch.equal(out1, out2), f"{dtype} {mode}: differ by {float((out1 - out2).abs().max()):.3e}"
        loop1.set_lora_scale("d", 1.2)
        assert not torch.equal(loop1.denoise(noise), out1)
        loop1.unload_lora("p")
        loop1.unload_lora("d")
        assert torch.equal(loop1.denoise(noise), base_out), "unload must restore the pre-load output bit for bit"
        assert loop1.graph is graph, "load, scale change and unload must not recapture"


@pytest.mark.parametrize("dtype", DTYPES)
def test_diffusers_hook_with_conv_dora_adapters_equals_fresh_hook_with_merged_weights(gpu, dtype):
    x, xg = _inputs(gpu, dtype)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u, **kw: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], added_cond_kwargs=cond, **kw)[0].clone()
    m = _model(dtype, gpu)
    unet1 = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    sd_d, _ = _adapter(m, 8, 141, dora=True)
    sd_p, _ = _adapter(m, 4, 142, dora=False, convs_only=True)
    base_out = call(unet1)
    assert torch.equal(base_out, call(unet1))
    with pytest.raises(ValueError, match="pass convs=True"):
        unet1.load_lora("d", sd_d, 0.9)
    assert torch.equal(call(unet1), base_out)
    assert unet1.load_lora("d", sd_d, 0.9, convs=True) == []
    assert unet1.load_lora("p", sd_p, 0.5, convs=True) == []
    out1 = call(unet1)
    assert not torch.equal(out1, base_out)
    unet2 = hooks.compile_unet_from_state_dict(_own_state(unet1.compiled, m), TINY, dtype, gpu)
    call(unet2)
    out2 = call(unet2)
    assert torch.equal(out1, out2), f"{dtype}: differ by {float((out1.float() - out2.float()).abs().max()):.3e}"
    unet1.unload_lora("d")
    unet1.unload_lora("p")
    assert torch.equal(call(unet1), base_out)


# ------------------------------------------------------------------------------------------------ numerics
def test_fp32_loop_with_conv_dora_adapters_vs_float64_merged_oracle(gpu):
    """DoRA on every Conv2d and Linear plus a plain conv-only adapter, against the oracle on weights merged in float64."""
    dtype = torch.float32
    x, _ = _inputs(gpu, dtype)
    m = _model(dtype, gpu)
    base = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    gm = optimize_model(m, cuda_graph=False)
    sd_d, facs_d = _adapter(m, 8, 151, dora=True)
    sd_p, facs_p = _adapter(m, 4, 152, dora=False, convs_only=True)
    assert "conv_in" in facs_d and "time_embedding.linear_1" in facs_d and "conv_out" in facs_p and "time_embedding.linear_1" not in facs_p
    tables = euler_discrete_tables(10)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", x, steps=10)
        loop.load_lora("d", sd_d, 0.8, convs=True)
        loop.load_lora("p", sd_p, -0.6, convs=True)
        out = loop.denoise(x["latent"][:1]).cpu()
    sd = {k: v.float() for k, v in _merge64(base, [(facs_d, 0.8), (facs_p, -0.6)]).items()}
    ehs, te, ti = (x[k][[0, 1]] for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    ref = orc.euler_denoise_cfg(lambda xi, t: orc.unet_forward(sd, xi, t, ehs, te, ti), x["latent"][:1], tables, G)
    sd0 = {k: v.float() for k, v in base.items()}
    ref0 = orc.euler_denoise_cfg(lambda xi, t: orc.unet_forward(sd0, xi, t, ehs, te, ti), x["latent"][:1], tables, G)
    err = float((out - ref).abs().max())
    print(f"tiny fp32 10-step CFG loop, DoRA on every Conv2d and Linear + a plain conv adapter: max abs err vs float64-merged "
          f"oracle {err:.2e} (|ref| max {float(ref.abs().max()):.2f}; the adapters move the result by {float((ref - ref0).abs().max()):.2e})")
    assert float((ref - ref0).abs().max()) > 100 * ABS_TOL_STRICT, "the adapters must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT
