"""LyCORIS forms end to end on the TINY network: a LoKr adapter with DoRA on every Linear and Conv2d, a LoHa adapter on every
Linear with a Tucker LoHa on the 3x3 convs, and a Tucker LoCon on the 3x3 convs - through lora.attach on a graphed
optimize_model result, DenoiseLoop.load_lora(convs=True, lycoris=True) and the Diffusers hook.

Plumbing is checked with no tolerance, as in test_lora_conv_dora_loop_gpu.py: a compiled module with the adapters loaded must
give the bits of a FRESHLY compiled module whose state dict already holds the merged weights.  Numerics are checked against
the oracle run on a state dict merged in float64 by the definitions restated in lora_forms_util.py."""
import pytest
import torch
from torch import nn

import lora_forms_util as lf
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
KW = dict(convs=True, lycoris=True)


def _model(dtype, dev, sd=None):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    if sd is None:
        synth.fill_module_(m, 0)
    else:
        m.load_state_dict(sd)
    return m


def _own_state(compiled, like):
    sd = compiled.state_dict()
    return {k: sd[k].detach().clone() for k in like.state_dict()}


def _is3x3(l):
    return isinstance(l, nn.Conv2d) and tuple(l.kernel_size) == (3, 3)


def _adapters(m, seed):
    """The three adapters of the module docstring: [(name, state dict, {module: parts}), ...].  Delta sizes are those of the
    plain family's tests (elements around 0.02): LoKr w1 ~ 0.15 N(0,1) (x) w2 ~ 0.12 N(0,1), alpha = rank so sigma = 1; LoHa two
    rank-4 products of 0.26 N(0,1) factors; Tucker cores 0.5 N(0,1) between 0.26 (LoHa) or 0.095 (LoCon) N(0,1) factors."""
    g = torch.Generator().manual_seed(seed)
    kr, ha, tu = {}, {}, {}
    for n, l in m.named_modules():
        if not isinstance(l, (nn.Conv2d, nn.Linear)):
            continue
        shape = tuple(l.weight.shape)
        p = lf.make("lokr", shape, g, std=0.15)
        p["lokr_w2"] = p["lokr_w2"] * 0.8
        p["dora_scale"] = (l.weight.detach().float().cpu().reshape(shape[0], -1).norm(dim=1)
                           * (0.8 + 0.4 * torch.rand(shape[0], generator=g))).reshape(-1, *([1] * (len(shape) - 1)))
        kr[n] = p
        if isinstance(l, nn.Linear):
            ha[n] = lf.make("loha", shape, g, rank=4, std=0.26, alpha=4)
        elif _is3x3(l):
            ha[n] = lf.make("loha_tucker", shape, g, rank=4, std=0.26, alpha=4)
            tu[n] = lf.make("tucker", shape, g, rank=4, std=0.095, alpha=4)
    return [(name, {k: v for n, p in parts.items() for k, v in lf.keyed(n, p).items()}, parts)
            for name, parts in (("kr", kr), ("ha", ha), ("tu", tu))]


SCALES = {"kr": 0.8, "ha": -0.9, "tu": 0.6}


def _merge64(base, adapters):
    merged = dict(base)
    for n in {n for _, _, parts in adapters for n in parts}:
        merged[n + ".weight"] = lf.merged64(base[n + ".weight"], [(parts[n], SCALES[name]) for name, _, parts in adapters if n in parts])
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


def _weights(m):
    return {n: l.weight.detach().clone() for n, l in m.named_modules() if isinstance(l, (nn.Conv2d, nn.Linear))}


def _same_weights(m, want):
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    return all(torch.equal(bits(l.weight.detach()), bits(want[n])) for n, l in m.named_modules() if n in want)


# ------------------------------------------------------------------------------------------------ plumbing, bit exact
@pytest.mark.parametrize("dtype", DTYPES)
def test_graphed_module_with_lycoris_adapters_equals_fresh_module_with_merged_weights(gpu, dtype):
    x, xg = _inputs(gpu, dtype)
    t = torch.tensor(500.0, device=gpu)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda gm: gm(xg["latent"], t, xg["encoder_hidden_states"], cond)[0].clone()
    m1 = _model(dtype, gpu)
    gm1 = optimize_model(m1, cuda_graph=True)
    ads = _adapters(m1, 211)
    with torch.no_grad():
        base_out = call(gm1)
        assert torch.equal(base_out, call(gm1))
        graphs = {k: e.graph for k, e in gm1.forward._cached.items()}
        assert graphs
        ls = lora.attach(gm1)
        before = _weights(gm1)
        with pytest.raises(ValueError, match="lycoris=True"):
            ls.load("kr", ads[0][1], 0.8, convs=True)
        assert _same_weights(gm1, before)
        for name, sd, _ in ads:
            assert ls.load(name, sd, SCALES[name], **KW) == []
        assert sorted(ls.adapted_modules()) == _all_targets(m1)
        assert ls._plan.forms and ls._plan.dora
        out1 = call(gm1)
        assert not torch.equal(out1, base_out) and torch.isfinite(out1).all()
        gm2 = optimize_model(_model(dtype, gpu, _own_state(gm1, m1)), cuda_graph=True)
        call(gm2)
        out2 = call(gm2)
        assert torch.equal(out1, out2), f"{dtype}: adapters loaded vs merged weights compiled afresh differ by {float((out1.float() - out2.float()).abs().max()):.3e}"
        ls.set_scale("kr", 0.3)
        assert not torch.equal(call(gm1), out1)
        ls.set_scale("kr", 0.8)
        assert torch.equal(call(gm1), out1), "returning to a scale must return the output"
        ls.unload_all()
        assert _same_weights(gm1, before), "unload must restore every weight bit for bit"
        assert torch.equal(call(gm1), base_out), "unload must restore the output bit for bit"
        now = {k: e.graph for k, e in gm1.forward._cached.items()}
        assert now.keys() == graphs.keys() and all(now[k] is graphs[k] for k in graphs), "load, scale change and unload must not recapture"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["loop", "step", "eager"])
def test_loop_with_lycoris_adapters_equals_fresh_loop_with_merged_weights(gpu, dtype, mode):
    x, _ = _inputs(gpu, dtype)
    m1 = _model(dtype, gpu)
    gm1 = optimize_model(m1, cuda_graph=False)
    ads = _adapters(m1, 221)
    noise = x["latent"][:1]
    with torch.no_grad():
        loop1 = _loop(gm1, dtype, gpu, mode, x)
        base_out = loop1.denoise(noise)
        graph = loop1.graph
        before = _weights(gm1)
        for name, sd, _ in ads:
            assert loop1.load_lora(name, sd, SCALES[name], **KW) == []
        out1 = loop1.denoise(noise)
        assert not torch.equal(out1, base_out) and torch.isfinite(out1).all()
        gm2 = optimize_model(_model(dtype, gpu, _own_state(gm1, m1)), cuda_graph=False)
        out2 = _loop(gm2, dtype, gpu, mode, x).denoise(noise)
        assert torch.equal(out1, out2), f"{dtype} {mode}: differ by {float((out1 - out2).abs().max()):.3e}"
        loop1.set_lora_scale("ha", 1.2)
        assert not torch.equal(loop1.denoise(noise), out1)
        for name, _, _ in ads:
            loop1.unload_lora(name)
        assert _same_weights(gm1, before), "unload must restore every weight bit for bit"
        assert torch.equal(loop1.denoise(noise), base_out), "unload must restore the pre-load output bit for bit"
        assert loop1.graph is graph, "load, scale change and unload must not recapture"


@pytest.mark.parametrize("dtype", DTYPES)
def test_diffusers_hook_with_lycoris_adapters_equals_fresh_hook_with_merged_weights(gpu, dtype):
    x, xg = _inputs(gpu, dtype)
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u, **kw: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], added_cond_kwargs=cond, **kw)[0].clone()
    m = _model(dtype, gpu)
    unet1 = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    ads = _adapters(m, 241)
    base_out = call(unet1)
    assert torch.equal(base_out, call(unet1))
    with pytest.raises(ValueError, match="lycoris=True"):
        unet1.load_lora("ha", ads[1][1], 0.9, convs=True)
    assert torch.equal(call(unet1), base_out)
    for name, sd, _ in ads:
        assert unet1.load_lora(name, sd, SCALES[name], **KW) == []
    out1 = call(unet1)
    assert not torch.equal(out1, base_out)
    unet2 = hooks.compile_unet_from_state_dict(_own_state(unet1.compiled, m), TINY, dtype, gpu)
    call(unet2)
    out2 = call(unet2)
    assert torch.equal(out1, out2), f"{dtype}: differ by {float((out1.float() - out2.float()).abs().max()):.3e}"
    for name, _, _ in ads:
        unet1.unload_lora(name)
    assert torch.equal(call(unet1), base_out)


# ------------------------------------------------------------------------------------------------ numerics
def test_fp32_loop_with_lycoris_adapters_vs_float64_merged_oracle(gpu):
    """LoKr with DoRA on every Conv2d and Linear, LoHa / Tucker LoHa, and a Tucker LoCon, against the oracle on weights merged
    in float64."""
    dtype = torch.float32
    x, _ = _inputs(gpu, dtype)
    m = _model(dtype, gpu)
    base = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    gm = optimize_model(m, cuda_graph=False)
    ads = _adapters(m, 251)
    assert "conv_in" in ads[0][2] and "time_embedding.linear_1" in ads[1][2] and "conv_in" in ads[2][2] and "time_embedding.linear_1" not in ads[2][2]
    tables = euler_discrete_tables(10)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", x, steps=10)
        for name, sd, _ in ads:
            loop.load_lora(name, sd, SCALES[name], **KW)
        out = loop.denoise(x["latent"][:1]).cpu()
    sd = {k: v.float() for k, v in _merge64(base, ads).items()}
    ehs, te, ti = (x[k][[0, 1]] for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    ref = orc.euler_denoise_cfg(lambda xi, t: orc.unet_forward(sd, xi, t, ehs, te, ti), x["latent"][:1], tables, G)
    sd0 = {k: v.float() for k, v in base.items()}
    ref0 = orc.euler_denoise_cfg(lambda xi, t: orc.unet_forward(sd0, xi, t, ehs, te, ti), x["latent"][:1], tables, G)
    err = float((out - ref).abs().max())
    print(f"tiny fp32 10-step CFG loop, LoKr + DoRA on every Conv2d and Linear, LoHa / Tucker LoHa, Tucker LoCon: max abs err vs "
          f"float64-merged oracle {err:.2e} (|ref| max {float(ref.abs().max()):.2f}; the adapters move the result by {float((ref - ref0).abs().max()):.2e})")
    assert float((ref - ref0).abs().max()) > 100 * ABS_TOL_STRICT, "the adapters must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT
