"""FreeU in the captured denoise loop and behind the two hooks, on the TINY network.

Plumbing is checked with no tolerance: the three loop modes give the same bits, a `set_freeu` on a captured loop keeps the
graph and gives the bits of a fresh eager-mode loop built with those parameters, and clearing restores the earlier bits."""
import pytest
import torch

from stabletriton_amd import hooks, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import freeu_util as FU
from tests.util import rounded

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
V = FU.SDXL_VALUES
G = 5.0


def _model(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


def _inputs():
    return synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


def _loop(gm, dtype, dev, mode, x, tables=None, guidance=None):
    loop = DenoiseLoop(gm, 1, 16, dtype, dev, tables or euler_discrete_tables(6), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim,
                       guidance_scale=guidance, mode=mode)
    rows = lambda k, r: x[k][r].to(dev, dtype)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    if guidance is None:
        loop.set_conditioning(*(rows(k, slice(1, 2)) for k in keys))
    else:
        loop.set_conditioning(*(rows(k, slice(1, 2)) for k in keys), *(rows(k, slice(0, 1)) for k in keys))
    return loop


@pytest.mark.parametrize("dtype", DTYPES)
def test_modes_agree_and_set_freeu_never_recaptures(gpu, dtype):
    x = _inputs()
    noise = x["latent"][:1]
    gm = optimize_model(_model(dtype, gpu), cuda_graph=False, freeu=True)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", x)
        before = loop.denoise(noise)                         # captured with neutral parameters
        graph = loop.graph
        assert graph is not None
        loop.set_freeu(**V)
        on = loop.denoise(noise)
        assert loop.graph is graph, "set_freeu must not recapture"
        assert torch.isfinite(on).all() and not torch.equal(on, before)
        for mode in ("step", "eager"):
            other = _loop(gm, dtype, gpu, mode, x).denoise(noise)
            assert torch.equal(other, on), f"{dtype} {mode}: differs from the loop graph by {float((other - on).abs().max()):.3e}"
        # a freshly compiled module, parameters set before anything ran, nothing captured
        gm2 = optimize_model(_model(dtype, gpu), cuda_graph=False, freeu=True)
        fresh = _loop(gm2, dtype, gpu, "eager", x)
        fresh.set_freeu(**V)
        out2 = fresh.denoise(noise)
        assert torch.equal(on, out2), f"{dtype}: captured loop after set_freeu vs fresh eager loop differ by {float((on - out2).abs().max()):.3e}"
        loop.set_freeu(**V, version=2)
        v2 = loop.denoise(noise)
        fresh.set_freeu(**V, version=2)
        assert loop.graph is graph and not torch.equal(v2, on) and torch.equal(v2, fresh.denoise(noise))
        loop.set_freeu(None)
        assert torch.equal(loop.denoise(noise), before), "set_freeu(None) must restore the earlier result bit for bit"
        assert loop.graph is graph


def test_guided_loop(gpu):
    """2B rows: every row is its own sample (version 2 normalises per row)."""
    dtype = torch.float32
    x = _inputs()
    noise = x["latent"][:1]
    m = _model(dtype, gpu)
    gm = optimize_model(m, cuda_graph=False, freeu=True)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", x, guidance=G)
        before = loop.denoise(noise)
        graph = loop.graph
        loop.set_freeu(**V, version=2)
        on = loop.denoise(noise)
        assert loop.graph is graph and not torch.equal(on, before) and torch.isfinite(on).all()
        eager = _loop(gm, dtype, gpu, "eager", x, guidance=G).denoise(noise)
        assert torch.equal(on, eager)
        # one guided UNet evaluation against the float64 hook route: rows [negative | positive] are independent samples
        ref_m = UNet2DConditionModel(TINY).eval().requires_grad_(False).double()
        ref_m.load_state_dict({k: v.detach().double().cpu() for k, v in m.state_dict().items()})
        xi = {k: v.double() for k, v in x.items()}
        with FU.hooked(ref_m, **V, version=2):
            both = ref_m(xi["latent"], torch.tensor(500.0), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]
            one = ref_m(xi["latent"][1:], torch.tensor(500.0), xi["encoder_hidden_states"][1:],
                        {"text_embeds": xi["text_embeds"][1:], "time_ids": xi["time_ids"][1:]})[0]
        assert float((both[1:] - one).abs().max()) < 1e-10
        xg = {k: v.to(gpu, dtype) for k, v in x.items()}
        out = gm(xg["latent"], torch.tensor(500.0, device=gpu), xg["encoder_hidden_states"],
                 {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0].double().cpu()
        err = float((out - both).abs().max())
        print(f"tiny fp32 batch-2 step, FreeU v2: {err:.2e}")
        assert err <= 1e-3
        loop.set_freeu(None)
        assert torch.equal(loop.denoise(noise), before)


def test_dpmpp_2m_loop(gpu):
    dtype = torch.bfloat16
    x = _inputs()
    noise = x["latent"][:1]
    tables = dpmpp_2m_tables(6)
    gm = optimize_model(_model(dtype, gpu), cuda_graph=False, freeu=True)
    with torch.no_grad():
        loop = _loop(gm, dtype, gpu, "loop", x, tables=tables, guidance=G)
        before = loop.denoise(noise)
        graph = loop.graph
        loop.set_freeu(**V)
        on = loop.denoise(noise)
        assert loop.graph is graph and not torch.equal(on, before) and torch.isfinite(on).all()
        for mode in ("step", "eager"):
            assert torch.equal(_loop(gm, dtype, gpu, mode, x, tables=tables, guidance=G).denoise(noise), on), mode
        loop.set_freeu(None)
        assert torch.equal(loop.denoise(noise), before)


def test_set_freeu_needs_a_unet_compiled_with_it(gpu):
    dtype = torch.float32
    x = _inputs()
    loop = _loop(optimize_model(_model(dtype, gpu), cuda_graph=False), dtype, gpu, "eager", x)
    with pytest.raises(ValueError, match="freeu=True"):
        loop.set_freeu(**V)
    with pytest.raises(ValueError, match="freeu=True"):
        loop.set_freeu(None)
    ok = _loop(optimize_model(_model(dtype, gpu), cuda_graph=False, freeu=True), dtype, gpu, "eager", x)
    with pytest.raises(ValueError):
        ok.set_freeu(0.9, 0.2, -1.3, 1.4)
    with pytest.raises(ValueError):
        ok.set_freeu(None, 0.2)


# ------------------------------------------------------------------------------------------------ hooks
def _ref_step(m, x, dtype, t, version):
    ref_m = UNet2DConditionModel(TINY).eval().requires_grad_(False).double()
    ref_m.load_state_dict({k: v.detach().double().cpu() for k, v in m.state_dict().items()})
    xi = {k: rounded(v, dtype).double() for k, v in x.items()}
    with torch.no_grad(), FU.hooked(ref_m, **V, version=version):
        return ref_m(xi["latent"], torch.tensor(t), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]


def test_diffusers_hook_enable_and_disable(gpu):
    dtype = torch.float32
    x = _inputs()
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    cond = {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]}
    call = lambda u: u(xg["latent"], torch.tensor(300.0), encoder_hidden_states=xg["encoder_hidden_states"], cross_attention_kwargs=None,
                       added_cond_kwargs=cond, return_dict=False)[0].clone()
    m = _model(dtype, gpu)
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu, freeu=True)
    base = call(unet)
    assert torch.equal(base, call(unet))                       # (the second call replays the captured graph)
    unet.enable_freeu(V["s1"], V["s2"], V["b1"], V["b2"])     # diffusers' positional order
    on = call(unet)
    assert not torch.equal(on, base) and torch.equal(on, call(unet))
    err = float((on.double().cpu() - _ref_step(m, x, dtype, 300.0, 1)).abs().max())
    print(f"diffusers hook, tiny fp32, FreeU v1: {err:.2e}")
    assert err <= 1e-3
    unet.disable_freeu()
    assert torch.equal(call(unet), base)
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, dtype, gpu)
    with pytest.raises(ValueError, match="freeu=True"):
        plain.enable_freeu(0.9, 0.2, 1.3, 1.4)
    with pytest.raises(ValueError, match="freeu=True"):
        plain.disable_freeu()


def test_comfy_hook_version_2(gpu):
    dtype = torch.float32
    m = _model(dtype, gpu)
    adapter = hooks.compile_comfy_unet(m, freeu=True)
    assert adapter.compiled.rewrite_stats["freeu_sites"] == 6
    x = _inputs()
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    with torch.no_grad():
        y = torch.cat([xg["text_embeds"], m.add_time_proj(xg["time_ids"].flatten()).reshape(2, -1).to(dtype)], dim=-1)
    call = lambda a: a(xg["latent"], timesteps=torch.full((2,), 300.0, device=gpu), context=xg["encoder_hidden_states"], y=y).clone()
    base = call(adapter)
    adapter.enable_freeu(**V, version=2)
    on = call(adapter)
    assert not torch.equal(on, base) and torch.equal(on, call(adapter))
    err = float((on.double().cpu() - _ref_step(m, x, dtype, 300.0, 2)).abs().max())
    print(f"comfy hook, tiny fp32, FreeU v2: {err:.2e}")
    assert err <= 1e-3
    adapter.disable_freeu()
    assert torch.equal(call(adapter), base)
    with pytest.raises(ValueError, match="freeu=True"):
        hooks.compile_comfy_unet(m).enable_freeu(**V, version=2)
