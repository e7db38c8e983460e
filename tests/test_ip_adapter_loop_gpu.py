"""IP-Adapter in the captured denoise loop and behind the hooks, on the TINY network: latent 16, bf16, 4 Euler steps unless stated,
one adapter of 4 image tokens unless stated (tests/ip_adapter_util.py: a synthetic checkpoint and synthetic image tokens)."""
import functools

import pytest
import torch

from stabletriton_amd import hooks, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import ip_adapter_util as IU
from tests import regions_util as RU

pytestmark = pytest.mark.gpu
DTYPE = torch.bfloat16
N, HW, STEPS = 4, 16, 4
G = 5.0


def _model(dev, dtype=DTYPE):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


@functools.lru_cache(maxsize=None)
def _compiled(ip, pag_layers=None, dtype=DTYPE):
    return optimize_model(_model(torch.device("cuda:0"), dtype), cuda_graph=False, pag_layers=pag_layers, ip_adapter=ip)


@functools.lru_cache(maxsize=None)
def _inputs():
    """Row 0: the negative conditioning, row 1: the positive one."""
    return synth.denoise_inputs(2, HW, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


def _loop(gm, dev, tables=None, guided=False, dtype=DTYPE, **kw):
    x = _inputs()
    if guided:
        kw["guidance_scale"] = G
    loop = DenoiseLoop(gm, 1, HW, dtype, dev, tables or euler_discrete_tables(STEPS), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, **kw)
    to = lambda t: t.to(dev, dtype)
    if guided:
        loop.set_conditioning(to(x["encoder_hidden_states"][1:2]), to(x["text_embeds"][1:2]), to(x["time_ids"][1:2]),
                              to(x["encoder_hidden_states"][0:1]), to(x["text_embeds"][0:1]), to(x["time_ids"][0:1]))
    else:
        loop.set_conditioning(to(x["encoder_hidden_states"][1:2]), to(x["text_embeds"][1:2]), to(x["time_ids"][1:2]))
    return loop


def _noise():
    return _inputs()["latent"][:1]


def _adapter(gm, n=N, seed=5, **kw):
    return IU.checkpoint(gm.ip_adapter, n, seed=seed, **kw)[0]


def _tokens(n=N, seed=91):
    return IU.image_tokens(1, n, TINY.cross_dim, seed)


def _all_off(gm):
    for a in range(gm.ip_adapter.slots):
        gm.ip_adapter.unload(a)


# ------------------------------------------------------------------------------------------------ compiled in, off
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("guided", [False, True])
def test_off_is_the_loop_without_the_pass(gpu, guided, dtype):
    plain_gm, gm = _compiled(None, None, dtype), _compiled(N, None, dtype)
    assert gm.rewrite_stats["ip_adapter_sites"] == 17
    with torch.no_grad():
        plain = _loop(plain_gm, gpu, guided=guided, dtype=dtype).denoise(_noise())
        loop = _loop(gm, gpu, guided=guided, dtype=dtype)
        off = loop.denoise(_noise())
        assert torch.isfinite(off).all()
        assert torch.equal(off, plain), f"nothing loaded: differs from the plain loop by {float((off - plain).abs().max()):.3e}"
        loop.load_ip_adapter(_adapter(gm))
        loop.set_ip_adapter_image(_tokens())
        assert float(gm.ip_adapter.kv_for(loop.x_in.shape[0], 0, 0).abs().max()) > 0
        loaded = loop.denoise(_noise())
        assert torch.equal(loaded, plain), "loaded, image set, scale 0: the sites skip the image segment"
        _all_off(gm)


# ------------------------------------------------------------------------------------------------ on, against the CPU run
def test_scale_06_against_the_cpu_run_of_the_traced_module(gpu):
    """The GPU latent with the adapter at scale 0.6 against the fp32 CPU run of the same traced module (the bf16 model's weights,
    adapter weights and inputs, widened), allowed 1.5 x the deviation measured here between the plain loop and ITS CPU run at the
    same shape - the protocol of tests/test_regions_loop_gpu.py: both deviations are the bf16 arithmetic of the same network, the
    image term adds one fp32 multiply-add per segment before the same single rounding."""
    x = _inputs()
    tables = euler_discrete_tables(STEPS)
    gm = _compiled(N)
    sd, tok = _adapter(gm), _tokens()
    with torch.no_grad():
        plain = _loop(_compiled(None), gpu).denoise(_noise()).cpu()
        loop = _loop(gm, gpu)
        loop.load_ip_adapter(sd)
        loop.set_ip_adapter_image(tok)
        loop.set_ip_adapter_scale(0.6)
        got = loop.denoise(_noise()).cpu()
        _all_off(gm)
    m32 = _model(torch.device("cpu")).float()
    wide = lambda t: t.to(DTYPE).float()
    ehs, te, ti = wide(x["encoder_hidden_states"][1:2]), wide(x["text_embeds"][1:2]), wide(x["time_ids"][1:2])
    cpu_plain, _ = IU.traced_cpu(m32)
    cpu_ip, sites = IU.traced_cpu(m32, N)
    assert sites == 17
    st = cpu_ip.ip_adapter
    st.bind(1, HW, "cpu")
    st.load({"ip_adapter": {k: wide(v) for k, v in sd["ip_adapter"].items()}}, 0)
    st.set_image(wide(tok), None, 0, 1)
    st.set_scale(0.6, 0)
    ref_plain = RU.euler_loop_cpu(cpu_plain, tables, _noise(), ehs, te, ti)
    ref = RU.euler_loop_cpu(cpu_ip, tables, _noise(), ehs, te, ti)
    dev_plain = float((plain - ref_plain).abs().max())
    dev = float((got - ref).abs().max())
    dist = float((got - plain).abs().max())
    msg = (f"IP-Adapter loop vs its CPU fp32 run: max abs {dev:.4e}; plain loop vs its CPU fp32 run: {dev_plain:.4e} (allowed 1.5 x = "
           f"{1.5 * dev_plain:.4e}); |ref| max {float(ref.abs().max()):.3f}; distance to the plain latent {dist:.3e}")
    print(msg)
    assert torch.isfinite(got).all()
    assert dist > 10 * dev_plain, "the image prompt must move the latent: " + msg
    assert dev <= 1.5 * dev_plain, msg


# ------------------------------------------------------------------------------------------------ in place, no new capture
def test_every_call_after_capture_needs_no_new_capture(gpu):
    gm = _compiled(N)
    sd, tok = _adapter(gm), _tokens()
    left = RU.left_right_masks(HW, HW)[0]
    with torch.no_grad():
        loop = _loop(gm, gpu, guided=True)
        off = loop.denoise(_noise())
        graph = loop.graph
        assert graph is not None
        loop.load_ip_adapter(sd)
        loop.set_ip_adapter_image(tok)
        loop.set_ip_adapter_scale(0.6)
        on = loop.denoise(_noise())
        assert loop.graph is graph and not torch.equal(on, off) and torch.isfinite(on).all()
        assert torch.equal(loop.denoise(_noise()), on), "two replays must repeat their bits"
        loop.set_ip_adapter_masks(left)
        masked = loop.denoise(_noise())
        assert loop.graph is graph and not torch.equal(masked, on)
        loop.set_ip_adapter_masks(None)
        assert torch.equal(loop.denoise(_noise()), on), "masks None restores"
        loop.set_ip_adapter_scale(0)
        assert torch.equal(loop.denoise(_noise()), off) and loop.graph is graph, "scale 0 restores the off bits"
        loop.set_ip_adapter_scale(0.6)
        assert torch.equal(loop.denoise(_noise()), on)
        loop.unload_ip_adapter()
        assert torch.equal(loop.denoise(_noise()), off) and loop.graph is graph, "unload restores the off bits"
        # before capture() is as legal as after it
        early = _loop(gm, gpu, guided=True)
        early.load_ip_adapter(sd)
        early.set_ip_adapter_image(tok)
        early.set_ip_adapter_scale(0.6)
        assert early.graph is None and torch.equal(early.denoise(_noise()), on)
        # negative tokens reach the negative block; the default is zero tokens
        early.set_ip_adapter_image(tok, tok)
        both = early.denoise(_noise())
        assert not torch.equal(both, on) and torch.isfinite(both).all()
        _all_off(gm)


def test_per_site_scales(gpu):
    gm = _compiled(N)
    with torch.no_grad():
        loop = _loop(gm, gpu)
        off = loop.denoise(_noise())
        loop.load_ip_adapter(_adapter(gm))
        loop.set_ip_adapter_image(_tokens())
        loop.set_ip_adapter_scale(0.6)
        everywhere = loop.denoise(_noise())
        loop.set_ip_adapter_scale({"mid": 0.6})
        mid = loop.denoise(_noise())
        assert gm.ip_adapter.scales[:, 1].tolist() == pytest.approx([0.0] * 6 + [0.6] * 2 + [0.0] * 9)
        assert not torch.equal(mid, everywhere) and not torch.equal(mid, off) and torch.isfinite(mid).all()
        loop.set_ip_adapter_scale({".*": 0})
        assert torch.equal(loop.denoise(_noise()), off)
        _all_off(gm)


def test_two_slots_and_masks(gpu):
    gm = _compiled((4, 16))
    assert gm.ip_adapter.tokens == (4, 16)
    masks = RU.left_right_masks(HW, HW)
    with torch.no_grad():
        loop = _loop(gm, gpu, guided=True)
        off = loop.denoise(_noise())
        loop.load_ip_adapter(_adapter(gm, 4, 5), 0)
        loop.load_ip_adapter(_adapter(gm, 16, 9), 1)
        loop.set_ip_adapter_image(_tokens(4, 91), slot=0)
        loop.set_ip_adapter_image(_tokens(16, 92), slot=1)
        loop.set_ip_adapter_scale(0.6, 0)
        first = loop.denoise(_noise())
        loop.set_ip_adapter_scale(0.5, 1)
        both = loop.denoise(_noise())
        assert not torch.equal(first, off) and not torch.equal(both, first) and torch.isfinite(both).all()
        loop.set_ip_adapter_masks(masks[0], 0)
        loop.set_ip_adapter_masks(masks[1], 1)
        split = loop.denoise(_noise())
        w = gm.ip_adapter.weights_for(2, 64)
        assert float(w[:, 0].min()) == 1.0 and torch.equal(w[0], w[1]) and float((w[0, 1] + w[0, 2]).min()) == 1.0 == float((w[0, 1] + w[0, 2]).max())
        assert not torch.equal(split, both) and torch.isfinite(split).all() and torch.equal(loop.denoise(_noise()), split)
        loop.set_ip_adapter_masks(None, 0)
        loop.set_ip_adapter_masks(None, 1)
        assert torch.equal(loop.denoise(_noise()), both), "masks None restores"
        loop.unload_ip_adapter(1)
        assert torch.equal(loop.denoise(_noise()), first)
        loop.unload_ip_adapter(0)
        assert torch.equal(loop.denoise(_noise()), off)
        with pytest.raises(ValueError, match="slot"):
            loop.set_ip_adapter_scale(1.0, 2)
        with pytest.raises(ValueError, match=r"\(B or 1, N, cross_dim\)"):
            loop.set_ip_adapter_image(_tokens(16), slot=0)
        with pytest.raises(ValueError, match="latent resolution"):
            loop.set_ip_adapter_masks(torch.ones(8, 8), 0)


def test_with_pag_and_with_the_sde_sampler(gpu):
    gm = _compiled(N, ("mid",))
    assert gm.rewrite_stats["ip_adapter_sites"] == 17 and gm.rewrite_stats["pag_sites"] == 2
    sd, tok, neg = _adapter(gm), _tokens(), _tokens(seed=93)
    with torch.no_grad():
        loop = _loop(gm, gpu, guided=True, pag_scale=3.0)
        assert loop.x_in.shape[0] == 3
        off = loop.denoise(_noise())
        loop.load_ip_adapter(sd)
        loop.set_ip_adapter_image(tok, neg)
        loop.set_ip_adapter_scale(0.6)
        kv = gm.ip_adapter.kv_for(3, 7, 0)
        assert torch.equal(kv[1], kv[2]) and not torch.equal(kv[0], kv[1]), "negative: the negative tokens; perturbed: the positive ones"
        on = loop.denoise(_noise())
        assert torch.isfinite(on).all() and not torch.equal(on, off) and torch.equal(loop.denoise(_noise()), on)
        # [positive | perturbed] without guidance: no negative block, both take the tokens
        unguided = _loop(gm, gpu, pag_scale=3.0)
        unguided.set_ip_adapter_image(tok)
        kv2 = gm.ip_adapter.kv_for(2, 7, 0)
        assert torch.equal(kv2[0], kv2[1]) and torch.equal(kv2[0], kv[1])
        with pytest.raises(ValueError, match="negative row block"):
            unguided.set_ip_adapter_image(tok, neg)
        _all_off(gm)
        gm2 = _compiled(N)
        sde = _loop(gm2, gpu, tables=dpmpp_2m_sde_tables(STEPS), guided=True)
        sde.set_seed(77)
        plain = sde.denoise(_noise())
        sde.load_ip_adapter(_adapter(gm2))
        sde.set_ip_adapter_image(tok)
        sde.set_ip_adapter_scale(0.6)
        out = sde.denoise(_noise())
        assert torch.isfinite(out).all() and torch.equal(sde.denoise(_noise()), out) and not torch.equal(out, plain)
        _all_off(gm2)


def test_errors(gpu):
    with pytest.raises(ValueError, match="ip_adapter=N"):
        _loop(_compiled(None), gpu).set_ip_adapter_scale(0.5)
    with pytest.raises(ValueError, match="ip_adapter=N"):
        _loop(_compiled(None), gpu).load_ip_adapter({})
    with pytest.raises(ValueError, match="fp8"):
        optimize_model(_model(gpu), cuda_graph=False, fp8=True, ip_adapter=N)
    with pytest.raises(ValueError, match="regions"):
        optimize_model(_model(gpu), cuda_graph=False, regions=2, ip_adapter=N)


# ------------------------------------------------------------------------------------------------ hooks
def test_diffusers_hook_set_and_clear(gpu):
    """The duck-typed Diffusers call (tests/test_hooks_gpu.py): batch [uncond | cond]."""
    x = _inputs()
    m = _model(gpu)
    ehs = x["encoder_hidden_states"].to(gpu, DTYPE)
    lat = x["latent"][:1].repeat(2, 1, 1, 1).to(gpu, DTYPE)
    cond = {"text_embeds": x["text_embeds"].to(gpu, DTYPE), "time_ids": x["time_ids"].to(gpu, DTYPE)}
    call = lambda u: u(lat, torch.tensor(300.0), encoder_hidden_states=ehs, cross_attention_kwargs=None, added_cond_kwargs=cond,
                       return_dict=False)[0].clone()
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DTYPE, gpu)
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DTYPE, gpu, ip_adapter=N)
    base = call(plain)
    unet.load_ip_adapter(_adapter(unet.compiled))            # before the first call: nothing is bound yet
    unet.set_ip_adapter_image(_tokens(), chunks=2)
    off = call(unet)
    assert torch.equal(off, base), "scale 0: the wrapper compiled without the pass"
    assert torch.equal(off, call(unet))                      # (the second call replays the captured graph)
    step_fn = next(iter(unet._steps.values()))
    unet.set_ip_adapter_scale(0.6)
    on = call(unet)
    assert len(step_fn._cached) == 1, "an in-place write: the captured graph stays"
    assert torch.equal(on[0], off[0]), "the uncond row takes zero tokens: no contribution"
    assert not torch.equal(on[1], off[1]) and torch.isfinite(on).all() and torch.equal(on, call(unet))
    unet.set_ip_adapter_image(_tokens(), _tokens(), chunks=2)
    neg = call(unet)
    assert not torch.equal(neg[0], off[0]) and torch.equal(neg[1], on[1]), "negative_tokens = tokens on the uncond row differs from the default"
    unet.set_ip_adapter_image(_tokens(), chunks=1)           # every row takes the tokens: the same K/V as above
    assert torch.equal(call(unet), neg)
    unet.set_ip_adapter_image(_tokens(), chunks=2)
    unet.set_ip_adapter_masks(RU.left_right_masks(HW, HW)[0])
    masked = call(unet)
    assert not torch.equal(masked[1], on[1]) and torch.equal(masked[0], off[0]) and len(step_fn._cached) == 1
    unet.set_ip_adapter_masks(torch.ones(HW // 2, HW // 2))
    with pytest.raises(ValueError, match="latent"):
        call(unet)
    unet.set_ip_adapter_masks(None)
    assert torch.equal(call(unet), on)
    unet.unload_ip_adapter()
    assert torch.equal(call(unet), off) and len(step_fn._cached) == 1
    for fn in (lambda: plain.load_ip_adapter({}), lambda: plain.set_ip_adapter_image(_tokens()), lambda: plain.set_ip_adapter_scale(1.0),
               lambda: plain.set_ip_adapter_masks(None), lambda: plain.unload_ip_adapter()):
        with pytest.raises(ValueError, match="ip_adapter=N"):
            fn()
    with pytest.raises(ValueError, match="N = 4 tokens"):
        unet.set_ip_adapter_image(_tokens(16))
    with pytest.raises(ValueError, match="chunks"):
        unet.set_ip_adapter_image(_tokens(), chunks=0)
    with pytest.raises(ValueError, match="regions"):
        hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DTYPE, gpu, regions=2, ip_adapter=N)
