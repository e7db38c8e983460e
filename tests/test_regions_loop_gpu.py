"""Regional prompts in the captured denoise loop and behind the hooks, on the TINY network: latent 16, bf16, 4 Euler steps unless
stated, R = 2 prompts of 77 tokens (tests/regions_util.py: synth's two prompts, left / right masks)."""
import functools

import pytest
import torch

from stabletriton_amd import hooks, regions, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import regions_util as RU

pytestmark = pytest.mark.gpu
DTYPE = torch.bfloat16
R, L, HW, STEPS = 2, 77, 16, 4
G = 5.0


def _model(dev, dtype=DTYPE):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


@functools.lru_cache(maxsize=None)
def _compiled(with_regions, pag_layers=None, dtype=DTYPE):
    return optimize_model(_model(torch.device("cuda:0"), dtype), cuda_graph=False, pag_layers=pag_layers, regions=R if with_regions else None,
                          region_tokens=L)


@functools.lru_cache(maxsize=None)
def _inputs():
    """Row 0: the negative conditioning, row 1: the positive one; `both`: the two prompts side by side, (2, 154, cross)."""
    x = synth.denoise_inputs(2, HW, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    x["both"] = RU.two_prompts(2, L, TINY.cross_dim)
    return x


def _loop(gm, dev, ehs, tables=None, guided=False, neg_ehs=None, dtype=DTYPE, **kw):
    """A loop over `gm` on the positive row's conditioning with the text state `ehs` (1, tokens, cross)."""
    x = _inputs()
    if guided:
        kw["guidance_scale"] = G
    loop = DenoiseLoop(gm, 1, HW, dtype, dev, tables or euler_discrete_tables(STEPS), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim,
                       tokens=ehs.shape[1], **kw)
    to = lambda t: t.to(dev, dtype)
    if guided:
        loop.set_conditioning(to(ehs), to(x["text_embeds"][1:2]), to(x["time_ids"][1:2]),
                              to(x["encoder_hidden_states"][0:1] if neg_ehs is None else neg_ehs), to(x["text_embeds"][0:1]), to(x["time_ids"][0:1]))
    else:
        loop.set_conditioning(to(ehs), to(x["text_embeds"][1:2]), to(x["time_ids"][1:2]))
    return loop


def _noise():
    return _inputs()["latent"][:1]


# ------------------------------------------------------------------------------------------------ compiled in, off
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("guided", [False, True])
def test_off_is_the_loop_without_regions_on_the_first_prompt(gpu, guided, dtype):
    """(TINY's cross-attentions have 64 and 16 queries, so both modules take the two-launch route there; the fused launch against
    the regional pair is tests/test_regions_gpu.py::test_off_pair_is_the_fused_query_projection_and_attention.)"""
    both = _inputs()["both"][1:2]
    plain_gm, gm = _compiled(False, None, dtype), _compiled(True, None, dtype)
    with torch.no_grad():
        plain = _loop(plain_gm, gpu, both[:, :L], guided=guided, dtype=dtype).denoise(_noise())
        off = _loop(gm, gpu, both, guided=guided, dtype=dtype).denoise(_noise())
    assert gm.rewrite_stats["region_sites"] == 17
    assert torch.isfinite(off).all()
    assert torch.equal(off, plain), f"off differs from the plain loop: max abs {float((off - plain).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ left / right masks
def test_left_right_masks_against_the_cpu_run_of_the_traced_module(gpu):
    """The regional GPU latent against the fp32 CPU run of the same traced module (the bf16 model's weights and inputs, widened),
    allowed 1.5 x the deviation measured here between the plain loop and ITS CPU run at the same shape: both deviations are the
    bf16 arithmetic of the same network, and the regional sum adds one fp32 multiply-add per segment before the same single
    rounding - the margin covers the run-to-run spread of a maximum over 1024 values, not a second error source."""
    x = _inputs()
    both = x["both"][1:2]
    first, second = both[:, :L], both[:, L:]
    tables = euler_discrete_tables(STEPS)
    masks = RU.left_right_masks(HW, HW)
    with torch.no_grad():
        plain_a = _loop(_compiled(False), gpu, first).denoise(_noise()).cpu()
        plain_b = _loop(_compiled(False), gpu, second).denoise(_noise()).cpu()
        loop = _loop(_compiled(True), gpu, both)
        loop.set_regions(masks)
        got = loop.denoise(_noise()).cpu()
        loop.set_regions(None)
    # the CPU side: the same weights (bf16 values in fp32), the same bf16-rounded conditioning
    m32 = _model(torch.device("cpu")).float()
    wide = lambda t: t.to(DTYPE).float()
    te, ti = wide(x["text_embeds"][1:2]), wide(x["time_ids"][1:2])
    cpu_plain, _ = RU.traced_cpu(m32)
    cpu_regions, sites = RU.traced_cpu(m32, R, L)
    assert sites == 17
    cpu_regions.regions.bind(1, HW, "cpu")
    cpu_regions.regions.set(masks, [0])
    ref_plain = RU.euler_loop_cpu(cpu_plain, tables, _noise(), wide(first), te, ti)
    ref = RU.euler_loop_cpu(cpu_regions, tables, _noise(), wide(both), te, ti)
    dev_plain = float((plain_a - ref_plain).abs().max())
    dev = float((got - ref).abs().max())
    da, db = float((got - plain_a).abs().max()), float((got - plain_b).abs().max())
    msg = (f"regional loop vs its CPU fp32 run: max abs {dev:.4e}; plain loop vs its CPU fp32 run: {dev_plain:.4e} (allowed 1.5 x = "
           f"{1.5 * dev_plain:.4e}); |ref| max {float(ref.abs().max()):.3f}; distance to the single-prompt latents {da:.3e} / {db:.3e}")
    print(msg)
    assert torch.isfinite(got).all()
    assert da > 10 * dev_plain and db > 10 * dev_plain, "the regional latent must differ from both single-prompt latents: " + msg
    assert dev <= 1.5 * dev_plain, msg


# ------------------------------------------------------------------------------------------------ in place, no new capture
def test_set_regions_after_capture_needs_no_new_capture(gpu):
    both = _inputs()["both"][1:2]
    with torch.no_grad():
        loop = _loop(_compiled(True), gpu, both, guided=True)
        off = loop.denoise(_noise())
        graph = loop.graph
        assert graph is not None
        loop.set_regions(RU.left_right_masks(HW, HW))
        on = loop.denoise(_noise())
        assert loop.graph is graph and not torch.equal(on, off) and torch.isfinite(on).all()
        assert torch.equal(loop.denoise(_noise()), on), "two replays must repeat their bits"
        loop.set_regions(RU.left_right_masks(HW, HW).flip(0))
        swapped = loop.denoise(_noise())
        assert loop.graph is graph and not torch.equal(swapped, on)
        loop.set_regions(None)
        assert torch.equal(loop.denoise(_noise()), off) and loop.graph is graph, "clearing restores the off bits"
        # before capture() is as legal as after it
        early = _loop(_compiled(True), gpu, both, guided=True)
        early.set_regions(RU.left_right_masks(HW, HW))
        assert early.graph is None and torch.equal(early.denoise(_noise()), on)
        early.set_regions(None)
    # a negative prompt per segment is taken as it is: the negative rows keep segment 0, so its second segment does not matter
    with torch.no_grad():
        neg = _inputs()["encoder_hidden_states"][0:1]
        wide_neg = _loop(_compiled(True), gpu, both, guided=True, neg_ehs=torch.cat([neg, both[:, L:]], dim=1))
        assert torch.equal(wide_neg.denoise(_noise()), off)


def test_with_pag_and_with_the_sde_sampler(gpu):
    both = _inputs()["both"][1:2]
    masks = RU.left_right_masks(HW, HW)
    gm = _compiled(True, ("mid",))
    assert gm.rewrite_stats["region_sites"] == 17 and gm.rewrite_stats["pag_sites"] == 2
    with torch.no_grad():
        loop = _loop(gm, gpu, both, guided=True, pag_scale=3.0)
        assert loop.x_in.shape[0] == 3
        off = loop.denoise(_noise())
        loop.set_regions(masks)
        w = gm.regions.weights_for(3, 64)
        assert w[0, 0].min() == 1.0 and torch.equal(w[1], w[2]) and float(w[1, 1].max()) == 1.0, "negative: segment 0; perturbed: the positive weights"
        on = loop.denoise(_noise())
        assert torch.isfinite(on).all() and not torch.equal(on, off) and torch.equal(loop.denoise(_noise()), on)
        loop.set_regions(None)
        sde = _loop(_compiled(True), gpu, both, tables=dpmpp_2m_sde_tables(STEPS), guided=True)
        sde.set_seed(77)
        sde.set_regions(masks)
        out = sde.denoise(_noise())
        assert torch.isfinite(out).all() and torch.equal(sde.denoise(_noise()), out)
        sde.set_regions(None)
        assert not torch.equal(sde.denoise(_noise()), out)


def test_errors(gpu):
    both = _inputs()["both"][1:2]
    with pytest.raises(ValueError, match="tokens=154"):
        _loop(_compiled(True), gpu, both[:, :L])
    with pytest.raises(ValueError, match="regions=R"):
        _loop(_compiled(False), gpu, both[:, :L]).set_regions(RU.left_right_masks(HW, HW))
    loop = _loop(_compiled(True), gpu, both)
    for bad in (torch.zeros(R, 8, 8), torch.zeros(3, HW, HW), torch.full((R, HW, HW), -1.0)):
        with pytest.raises(ValueError):
            loop.set_regions(bad)
    with pytest.raises(ValueError, match="fp8"):
        optimize_model(_model(gpu), cuda_graph=False, fp8=True, regions=R)


# ------------------------------------------------------------------------------------------------ hooks
def test_diffusers_hook_set_and_clear(gpu):
    """The duck-typed Diffusers call (tests/test_hooks_gpu.py): batch [uncond | cond], the two prompts side by side."""
    x = _inputs()
    m = _model(gpu)
    ehs = torch.cat([torch.cat([x["encoder_hidden_states"][0:1]] * R, dim=1), x["both"][1:2]]).to(gpu, DTYPE)      # (2, 154, cross)
    lat = x["latent"][:1].repeat(2, 1, 1, 1).to(gpu, DTYPE)
    cond = {"text_embeds": x["text_embeds"].to(gpu, DTYPE), "time_ids": x["time_ids"].to(gpu, DTYPE)}
    call = lambda u, e: u(lat, torch.tensor(300.0), encoder_hidden_states=e, cross_attention_kwargs=None, added_cond_kwargs=cond,
                          return_dict=False)[0].clone()
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DTYPE, gpu)
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DTYPE, gpu, regions=R, region_tokens=L)
    base = call(plain, ehs[:, :L].contiguous())
    off = call(unet, ehs)
    assert torch.equal(off, base), "off: the wrapper compiled without regions on the first prompt"
    assert torch.equal(off, call(unet, ehs))                      # (the second call replays the captured graph)
    step_fn = next(iter(unet._steps.values()))
    unet.set_regions(RU.left_right_masks(HW, HW), 2)
    on = call(unet, ehs)
    assert len(step_fn._cached) == 1, "an in-place write: the captured graph stays"
    assert torch.equal(on[0], off[0]), "the uncond row keeps segment 0"
    assert not torch.equal(on[1], off[1]) and torch.isfinite(on).all() and torch.equal(on, call(unet, ehs))
    unet.set_regions(RU.left_right_masks(HW, HW), 1)              # every row takes the masks: the cond row's weights are the same
    assert torch.equal(call(unet, ehs)[1], on[1])
    unet.set_regions(RU.left_right_masks(HW // 2, HW // 2), 2)    # masks of another size than the call's latent
    with pytest.raises(ValueError, match="latent"):
        call(unet, ehs)
    unet.clear_regions()
    assert torch.equal(call(unet, ehs), off) and len(step_fn._cached) == 1
    # a wrapper that sets nothing writes nothing: weights another owner of the compiled module set stay
    unet.compiled.regions.set(RU.left_right_masks(HW, HW), [1], 2)
    assert torch.equal(call(unet, ehs), on)
    unet.clear_regions()
    with pytest.raises(ValueError, match="regions=R"):
        plain.set_regions(RU.left_right_masks(HW, HW), 2)
    with pytest.raises(ValueError, match="regions=R"):
        plain.clear_regions()
    with pytest.raises(ValueError, match="chunks"):
        unet.set_regions(RU.left_right_masks(HW, HW), 0)
    with pytest.raises(ValueError, match="masks"):
        unet.set_regions(torch.zeros(3, HW, HW), 2)
