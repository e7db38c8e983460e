"""Self-attention guidance in the denoise loop, on the TINY network (latent 16, 3 steps): what must be bit-equal is, and one eager
step is the float64 composition of its own parts."""
import functools

import pytest
import torch

from stabletriton_amd import sag, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3           # the loop tests' gate for this network in fp32 (tests/test_pag_loop_gpu.py)
G = 5.0
TABLES = {"euler": lambda: euler_discrete_tables(3), "dpmpp": lambda: dpmpp_2m_tables(3, karras=True), "sde": lambda: dpmpp_2m_sde_tables(3)}
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _compiled(dtype, sag_layer=True):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(DEV, dtype)
    synth.fill_module_(m, 0)
    return optimize_model(m, cuda_graph=False, sag_layer=sag_layer)


@functools.lru_cache(maxsize=None)
def _inputs():
    return synth.denoise_inputs(4, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


def _loop(gm, dtype, sampler="euler", mode="loop", batch=2, **kw):
    x = _inputs()
    loop = DenoiseLoop(gm, batch, 16, dtype, DEV, TABLES[sampler](), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode,
                       guidance_scale=G, **kw)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    loop.set_conditioning(*(x[k][batch:2 * batch].to(DEV, dtype) for k in keys), *(x[k][:batch].to(DEV, dtype) for k in keys))
    return loop


def _run(loop, batch=2):
    with torch.no_grad():
        return loop.denoise(_inputs()["latent"][:batch], seed=11).cpu()


@pytest.mark.parametrize("sampler", ["euler", "dpmpp", "sde"])
def test_scale_zero_is_the_loop_without_sag_and_capture_is_eager(gpu, sampler):
    gm = _compiled(torch.bfloat16)
    plain = _run(_loop(gm, torch.bfloat16, sampler))
    assert torch.equal(_run(_loop(gm, torch.bfloat16, sampler, sag_scale=0.0)), plain), "sag_scale = 0 differs from the loop without it"
    loop = _loop(gm, torch.bfloat16, sampler, sag_scale=0.5)
    on = _run(loop)
    assert torch.equal(on, _run(loop)), "a replay must repeat its bits"
    assert torch.equal(on, _run(_loop(gm, torch.bfloat16, sampler, mode="eager", sag_scale=0.5))), "captured differs from eager"
    assert torch.isfinite(on).all() and not torch.equal(on, plain)
    assert gm.sag.rows == 0, "the loop names the recording rows around its own calls only"
    mask = gm.sag.mask
    assert mask.shape == (2, 16, 16) and bool(((mask == 0) | (mask == 1)).all())


def test_a_unet_with_the_site_in_a_plain_loop_gives_the_bits_of_one_without(gpu):
    assert torch.equal(_run(_loop(_compiled(torch.bfloat16), torch.bfloat16)), _run(_loop(_compiled(torch.bfloat16, None), torch.bfloat16)))


def test_one_eager_step_is_the_float64_composition_of_its_parts(gpu):
    """fp32: the UNet through the loop's own calls at 2B and at B rows, steps 2 and 4 of sag.py's docstring in float64 with the mask
    the kernel wrote (no threshold flip to argue about), the Euler update in float64."""
    gm, s = _compiled(torch.float32), 0.5
    loop = _loop(gm, torch.float32, mode="eager", sag_scale=s)
    with torch.no_grad():
        loop.set_noise(_inputs()["latent"][:2])
        x, x_in = loop.latent.double(), loop.x_in.clone()
        loop.run_steps(1)
        got, mask = loop.latent.double(), gm.sag.mask.clone()
        assert 0.0 < float(mask.mean()) < 1.0, "a mask of one value would leave the blur or the selection untested"
        loop.x_in.copy_(x_in)
        rows, step = loop._time_rows(lambda tbl: tbl[0]), loop.step_ids[0:1]
        eps = loop._unet(loop.timesteps[0], rows[0], step).double()
        e_neg, e_pos = eps[:2], eps[2:]
        sigma, sc, ds = float(loop.tables.sigmas[0]), float(loop.in_scale[0]), float(loop.dsigma[0])
        second, ref_mask = sag.degrade_reference(x, e_neg, mask.reshape(2, -1), (16, 16), sigma, sc, 0.5, gm.sag.sigma)
        assert torch.equal(ref_mask.float(), mask)
        loop.x_sag.copy_(second)
        e_sag = loop._unet(loop.timesteps[0], rows[1], step, second=True).double()
    want = x + (e_neg + G * (e_pos - e_neg) + s * (e_neg - e_sag)) * ds
    err = float((got - want).abs().max())
    moved = float((s * (e_neg - e_sag) * ds).abs().max())
    print(f"one SAG step fp32: max abs err vs the float64 composition {err:.2e}; the SAG term moves the latent by {moved:.2e}")
    assert moved > 10 * ABS_TOL_STRICT, "the SAG term must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


def test_set_sag_needs_no_recapture(gpu):
    gm = _compiled(torch.bfloat16)
    loop = _loop(gm, torch.bfloat16, sag_scale=0.5)
    base = _run(loop)
    graph = loop.graph
    assert graph is not None
    for kw in (dict(scale=1.5), dict(sigma=0.7), dict(threshold=0.9)):
        loop.set_sag(**{"scale": 0.5, "sigma": 2.0, "threshold": 1.0, **kw})
        fresh = _loop(gm, torch.bfloat16, mode="eager", sag_scale=kw.get("scale", 0.5), sag_sigma=kw.get("sigma", 2.0),
                      sag_threshold=kw.get("threshold", 1.0))
        out = _run(loop)
        assert loop.graph is graph, "set_sag must not drop the captured graph"
        assert not torch.equal(out, base), f"{kw} changed nothing"
        assert torch.equal(out, _run(fresh)), f"{kw}: the captured loop differs from a loop built with these values"
    loop.set_sag(scale=0.5, sigma=2.0, threshold=1.0)
    assert torch.equal(_run(loop), base)
