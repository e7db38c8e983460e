"""Masked inpainting in the captured denoise loop, on the TINY network in fp32: 10-step schedules, g = 5, latent 16 x 16 (tiled: canvas
16 x 24), start noise from torch.Generator().manual_seed(99), the init latent and the masks from tests/inpaint_util.py, prompts from
synth.denoise_inputs(2, 16, 1234) (row 0 the negative prompt, row 1 the prompt).

"Off" (no set_inpaint, set_inpaint(None), a mask of ones) is compared bit for bit with a loop built without the flag; a kept pixel
ends on the init latent bit for bit; everything else is compared with the tests' own float64 loop around the eager CPU module
(tests/inpaint_util.py) under the project's gate for this network and schedule, ABS_TOL_STRICT.  tests/test_inpaint_host.py shows in
float64 that a wrong blend (the known region one sigma late) ends 3.85 from the right one, far outside that gate."""
import functools

import pytest
import torch

from stabletriton_amd import inpaint as I, synth, tiles as T
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_ancestral_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import inpaint_util as IU
from tests import tiles_util as TU

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
G = 5.0
N = 10
HW = (16, 16)
KEYS = ("encoder_hidden_states", "text_embeds", "time_ids")
TABLES = {"euler": euler_discrete_tables, "dpmpp": dpmpp_2m_tables, "euler_a": euler_ancestral_tables, "dpmpp_sde": dpmpp_2m_sde_tables}


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
    return synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _compiled(**kw):
    return optimize_model(_model(torch.float32, torch.device("cuda:0")), cuda_graph=False, **kw)


def _loop(gm, dev, hw=HW, mode="loop", sampler="euler", **kw):
    x = _inputs()
    kw.setdefault("guidance_scale", G)
    loop = DenoiseLoop(gm, 1, hw, torch.float32, dev, TABLES[sampler](N), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode, **kw)
    loop.set_conditioning(*(x[k][1:2].to(dev) for k in KEYS), *(x[k][0:1].to(dev) for k in KEYS))
    return loop


@functools.lru_cache(maxsize=None)
def _ref(sampler="euler", mask="half", differential=False, tiled=False):
    """The float64 loop, once per configuration."""
    hw = (16, 24) if tiled else HW
    tiles = None
    if tiled:
        tiles = (TU.starts(16, 16, 8), TU.starts(24, 16, 8), (16, 16), torch.ones(16, 16, dtype=torch.float64))
    thr = [1.0 - (i + 1) / N for i in range(N)] if differential else None
    return IU.loop64(_model64(), _inputs(), TU.canvas_noise(hw), TABLES[sampler](N), IU.init_latent(hw), _mask(mask, hw), g=G, thr=thr,
                     tiles=tiles)


def _mask(name, hw=HW):
    return {"half": lambda: IU.half_mask(hw), "soft": lambda: IU.level_mask(hw, (0.0, 0.25, 1.0)),
            "map": lambda: IU.level_mask(hw, (0.0, 0.5, 1.0)), "ones": lambda: torch.ones((1,) + hw)}[name]()


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


def _kept(mask, like):
    return (mask == 0)[:, None].expand_as(like)


# ------------------------------------------------------------------------------------------------ 1: "off" is the plain loop, bit for bit
@pytest.mark.parametrize("mode", ["loop", "step"])
@pytest.mark.parametrize("sampler", ["euler", "dpmpp_sde"])
def test_off_is_the_plain_loop(gpu, sampler, mode):
    gm = _compiled()
    noise = TU.canvas_noise(HW)
    run = (lambda l: l.denoise(seed=77)) if sampler == "dpmpp_sde" else (lambda l: l.denoise(noise))
    with torch.no_grad():
        plain = _loop(gm, gpu, mode=mode, sampler=sampler)
        assert plain.inpaint_mask is None
        want = run(plain)
        loop = _loop(gm, gpu, mode=mode, sampler=sampler, inpaint=True)
        fresh = run(loop)                                        # no set_inpaint at all
        graph = loop.graph
        loop.set_inpaint(IU.init_latent(HW), IU.half_mask(HW))
        on = run(loop)
        loop.set_inpaint(None)
        off = run(loop)
    assert torch.isfinite(want).all() and torch.equal(fresh, want), "inpaint=True without set_inpaint must be the plain loop's bits"
    assert not torch.equal(on, want)
    assert torch.equal(off, want) and loop.graph is graph and graph is not None, "set_inpaint(None) must give the plain loop's bits again"


# ------------------------------------------------------------------------------------------------ 2: mask all zeros ends on init
@pytest.mark.parametrize("form", ["euler", "dpmpp", "euler_a", "dpmpp_sde", "pag"])
def test_mask_of_zeros_ends_on_init(gpu, form):
    init = IU.init_latent(HW)
    with torch.no_grad():
        if form == "pag":
            loop = _loop(_compiled(pag_layers=("mid",)), gpu, guidance_rescale=0.7, pag_scale=3.0, inpaint=True)
            assert loop.x_step.shape[0] == 3
        else:
            loop = _loop(_compiled(), gpu, sampler=form, guidance_rescale=0.7, inpaint=True)
        loop.set_inpaint(init, torch.zeros(HW))
        out = loop.denoise(TU.canvas_noise(HW), seed=5 if form in ("euler_a", "dpmpp_sde") else None).cpu()
    assert torch.equal(out, init), f"{form}: every pixel kept must end on the init latent, bit for bit"


# ------------------------------------------------------------------------------------------------ 3: binary mask against float64
@pytest.mark.parametrize("sampler", ["euler", "dpmpp"])
def test_binary_mask_matches_the_float64_loop(gpu, sampler):
    """Measured on an MI355X: the fp32 loop ends 4.19e-05 (Euler) and 4.09e-05 (DPM++ 2M) from loop64; gate 1e-3."""
    init, mask = IU.init_latent(HW), IU.half_mask(HW)
    with torch.no_grad():
        loop = _loop(_compiled(), gpu, sampler=sampler, inpaint=True)
        loop.set_inpaint(init, mask)
        out = loop.denoise(TU.canvas_noise(HW)).cpu()
    kept = _kept(mask, out)
    assert torch.equal(out[kept], init[kept]), "the kept half must equal the init latent bit for bit"
    ref = _ref(sampler)
    plain = _ref(sampler, "ones")
    err, moved = _err(out, ref), float((ref - plain)[~kept].abs().max())
    print(f"inpainting loop {sampler} fp32, half kept: max abs err vs the float64 loop {err:.2e} (|latent| max {float(ref.abs().max()):.1f}; the "
          f"kept half moves the repainted one by {moved:.2f})")
    assert moved > 100 * ABS_TOL_STRICT, "the kept half must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ 4: soft mask, differential mode
@pytest.mark.parametrize("kind", ["soft", "differential"])
def test_soft_and_differential_step_by_step(gpu, kind):
    init, noise = IU.init_latent(HW), TU.canvas_noise(HW)
    mask = _mask("soft" if kind == "soft" else "map")
    thr = I.differential_thresholds(N) if kind == "differential" else None
    with torch.no_grad():
        loop = _loop(_compiled(), gpu, mode="eager", inpaint=True)
        loop.set_inpaint(init, mask, differential=kind == "differential")
        loop.set_noise(noise)
        sig = [float(v) for v in loop.tables.sigmas]
        frozen_steps = 0
        for i in range(N):
            loop.run_steps(1)
            lat = loop.latent.cpu()
            w = IU.weight64(mask, None if thr is None else float(thr[i]))
            frozen = (w == 0).expand_as(lat)
            known = init.double() + sig[i + 1] * noise.double()
            assert bool(frozen.any()) and bool(torch.isfinite(lat).all())
            over = ((lat.double() - known).abs() - IU.ulp(known, torch.float32))[frozen]
            assert float(over.max()) <= 0.0, f"{kind} step {i}: a frozen pixel is not init + sigma[{i + 1}] noise to one fp32 ulp"
            frozen_steps += int(frozen[0, 0].sum())
        out = loop.latent.contiguous().cpu()
    kept = _kept(mask, out)
    assert torch.equal(out[kept], init[kept])
    if kind == "differential":                                 # bands 0, 0.5, 1 of 5, 5 and 6 columns: frozen for 10, 5 and 0 steps
        assert frozen_steps == 16 * (5 * 10 + 5 * 5)
    ref = _ref("euler", "soft") if kind == "soft" else _ref("euler", "map", differential=True)
    other = _ref("euler", "half")
    err = _err(out, ref)
    print(f"inpainting loop {kind} fp32: max abs err vs the float64 loop {err:.2e} (a binary mask ends {float((ref - other).abs().max()):.2f} away)")
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ 5: no recapture
def test_set_inpaint_needs_no_recapture(gpu):
    init, noise = IU.init_latent(HW), TU.canvas_noise(HW)
    with torch.no_grad():
        loop = _loop(_compiled(), gpu, inpaint=True)
        loop.capture()
        graph = loop.graph
        assert graph is not None
        plain = loop.denoise(noise).cpu()
        loop.set_inpaint(init, _mask("half"))
        half = loop.denoise(noise).cpu()
        assert loop.graph is graph and not torch.equal(half, plain)
        assert torch.equal(loop.denoise(noise).cpu(), half), "a second identical run must repeat its bits"
        loop.set_inpaint(init, _mask("map"), differential=True)  # both forms of w through the one captured launch
        diff = loop.denoise(noise).cpu()
        loop.set_inpaint(init, _mask("map"))
        soft = loop.denoise(noise).cpu()
        assert loop.graph is graph and not torch.equal(diff, soft) and not torch.equal(diff, half)
        fresh = _loop(_compiled(), gpu, inpaint=True)
        fresh.set_inpaint(init, _mask("half"))
        assert torch.equal(fresh.denoise(noise).cpu(), half), "the bits of a loop that had the mask before its capture"
    assert _err(half, _ref("euler")) <= ABS_TOL_STRICT
    assert _err(diff, _ref("euler", "map", differential=True)) <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ 6: tiled, the mask on the canvas
def test_tiled_canvas(gpu):
    hw = (16, 24)
    init, mask, noise = IU.init_latent(hw), IU.half_mask(hw), TU.canvas_noise(hw)
    with torch.no_grad():
        loop = _loop(_compiled(), gpu, hw, tile_hw=16, tile_stride=8, inpaint=True)
        grid = T.TileGrid(hw, 16, 8)
        assert (loop.tile_grid.xs, loop.tile_grid.T) == (grid.xs, 2) and tuple(loop.inpaint_mask.shape) == (1, 16, 24)
        loop.set_inpaint(init, mask)
        out = loop.denoise(noise).cpu()
    kept = _kept(mask, out)
    assert torch.equal(out[kept], init[kept]), "the kept region of the canvas must equal the init latent bit for bit"
    err = _err(out, _ref("euler", "half", tiled=True))
    print(f"tiled inpainting loop 16x24 fp32: max abs err vs the float64 tiled loop {err:.2e}")
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ 7: partial strength (img2img start)
def test_partial_strength_in_step_mode(gpu):
    init, mask, noise = IU.init_latent(HW), IU.half_mask(HW), TU.canvas_noise(HW)

    def run(loop):
        k = loop.set_image(init, noise, 0.5)
        assert k == 5
        loop.run_steps(k)
        return loop.latent.contiguous().cpu()

    with torch.no_grad():
        plain = run(_loop(_compiled(), gpu, mode="step"))
        loop = _loop(_compiled(), gpu, mode="step", inpaint=True)
        loop.set_inpaint(init, mask)
        out = run(loop)
        loop.set_inpaint(init, torch.ones(HW))
        ones = run(loop)
    kept = _kept(mask, out)
    assert torch.equal(out[kept], init[kept]) and not torch.equal(out, plain)
    assert torch.equal(ones, plain), "a mask of ones must give the bits of the same run without inpaint"
    ref = IU.loop64(_model64(), _inputs(), noise, TABLES["euler"](N), init, mask, g=G, start=5)
    assert _err(out, ref) <= ABS_TOL_STRICT
