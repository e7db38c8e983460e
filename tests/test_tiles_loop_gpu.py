"""Tiled denoising (MultiDiffusion) in the captured denoise loop, on the TINY network in fp32: Euler 10 steps, g = 5, windows 16 x 16,
canvas noise from torch.Generator().manual_seed(99), prompts from synth.denoise_inputs(2, 16, 1234) (row 0 the negative prompt, row 1
the prompt).

Where a tiled loop has an untiled equal (one window; disjoint windows) the comparison is bit for bit.  Overlapping windows are compared
with the tests' own float64 tiled loop around the eager CPU module (tests/tiles_util.py) under the project's gate for this network and
schedule, ABS_TOL_STRICT; the same test shows in float64 that a wrong blend ("the last window wins") ends far outside that gate."""
import functools

import pytest
import torch

from stabletriton_amd import synth, tiles as T
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import tiles_util as TU

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
G = 5.0
WIN = 16
KEYS = ("encoder_hidden_states", "text_embeds", "time_ids")
# canvas, stride, wrap: the four canvases the feature was sized on
OVERLAP = {"16x24": ((16, 24), 8, False), "24x24": ((24, 24), 8, False), "16x24_wrap": ((16, 24), 8, True), "20x28": ((20, 28), (4, 6), False)}


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
def _inputs(rows=2):
    return synth.denoise_inputs(rows, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _compiled(**kw):
    return optimize_model(_model(torch.float32, torch.device("cuda:0")), cuda_graph=False, **kw)


def _euler():
    return euler_discrete_tables(10)


def _loop(gm, dev, hw, mode="loop", tables=None, batch=1, x=None, pos=slice(1, 2), neg=slice(0, 1), **kw):
    x = x or _inputs()
    kw.setdefault("guidance_scale", G)
    loop = DenoiseLoop(gm, batch, hw, torch.float32, dev, tables or _euler(), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode, **kw)
    rows = lambda k, r: x[k][r].to(dev)
    loop.set_conditioning(*(rows(k, pos) for k in KEYS), *(rows(k, neg) for k in KEYS))
    return loop


def _grid(case):
    hw, stride, wrap = OVERLAP[case]
    return T.TileGrid(hw, WIN, stride, wrap_w=wrap)


@functools.lru_cache(maxsize=None)
def _ref(case, weights="uniform", mode="mean", **kw):
    """The float64 tiled loop, once per configuration."""
    g = _grid(case)
    wt = TU.gaussian64(WIN, WIN) if weights == "gaussian" else torch.ones(WIN, WIN, dtype=torch.float64)
    return TU.loop64(_model64(), _inputs(), TU.canvas_noise(g.canvas_hw), _euler(), TU.starts(g.canvas_hw[0], WIN, g.stride[0]),
                     TU.starts(g.canvas_hw[1], WIN, g.stride[1], g.wrap_w), (WIN, WIN), wt, g=G, mode=mode, **kw)


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


def _tile_kw(case, **kw):
    hw, stride, wrap = OVERLAP[case]
    return dict(tile_hw=WIN, tile_stride=stride, tile_wrap_w=wrap, **kw)


# ------------------------------------------------------------------------------------------------ 1, 2: untiled equals, bit for bit
@pytest.mark.parametrize("sampler", ["euler", "dpmpp_sde"])
def test_one_window_is_the_untiled_loop(gpu, sampler):
    gm = _compiled()
    tables = (lambda: dpmpp_2m_sde_tables(10)) if sampler == "dpmpp_sde" else _euler
    noise = TU.canvas_noise((16, 16))
    with torch.no_grad():
        tiled, plain = _loop(gm, gpu, 16, tables=tables(), tile_hw=16), _loop(gm, gpu, 16, tables=tables())
        assert tiled.tile_grid.T == 1 and tiled.x_step is not tiled.x_in and plain.x_step is plain.x_in
        if sampler == "dpmpp_sde":
            a, b = tiled.denoise(seed=77), plain.denoise(seed=77)
        else:
            a, b = tiled.denoise(noise), plain.denoise(noise)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("sampler", ["euler", "dpmpp"])
def test_disjoint_windows_are_an_untiled_batch(gpu, sampler):
    """Canvas 16 x 32, stride 16: two windows that share no pixel, B = 1, against an untiled B = 2 loop on the two halves of the noise
    with the same prompts - the UNet rows [n0 n1 | p0 p1] are the same in both."""
    gm = _compiled()
    tables = (lambda: dpmpp_2m_tables(10)) if sampler == "dpmpp" else _euler
    noise = TU.canvas_noise((16, 32))
    halves = torch.cat([noise[:, :, :, :16], noise[:, :, :, 16:]])
    with torch.no_grad():
        tiled = _loop(gm, gpu, (16, 32), tables=tables(), tile_hw=16, tile_stride=16)
        assert (tiled.tile_grid.xs, tiled.x_in.shape[0]) == ([0, 16], 4)
        x = {k: v[[0, 0, 1, 1]] for k, v in _inputs().items()}
        plain = _loop(gm, gpu, 16, tables=tables(), batch=2, x=x, pos=slice(2, 4), neg=slice(0, 2))
        a, b = tiled.denoise(noise), plain.denoise(halves)
    assert torch.equal(a[:, :, :, :16], b[0:1]) and torch.equal(a[:, :, :, 16:], b[1:2])


# ------------------------------------------------------------------------------------------------ 3: overlap against float64
@pytest.mark.parametrize("case,weights", [("16x24", "uniform"), ("24x24", "uniform"), ("16x24_wrap", "uniform"), ("20x28", "uniform"),
                                          ("24x24", "gaussian")])
def test_overlapping_windows_match_the_float64_tiled_loop(gpu, case, weights):
    gm = _compiled()
    grid = _grid(case)
    noise = TU.canvas_noise(grid.canvas_hw)
    with torch.no_grad():
        loop = _loop(gm, gpu, grid.canvas_hw, **_tile_kw(case, tile_weights=weights))
        assert (loop.tile_grid.ys, loop.tile_grid.xs) == (grid.ys, grid.xs) and loop.x_in.shape[0] == 2 * grid.T
        out = loop.denoise(noise).cpu()
    ref = _ref(case, weights)
    wrong = _ref(case, weights, mode="last")
    apart = float((wrong - ref).abs().max())
    err = _err(out, ref)
    print(f"tiled loop {case} {weights} fp32: max abs err vs the float64 tiled loop {err:.2e} (|latent| max {float(ref.abs().max()):.1f}; "
          f"'last window wins' ends {apart:.1f} away in float64)")
    assert apart > 1.0, "a wrong blend must end far outside the gate for this check to mean anything"
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ 4, 5: modes, weights in place
def test_modes_agree_and_a_replay_repeats(gpu):
    gm = _compiled()
    noise = TU.canvas_noise((24, 24))
    finals = {}
    with torch.no_grad():
        for mode in ("eager", "step", "loop"):
            loop = _loop(gm, gpu, 24, mode, **_tile_kw("24x24"))
            finals[mode] = loop.denoise(noise).cpu()
            assert torch.equal(finals[mode], loop.denoise(noise).cpu()), f"{mode}: a replay must repeat its bits"
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    assert _err(finals["loop"], _ref("24x24")) <= ABS_TOL_STRICT


def test_set_tile_weights_needs_no_recapture(gpu):
    gm = _compiled()
    noise = TU.canvas_noise((24, 24))
    with torch.no_grad():
        loop = _loop(gm, gpu, 24, **_tile_kw("24x24"))
        uniform = loop.denoise(noise).cpu()
        graph = loop.graph
        assert graph is not None
        loop.set_tile_weights("gaussian")
        gauss = loop.denoise(noise).cpu()
        assert loop.graph is graph and not torch.equal(gauss, uniform)
        fresh = _loop(gm, gpu, 24, **_tile_kw("24x24", tile_weights="gaussian")).denoise(noise).cpu()
        assert torch.equal(gauss, fresh), "the bits of a loop built with those weights"
        loop.set_tile_weights("uniform")
        assert torch.equal(loop.denoise(noise).cpu(), uniform) and loop.graph is graph
        with pytest.raises(ValueError, match="positive"):
            loop.set_tile_weights(torch.zeros(16, 16))
    assert _err(gauss, _ref("24x24", "gaussian")) <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ 6, 7, 8: conditioning and guidance forms
def test_one_prompt_per_window(gpu):
    gm = _compiled()
    case = "16x24_wrap"                                        # T = 3: windows 0, 1, 2 take prompts 1, 2, 3; one negative (row 0)
    x = _inputs(4)
    noise = TU.canvas_noise((16, 24))
    with torch.no_grad():
        loop = _loop(gm, gpu, (16, 24), x=x, pos=slice(1, 4), neg=slice(0, 1), **_tile_kw(case))
        out = loop.denoise(noise).cpu()
        same = _loop(gm, gpu, (16, 24), x=x, **_tile_kw(case)).denoise(noise).cpu()
    g = _grid(case)
    ref = TU.loop64(_model64(), x, noise, _euler(), g.ys, g.xs, (WIN, WIN), torch.ones(WIN, WIN, dtype=torch.float64), g=G,
                    pos=slice(1, 4), neg=slice(0, 1))
    err = _err(out, ref)
    print(f"tiled loop, one prompt per window fp32: max abs err vs the float64 tiled loop {err:.2e}")
    assert float((out - same).abs().max()) > 100 * ABS_TOL_STRICT, "the windows' own prompts must matter"
    assert err <= ABS_TOL_STRICT


def test_guidance_rescale_over_the_canvas(gpu):
    gm = _compiled()
    noise = TU.canvas_noise((16, 24))
    with torch.no_grad():
        out = _loop(gm, gpu, (16, 24), guidance_rescale=0.7, **_tile_kw("16x24")).denoise(noise).cpu()
    ref = _ref("16x24", phi=0.7)
    err = _err(out, ref)
    moved = float((ref - _ref("16x24")).abs().max())
    print(f"tiled loop with guidance rescale 0.7 fp32: max abs err vs the float64 tiled loop {err:.2e} (the rescale moves it by {moved:.2f})")
    assert moved > 100 * ABS_TOL_STRICT and err <= ABS_TOL_STRICT


@pytest.mark.parametrize("form", ["pag", "seg"])
def test_perturbed_guidance_on_windows(gpu, form):
    noise = TU.canvas_noise((16, 24))
    if form == "pag":
        gm, kw, ref_kw = _compiled(pag_layers=("mid",)), dict(pag_scale=3.0), dict(s=3.0)
    else:
        gm, kw, ref_kw = _compiled(seg_layers=("mid",)), dict(seg_scale=3.0, seg_sigma=1.0), dict(s=3.0, seg_sigma=1.0)
    with torch.no_grad():
        loop = _loop(gm, gpu, (16, 24), **kw, **_tile_kw("16x24"))
        assert loop.x_in.shape[0] == 3 * 2 and tuple(loop.x_step.shape) == (3, 4, 16, 24)
        out = loop.denoise(noise).cpu()
        assert torch.equal(out, loop.denoise(noise).cpu())
    ref = _ref("16x24", **ref_kw)
    err = _err(out, ref)
    moved = float((ref - _ref("16x24")).abs().max())
    print(f"tiled loop with {form} fp32: max abs err vs the float64 tiled loop {err:.2e} (the perturbed block moves it by {moved:.2f})")
    assert moved > 100 * ABS_TOL_STRICT and err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals(gpu):
    for flag, tokens in ((dict(regions=2), 154), (dict(ip_adapter=1), 77), (dict(t2i_adapter=True), 77)):
        gm = optimize_model(_model(torch.float32, gpu), cuda_graph=False, **flag)
        with pytest.raises(ValueError, match=f"tile_hw cannot be combined with a UNet compiled with {next(iter(flag))}"):
            DenoiseLoop(gm, 1, (16, 24), torch.float32, gpu, _euler(), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, tokens=tokens,
                        guidance_scale=G, tile_hw=16)
    gm = _compiled()
    with pytest.raises(ValueError, match="multiples of 4"):
        _loop(gm, gpu, (16, 24), tile_hw=10)
    with pytest.raises(ValueError, match="larger than the canvas"):
        _loop(gm, gpu, (16, 24), tile_hw=(32, 16))
    with pytest.raises(ValueError, match="B = 1 rows"):
        _loop(gm, gpu, (16, 24), x=_inputs(4), pos=slice(0, 4), **_tile_kw("16x24"))
