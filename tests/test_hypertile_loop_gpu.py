"""HyperTile in the captured denoise loop and behind the Diffusers wrapper, on the TINY network at LATENT 64: its first attention level
(128 channels, 2 heads) has a 32 x 32 token grid, the second 16 x 16.  With tile = 16, swap = 1 the first level runs (2, 2) windows at
every step and the second keeps the whole grid.  The float64 reference is the tests' own: the eager CPU module whose first-level attn1
modules run on window-major copies of their input (projections are per token), in tests/reference_util.py's Euler loop, 6 steps."""
import functools
import types

import pytest
import torch

from stabletriton_amd import hooks, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import reference_util as RU

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
HW, STEPS = 64, 6
GRID, TILING = (32, 32), (2, 2)


def _model(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


@functools.lru_cache(maxsize=None)
def _inputs():
    return synth.denoise_inputs(2, HW, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _compiled(dtype, hypertile=True):
    return optimize_model(_model(dtype, torch.device("cuda:0")), cuda_graph=False, hypertile_layers=(".*",) if hypertile else None)


def _loop(gm, dtype, dev, mode="loop"):
    x = _inputs()
    loop = DenoiseLoop(gm, 1, HW, dtype, dev, euler_discrete_tables(STEPS), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode)
    loop.set_conditioning(*(x[k][1:2].to(dev, dtype) for k in ("encoder_hidden_states", "text_embeds", "time_ids")))
    return loop


def _model64(windowed):
    """The float64 eager module; `windowed`: its 1024-token self-attentions run per (2, 2) window."""
    m = _model(torch.float64, "cpu")
    if not windowed:
        return m
    gh, gw = GRID
    th, tw = gh // TILING[0], gw // TILING[1]

    def hook(mod, args, out):
        x = args[0]
        if x.shape[1] != gh * gw:
            return out
        b, _, c = x.shape
        xw = x.reshape(b, TILING[0], th, TILING[1], tw, c).permute(0, 1, 3, 2, 4, 5).reshape(b * TILING[0] * TILING[1], th * tw, c)
        ow = type(mod).forward(mod, xw)
        return ow.reshape(b, TILING[0], TILING[1], th, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(b, gh * gw, c)

    for name, mod in m.named_modules():
        if name.endswith("attn1"):
            mod.register_forward_hook(hook)
    return m


def test_tables_off_equal_the_plain_loop_and_are_written_without_recapture(gpu):
    dtype = torch.bfloat16
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        plain = _loop(_compiled(dtype, False), dtype, gpu).denoise(noise).cpu()
        gm = _compiled(dtype)
        assert gm.rewrite_stats["hypertile_sites"] == 17
        loop = _loop(gm, dtype, gpu)
        loop.set_hypertile(None)
        off = loop.denoise(noise).cpu()
        assert any(s.grid == GRID and s.rows for s in gm.hypertile._sites.values()), "the 32 x 32 level runs the window kernel"
        assert torch.isfinite(off).all() and torch.equal(off, plain), "every row (1, 1): the bits of a loop compiled without the pass"
        graph = loop.graph
        assert graph is not None
        loop.set_hypertile(tile=16, swap=2, seed=7)
        on = loop.denoise(noise).cpu()
        assert loop.graph is graph and torch.isfinite(on).all() and not torch.equal(on, off)
        assert torch.equal(loop.denoise(noise).cpu(), on), "a second run repeats its bits"
        before = _loop(gm, dtype, gpu)                        # the tables are the module's: this loop captures with them written
        assert torch.equal(before.denoise(noise).cpu(), on), "a loop that had the table before capture gives the same bits"
        loop.set_hypertile(None)
        assert torch.equal(loop.denoise(noise).cpu(), off) and loop.graph is graph


def test_fp32_fixed_tiling_matches_the_float64_windowed_loop(gpu):
    dtype = torch.float32
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(_compiled(dtype), dtype, gpu)
        loop.set_hypertile(tile=16, swap=1)
        out = loop.denoise(noise).cpu()
    ref, whole = (RU.loop64(_model64(w), _inputs(), euler_discrete_tables(STEPS), None, None) for w in (True, False))
    moved = float((ref - whole).abs().max())
    err = float((out.double() - ref).abs().max())
    print(f"tiny hypertile (2, 2) {STEPS}-step loop fp32: max abs err vs the float64 windowed loop {err:.2e}; the windows move the float64 result by {moved:.2e}")
    assert moved > 10 * ABS_TOL_STRICT, "the windows must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT



def test_diffusers_hook_tiles_in_place_and_counts_its_calls(gpu):
    x, t, dtype = _inputs(), torch.tensor(300.0), torch.bfloat16

    def call(u, dtype):
        ehs, cond = x["encoder_hidden_states"][:1].to(gpu, dtype), {k: x[k][:1].to(gpu, dtype) for k in ("text_embeds", "time_ids")}
        return u(x["latent"][:1].to(gpu, dtype), t, encoder_hidden_states=ehs, added_cond_kwargs=cond)[0].clone()

    make = lambda dtype, **kw: hooks.attach_to_diffusers(types.SimpleNamespace(unet=_model(dtype, gpu)), TINY, dtype, **kw).unet
    unet, plain = make(dtype, hypertile_layers=(".*",)), make(dtype)
    off = call(unet, dtype)
    assert torch.equal(off, call(plain, dtype)), "off: the bits of a wrapper compiled without the sites"
    cached = next(iter(unet._steps.values()))._cached
    graphs = dict(cached)
    unet.enable_hypertile(tile=16, swap=2, seed=7)
    on = [call(unet, dtype) for _ in range(3)]
    assert any(s.rows and s.host[0] != (1, 1) for s in unet.compiled.hypertile._sites.values()), "draw 0 tiles a site"
    assert dict(cached) == graphs and int(unet._hypertile_step) == 2 and torch.isfinite(on[0]).all() and not torch.equal(on[0], off)
    unet.enable_hypertile(tile=16, swap=2, seed=7)
    assert torch.equal(call(unet, dtype), on[0]), "the counter starts again: draw 0"
    unet.disable_hypertile()
    assert torch.equal(call(unet, dtype), off) and dict(cached) == graphs
    with pytest.raises(ValueError, match="hypertile_layers"):
        plain.enable_hypertile()
    strict = make(torch.float32, hypertile_layers=(".*",))      # strict mode: the slow path's HOST tiling, so its graphs are captured again
    whole = call(strict, torch.float32)
    with pytest.raises(ValueError, match="slow path"):
        strict.enable_hypertile(tile=16, swap=2)
    strict.enable_hypertile(tile=16, swap=1)
    assert not torch.equal(call(strict, torch.float32), whole)
