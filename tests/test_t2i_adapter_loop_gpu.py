"""T2I-Adapter in the captured denoise loop and behind the hooks, on the TINY network.

The reference is the tests' own: the EAGER module in float64 on the CPU with forward hooks at the four places (tests/t2i_util.py),
hooked per step with that step's scale, inside the float64 guided loop of tests/pag_util.py.  Euler 10 steps, g = 5, fp32; rows
[negative | positive] from synth.denoise_inputs(2, 16, 1234): row 0 the negative prompt, row 1 the prompt, row 0's noise."""
import functools

import pytest
import torch

from stabletriton_amd import hooks, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import pag_util as PU
from tests import t2i_util as TU

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
G, S, N = 5.0, 0.7, 10
DT = torch.float32


def _model(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


@functools.lru_cache(maxsize=None)
def _model64():
    """The same weights (synth.fill_module_ is a function of the names and the seed) in float64 on the CPU."""
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double()


@functools.lru_cache(maxsize=None)
def _inputs(batch=1):
    """2 * batch rows: the first `batch` the negative prompts (and the noise), the others the prompts."""
    return synth.denoise_inputs(2 * batch, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _feats(batch=1):
    """One feature row per sample; the rows of a batch differ."""
    return tuple(TU.features(TINY, 16, rows=batch))


@functools.lru_cache(maxsize=None)
def _compiled(sites=True, pag=False):
    return optimize_model(_model(DT, torch.device("cuda:0")), cuda_graph=False, t2i_adapter=sites, pag_layers=("mid",) if pag else None)


class _Stepped:
    """The float64 eager module, hooked at call i with the scale of step i (None / 0: not hooked)."""

    def __init__(self, scales, batch=1):
        self.m, self.scales, self.i, self.batch = _model64(), list(scales), 0, batch

    def named_modules(self):
        return self.m.named_modules()

    def __call__(self, *args):
        s = self.scales[self.i]
        self.i += 1
        with TU.hooked(self.m, [f.double() for f in _feats(self.batch)], s if s else None):
            return self.m(*args)


@functools.lru_cache(maxsize=None)
def _ref(scales, pag=None, batch=1):
    """float64 hooked loop, computed once per configuration (the hooks repeat the `batch` feature rows over the row blocks)."""
    return PU.loop64(_Stepped(scales, batch), _inputs(batch), euler_discrete_tables(N), pag, g=G, pos=slice(batch, 2 * batch),
                     neg=slice(0, batch))[0]


def _loop(gm, dev, mode="loop", batch=1, **kw):
    x = _inputs(batch)
    loop = DenoiseLoop(gm, batch, 16, DT, dev, euler_discrete_tables(N), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode,
                       guidance_scale=G, **kw)
    rows = lambda k, r: x[k][r].to(dev, DT)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    loop.set_conditioning(*(rows(k, slice(batch, 2 * batch)) for k in keys), *(rows(k, slice(0, batch)) for k in keys))
    return loop


def _gf(dev, batch=1):
    return [f.to(dev) for f in _feats(batch)]


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ modes
def test_modes_agree_and_match_the_float64_hooked_loop(gpu):
    gm = _compiled()
    noise = _inputs()["latent"][:1]
    finals = {}
    with torch.no_grad():
        for mode in ("eager", "step", "loop"):
            loop = _loop(gm, gpu, mode)
            loop.set_t2i_adapter(_gf(gpu), S)
            finals[mode] = loop.denoise(noise).cpu()
            assert torch.equal(finals[mode], loop.denoise(noise).cpu()), f"{mode}: a replay must repeat its bits"
            assert gm.t2i_adapter._use is None, "the loop hands its table to the sites around its own calls only"
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    ref, plain = _ref((S,) * N), _ref((0.0,) * N)
    moved = float((ref - plain).abs().max())
    err = _err(finals["loop"], ref)
    print(f"tiny CFG + T2I sites 10-step loop fp32: max abs err vs the float64 hooked loop {err:.2e}; the residuals move the float64 "
          f"result by {moved:.2f}")
    assert moved > 100 * ABS_TOL_STRICT, "the residuals must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


@pytest.mark.parametrize("mode", ["loop", "step"])
def test_factor_switches_the_sites_off_after_its_share_of_the_steps(gpu, mode):
    gm = _compiled()
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, gpu, mode)
        loop.set_t2i_adapter(_gf(gpu), S, factor=0.5)
        assert loop.t2i_table.tolist() == [pytest.approx(S)] * 5 + [0.0] * 5
        out = loop.denoise(noise).cpu()
    ref = _ref((S,) * 5 + (0.0,) * 5)
    err = _err(out, ref)
    print(f"tiny T2I factor 0.5 (mode {mode}): max abs err vs the float64 loop hooked on its first 5 steps {err:.2e}; that loop is "
          f"{float((ref - _ref((S,) * N)).abs().max()):.2f} from the one hooked on all 10")
    assert float((ref - _ref((S,) * N)).abs().max()) > 100 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ no recapture
def test_set_after_capture_keeps_the_graph_and_none_is_the_plain_unet(gpu):
    gm = _compiled()
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, gpu, "loop")
        loop.capture()
        graph = loop.graph
        assert graph is not None
        plain_bits = loop.denoise(noise).cpu()                     # nothing set: off
        loop.set_t2i_adapter(_gf(gpu), S, factor=0.5)
        late = loop.denoise(noise).cpu()
        assert loop.graph is graph, "no new capture"
        fresh_loop = _loop(gm, gpu, "loop")
        fresh_loop.set_t2i_adapter(_gf(gpu), S, factor=0.5)
        fresh = fresh_loop.denoise(noise).cpu()
        assert torch.equal(late, fresh), "set after capture() gives the bits of a loop set up that way from the start"
        assert not torch.equal(late, plain_bits)
        loop.set_t2i_adapter_scale([S] * N)
        assert loop.graph is graph and _err(loop.denoise(noise), _ref((S,) * N)) <= ABS_TOL_STRICT
        loop.set_t2i_adapter(None)
        off = loop.denoise(noise).cpu()
        assert loop.graph is graph and torch.equal(off, plain_bits)
        without = _loop(_compiled(sites=False), gpu, "loop").denoise(noise).cpu()
        assert torch.equal(off, without), "set_t2i_adapter(None) gives the bits of a loop on a UNet compiled without sites"
    with pytest.raises(ValueError, match="takes a float or 10 values"):
        loop.set_t2i_adapter_scale([1.0] * 3)
    with pytest.raises(ValueError, match="takes 4 feature maps"):
        loop.set_t2i_adapter(_gf(gpu)[:2])
    with pytest.raises(ValueError, match="compiled without T2I-Adapter sites"):
        _loop(_compiled(sites=False), gpu, "eager").set_t2i_adapter(_gf(gpu))


def test_three_row_blocks_share_one_feature_copy(gpu):
    """CFG + PAG at B = 2: rows [n0 n1 | p0 p1 | x0 x1] = 3 B on a buffer of B DIFFERENT feature rows; row n reads feature row
    n % B.  (A mapping such as n // blocks would hand sample 1's negative row the features of sample 0: the reference with the
    two feature rows swapped is far from the result, which is what makes the check below mean something.)"""
    B = 2
    gm = _compiled(pag=True)
    noise = _inputs(B)["latent"][:B]
    feats = _gf(gpu, B)
    assert all(not torch.equal(f[0], f[1]) for f in feats)
    with torch.no_grad():
        loop = _loop(gm, gpu, "loop", batch=B, pag_scale=3.0)
        assert loop.x_in.shape[0] == 3 * B
        assert all(gm.t2i_adapter.features_for(3 * B, k, h, w).shape[0] == B for k, (_, h, w) in enumerate(TU.site_shapes(TINY, 16)))
        loop.set_t2i_adapter(feats, S)
        out = loop.denoise(noise).cpu()
        loop.set_t2i_adapter([f.flip(0) for f in feats], S)
        swapped = loop.denoise(noise).cpu()
    ref = _ref((S,) * N, 3.0, B)
    err = _err(out, ref)
    apart = _err(swapped, ref)
    print(f"tiny CFG + PAG + T2I sites loop fp32, B = 2: max abs err vs the float64 hooked loop {err:.2e}; with the two feature rows "
          f"swapped the loop ends {apart:.2f} away")
    assert apart > 100 * ABS_TOL_STRICT, "the two feature rows must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ hooks
def _call_args(dev, dtype):
    x = _inputs()
    return (x["latent"].to(dev, dtype), torch.tensor(500.0, device=dev)), dict(
        encoder_hidden_states=x["encoder_hidden_states"].to(dev, dtype),
        added_cond_kwargs={"text_embeds": x["text_embeds"].to(dev, dtype), "time_ids": x["time_ids"].to(dev, dtype)})


def _eager64_step(scale):
    x = {k: v.double() for k, v in _inputs().items()}
    m64 = _model64()
    feats = [f.double().repeat(2, 1, 1, 1) for f in _feats()]
    with torch.no_grad(), TU.hooked(m64, feats, scale):
        return m64(x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


def test_diffusers_hook_honours_intrablock_residuals(gpu):
    m = _model(DT, gpu)
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DT, gpu, cuda_graph=True, t2i_adapter=True)
    args, kw = _call_args(gpu, DT)
    residuals = [(S * f).to(gpu).repeat(2, 1, 1, 1) for f in _feats()]          # scaled by the pipeline, the same for both halves
    with torch.no_grad():
        on = unet(*args, **kw, down_intrablock_additional_residuals=[r.clone() for r in residuals])[0]
        off = unet(*args, **kw, down_intrablock_additional_residuals=None)[0]
        on2 = unet(*args, **kw, down_intrablock_additional_residuals=residuals)[0]
        off2 = unet(*args, **kw)[0]
    assert len(unet._steps) == 1
    step_fn = next(iter(unet._steps.values()))
    assert len(step_fn._cached) == 1, "ONE captured graph: residuals on, off and on again are in-place writes, never a new capture"
    assert torch.equal(off, off2)
    assert _err(on, _eager64_step(S)) <= ABS_TOL_STRICT and _err(off, _eager64_step(None)) <= ABS_TOL_STRICT
    assert torch.equal(on, on2) and not torch.equal(on, off)
    for name in ("down_block_additional_residuals", "mid_block_additional_residual"):
        with pytest.raises(NotImplementedError, match="ControlNet"):
            unet(*args, **kw, **{name: residuals[0]})
    with pytest.raises(ValueError, match="4 tensors expected"):
        unet(*args, **kw, down_intrablock_additional_residuals=residuals[:3])
    # a wrapper compiled without the flag ignores all three, exactly as before
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DT, gpu, cuda_graph=True)
    with torch.no_grad():
        a = plain(*args, **kw)[0]
        b = plain(*args, **kw, down_intrablock_additional_residuals=residuals, mid_block_additional_residual=residuals[3])[0]
    assert torch.equal(a, b) and torch.equal(a, off), "scale 0 is the wrapper without sites, bit for bit"


def test_comfy_hook_takes_control_input_and_middle(gpu):
    m = _model(DT, gpu)
    adapter = hooks.compile_comfy_unet(m, cuda_graph=True, t2i_adapter=True)
    st = adapter.compiled.t2i_adapter
    assert st.input_blocks == (3, 5, 8, None)
    x = _inputs()
    lat, ehs = x["latent"].to(gpu, DT), x["encoder_hidden_states"].to(gpu, DT)
    with torch.no_grad():
        tid = m.add_time_proj(x["time_ids"].to(gpu, DT).flatten()).reshape(2, -1)
        y = torch.cat([x["text_embeds"].to(gpu, DT), tid.to(DT)], dim=-1)
    t = torch.full((2,), 500.0, device=gpu)
    residuals = [(S * f).to(gpu).repeat(2, 1, 1, 1) for f in _feats()]
    inputs = [None] * 9
    inputs[-1 - 3], inputs[-1 - 5], inputs[-1 - 8] = residuals[:3]
    control = {"input": inputs, "middle": [residuals[3]], "output": []}
    with torch.no_grad():
        on = adapter(lat, t, ehs, y, control=control)
        off = adapter(lat, t, ehs, y, control=None)
        again = adapter(lat, t, ehs, y, control=control)
    step_fn = next(iter(adapter._steps.values()))
    assert len(adapter._steps) == 1 and len(step_fn._cached) == 1, "one captured graph for control on, off and on again"
    assert torch.equal(on, again)
    assert _err(on, _eager64_step(S)) <= ABS_TOL_STRICT and _err(off, _eager64_step(None)) <= ABS_TOL_STRICT
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DT, gpu, cuda_graph=False, t2i_adapter=True)
    args, kw = _call_args(gpu, DT)
    with torch.no_grad():
        same = unet(*args, **kw, down_intrablock_additional_residuals=residuals)[0]
    # (not bit for bit: this test builds y's Fourier features in torch, the Diffusers entry's graph with the timestep kernel)
    diff = float((on - same).abs().max())
    print(f"ComfyUI entry vs Diffusers entry with the same residuals: max abs diff {diff:.2e}")
    assert diff <= ABS_TOL_STRICT and float((on - off).abs().max()) > 100 * ABS_TOL_STRICT
    with pytest.raises(NotImplementedError, match="output"):
        adapter(lat, t, ehs, y, control={"input": inputs, "middle": [], "output": [residuals[0]]})
    wrong = [None] * 9
    wrong[-1 - 4] = residuals[1]
    with pytest.raises(NotImplementedError, match="input block 4"):
        adapter(lat, t, ehs, y, control={"input": wrong})
    # a wrapper compiled without the flag raises on any control, exactly as before
    plain = hooks.compile_comfy_unet(m, cuda_graph=False)
    with pytest.raises(NotImplementedError, match="ControlNet residuals"):
        plain(lat, t, ehs, y, control=control)
