"""ControlNet in the captured denoise loop and behind the hooks, on the TINY network.

The reference is the tests' own: the EAGER UNet in float64 on the CPU, its `denoise` restated with the residuals added behind the
encoder and the middle block (tests/controlnet_util.py), the residuals computed per step by the eager float64 ControlNetXL on that
step's own input rows, inside the float64 guided loop of tests/pag_util.py.  Euler 10 steps, g = 5, fp32; rows [negative | positive]
from synth.denoise_inputs(2, 16, 1234): row 0 the negative prompt, row 1 the prompt, row 0's noise.  The gate is the T2I-Adapter loop
test's for the same comparison: the project's strict 1e-3."""
import functools

import pytest
import torch

from stabletriton_amd import controlnet as CN, hooks, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import controlnet_util as CU
from tests import pag_util as PU

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
def _branch64():
    return CU.branch(TINY).double()


@functools.lru_cache(maxsize=None)
def _inputs():
    return synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _image():
    return CU.control_image(1, 16)


@functools.lru_cache(maxsize=None)
def _compiled(sites=True, pag=False):
    return optimize_model(_model(DT, torch.device("cuda:0")), cuda_graph=False, controlnet=sites, pag_layers=("mid",) if pag else None)


@functools.lru_cache(maxsize=None)
def _compiled_branch():
    return optimize_model(CU.branch(TINY).to("cuda:0", DT), cuda_graph=False)


@functools.lru_cache(maxsize=None)
def _cond():
    """The control image's embedding, computed ONCE: `embed_condition` is eager torch (off the hot path), whose convolutions do not
    promise the same bits from one call to the next, so every loop of a bit-for-bit comparison is handed this one tensor."""
    return _compiled_branch().embed_condition(_image().to("cuda:0"))


class _Stepped:
    """The float64 eager pair: call i runs the branch on the call's own rows and the UNet with its residuals at the scale of step i
    (0: the plain UNet)."""

    def __init__(self, scales, weights=None):
        self.m, self.net, self.scales, self.weights, self.i = _model64(), _branch64(), list(scales), weights, 0
        self.cond = self.net.embed_condition(_image().double())

    def named_modules(self):
        return self.m.named_modules()

    def __call__(self, xin, t, ehs, cond):
        s = self.scales[self.i]
        self.i += 1
        if not s:
            return self.m(xin, t, ehs, cond)
        res = CU.branch_residuals(self.net, xin, t, ehs, cond, self.cond.repeat(xin.shape[0], 1, 1, 1))
        return CU.controlled(self.m, xin, t, ehs, cond, res, s, self.weights)


@functools.lru_cache(maxsize=None)
def _ref(scales, pag=None, sampler="euler", weights=None):
    """float64 controlled loop, computed once per configuration."""
    tables = euler_discrete_tables(N) if sampler == "euler" else dpmpp_2m_tables(N)
    return PU.loop64(_Stepped(scales, weights), _inputs(), tables, pag, g=G, pos=slice(1, 2), neg=slice(0, 1))[0]


def _loop(gm, dev, mode="loop", branch=True, tables=None, **kw):
    x = _inputs()
    loop = DenoiseLoop(gm, 1, 16, DT, dev, tables or euler_discrete_tables(N), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode,
                       guidance_scale=G, controlnet=_compiled_branch() if branch else None, **kw)
    rows = lambda k, r: x[k][r].to(dev, DT)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    loop.set_conditioning(*(rows(k, slice(1, 2)) for k in keys), *(rows(k, slice(0, 1)) for k in keys))
    return loop


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ modes
def test_modes_agree_and_match_the_float64_controlled_loop(gpu):
    gm = _compiled()
    noise = _inputs()["latent"][:1]
    finals = {}
    with torch.no_grad():
        for mode in ("eager", "step", "loop"):
            loop = _loop(gm, gpu, mode)
            loop.set_controlnet(_cond(), S)
            finals[mode] = loop.denoise(noise).cpu()
            assert torch.equal(finals[mode], loop.denoise(noise).cpu()), f"{mode}: a replay must repeat its bits"
            assert gm.controlnet._use is None, "the loop lends its table and residuals around its own calls only"
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    ref, plain = _ref((S,) * N), _ref((0.0,) * N)
    moved = float((ref - plain).abs().max())
    err = _err(finals["loop"], ref)
    print(f"tiny CFG + ControlNet 10-step loop fp32: max abs err vs the float64 controlled loop {err:.2e} ({err / ABS_TOL_STRICT:.3f} of the "
          f"gate); the residuals move the float64 result by {moved:.2f}")
    assert moved > 10 * ABS_TOL_STRICT, "the residuals must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


@pytest.mark.parametrize("mode,start,end", [("loop", 0.0, 0.5), ("step", 0.2, 0.75)])
def test_start_and_end_window_the_control(gpu, mode, start, end):
    gm = _compiled()
    noise = _inputs()["latent"][:1]
    lo, hi = int(N * start), int(N * end)
    scales = (0.0,) * lo + (S,) * (hi - lo) + (0.0,) * (N - hi)
    with torch.no_grad():
        loop = _loop(gm, gpu, mode)
        loop.set_controlnet(_image().to(gpu), S, start=start, end=end)
        assert loop.controlnet_table.tolist() == [pytest.approx(v) for v in scales]
        out = loop.denoise(noise).cpu()
    ref = _ref(scales)
    err = _err(out, ref)
    apart = float((ref - _ref((S,) * N)).abs().max())
    print(f"tiny ControlNet on steps [{lo}, {hi}) (mode {mode}): max abs err vs the float64 loop controlled on those steps {err:.2e}; "
          f"that loop is {apart:.2f} from the one controlled on all 10")
    assert apart > 10 * ABS_TOL_STRICT
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
        plain_bits = loop.denoise(noise).cpu()                     # nothing set: off (the branch runs on a zero embedding)
        loop.set_controlnet(_cond(), S, end=0.5)
        late = loop.denoise(noise).cpu()
        assert loop.graph is graph, "no new capture"
        fresh_loop = _loop(gm, gpu, "loop")
        fresh_loop.set_controlnet(_cond(), S, end=0.5)
        fresh = fresh_loop.denoise(noise).cpu()
        assert torch.equal(late, fresh), "set after capture() gives the bits of a loop set up that way from the start"
        assert not torch.equal(late, plain_bits)
        # the image itself instead of its embedding (embedded by the branch's eager `embed_condition`); per-site weights on top
        w = tuple(0.5 + 0.125 * k for k in range(10))
        loop.set_controlnet(_image().to(gpu), S)
        assert not torch.equal(loop.controlnet_cond, torch.zeros_like(loop.controlnet_cond))
        assert float((loop.controlnet_cond - _cond()).abs().max()) <= 1e-5 * float(_cond().abs().max())
        loop.set_controlnet_scale([S] * N, site_weights=w)
        assert loop.graph is graph and _err(loop.denoise(noise), _ref((S,) * N, weights=w)) <= ABS_TOL_STRICT
        loop.set_controlnet_scale(S, site_weights=[1.0] * 10)
        assert _err(loop.denoise(noise), _ref((S,) * N)) <= ABS_TOL_STRICT
        loop.set_controlnet(None)
        off = loop.denoise(noise).cpu()
        assert loop.graph is graph and torch.equal(off, plain_bits)
        without = _loop(_compiled(sites=False), gpu, "loop", branch=False).denoise(noise).cpu()
        assert torch.equal(off, without), "set_controlnet(None) gives the bits of a loop on a UNet compiled without sites"
    with pytest.raises(ValueError, match="takes a float or 10 values"):
        loop.set_controlnet_scale([1.0] * 3)
    with pytest.raises(ValueError, match="takes a control image"):
        loop.set_controlnet(torch.zeros(1, 3, 64, 64, device=gpu))
    with pytest.raises(ValueError, match="compiled without ControlNet sites"):
        _loop(_compiled(sites=False), gpu, "eager")
    with pytest.raises(ValueError, match="compiled without ControlNet sites"):
        _loop(_compiled(sites=False), gpu, "eager", branch=False).set_controlnet(None)
    with pytest.raises(ValueError, match="built without controlnet="):
        _loop(gm, gpu, "eager", branch=False).set_controlnet(_image().to(gpu))
    with pytest.raises(ValueError, match="tile_hw cannot be combined with a UNet compiled with controlnet"):
        DenoiseLoop(gm, 1, 24, DT, gpu, euler_discrete_tables(N), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, tile_hw=16)


# ------------------------------------------------------------------------------------------------ other samplers and guidance forms
def test_dpmpp_2m(gpu):
    gm = _compiled()
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, gpu, "loop", tables=dpmpp_2m_tables(N))
        loop.set_controlnet(_image().to(gpu), S)
        out = loop.denoise(noise).cpu()
    ref = _ref((S,) * N, sampler="dpmpp")
    err = _err(out, ref)
    print(f"tiny CFG + ControlNet DPM++ 2M loop fp32: max abs err vs the float64 controlled loop {err:.2e}")
    assert float((ref - _ref((0.0,) * N, sampler="dpmpp")).abs().max()) > 10 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT


def test_with_pag_rows(gpu):
    """CFG + PAG: rows [negative | positive | perturbed]; the branch runs on all three with ordinary attention, the UNet's perturbed
    rows carry their own residuals."""
    gm = _compiled(pag=True)
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        loop = _loop(gm, gpu, "loop", pag_scale=3.0)
        assert loop.x_in.shape[0] == 3 and loop.controlnet_cond.shape[0] == 3
        loop.set_controlnet(_image().to(gpu), S)
        out = loop.denoise(noise).cpu()
    ref = _ref((S,) * N, 3.0)
    err = _err(out, ref)
    print(f"tiny CFG + PAG + ControlNet loop fp32: max abs err vs the float64 controlled loop {err:.2e}")
    assert float((ref - _ref((0.0,) * N, 3.0)).abs().max()) > 10 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT


# ------------------------------------------------------------------------------------------------ hooks
def _call_args(dev, dtype):
    x = _inputs()
    return (x["latent"].to(dev, dtype), torch.tensor(500.0, device=dev)), dict(
        encoder_hidden_states=x["encoder_hidden_states"].to(dev, dtype),
        added_cond_kwargs={"text_embeds": x["text_embeds"].to(dev, dtype), "time_ids": x["time_ids"].to(dev, dtype)})


@functools.lru_cache(maxsize=None)
def _step_residuals():
    """What a ControlNet pipeline hands the UNet at one step: the float64 branch's outputs on the call's own rows, scaled by S and
    rounded to the compute type."""
    x = {k: v.double() for k, v in _inputs().items()}
    net = _branch64()
    cond = net.embed_condition(_image().double()).repeat(2, 1, 1, 1)
    res = CU.branch_residuals(net, x["latent"], torch.tensor(500.0), x["encoder_hidden_states"],
                              {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]}, cond)
    return tuple((S * r).to(DT) for r in res)


def _eager64_step(on):
    x = {k: v.double() for k, v in _inputs().items()}
    res = [r.double() for r in _step_residuals()] if on else None
    with torch.no_grad():
        return CU.controlled(_model64(), x["latent"], torch.tensor(500.0), x["encoder_hidden_states"],
                             {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]}, res, 1.0)[0]


def test_diffusers_hook_honours_the_controlnet_residuals(gpu):
    m = _model(DT, gpu)
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DT, gpu, cuda_graph=True, controlnet=True)
    args, kw = _call_args(gpu, DT)
    res = [r.to(gpu) for r in _step_residuals()]
    with torch.no_grad():
        on = unet(*args, **kw, down_block_additional_residuals=[r.clone() for r in res[:9]], mid_block_additional_residual=res[9].clone())[0]
        off = unet(*args, **kw, down_block_additional_residuals=None, mid_block_additional_residual=None)[0]
        on2 = unet(*args, **kw, down_block_additional_residuals=res[:9], mid_block_additional_residual=res[9])[0]
        off2 = unet(*args, **kw)[0]
    assert len(unet._steps) == 1
    step_fn = next(iter(unet._steps.values()))
    assert len(step_fn._cached) == 1, "ONE captured graph: residuals on, off and on again are in-place writes, never a new capture"
    assert torch.equal(off, off2) and torch.equal(on, on2) and not torch.equal(on, off)
    ref_on, ref_off = _eager64_step(True), _eager64_step(False)
    assert float((ref_on - ref_off).abs().max()) > 10 * ABS_TOL_STRICT
    assert _err(on, ref_on) <= ABS_TOL_STRICT and _err(off, ref_off) <= ABS_TOL_STRICT
    with pytest.raises(NotImplementedError, match="down_intrablock_additional_residuals"):
        unet(*args, **kw, down_intrablock_additional_residuals=res[:4])
    plain = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DT, gpu, cuda_graph=True)
    with torch.no_grad():
        a = plain(*args, **kw)[0]
        b = plain(*args, **kw, down_block_additional_residuals=res[:9], mid_block_additional_residual=res[9])[0]
    assert torch.equal(a, b) and torch.equal(a, off), "scale 0 is the wrapper without sites, bit for bit"


def test_comfy_hook_matches_the_diffusers_hook(gpu):
    m = _model(DT, gpu)
    adapter = hooks.compile_comfy_unet(m, cuda_graph=True, controlnet=True)
    x = _inputs()
    lat, ehs = x["latent"].to(gpu, DT), x["encoder_hidden_states"].to(gpu, DT)
    with torch.no_grad():
        tid = m.add_time_proj(x["time_ids"].to(gpu, DT).flatten()).reshape(2, -1)
        y = torch.cat([x["text_embeds"].to(gpu, DT), tid.to(DT)], dim=-1)
    t = torch.full((2,), 500.0, device=gpu)
    res = [r.to(gpu) for r in _step_residuals()]
    control = {"input": [], "middle": [res[9]], "output": list(res[:9])}
    with torch.no_grad():
        on = adapter(lat, t, ehs, y, control=control)
        off = adapter(lat, t, ehs, y, control=None)
        again = adapter(lat, t, ehs, y, control=control)
    step_fn = next(iter(adapter._steps.values()))
    assert len(adapter._steps) == 1 and len(step_fn._cached) == 1, "one captured graph for control on, off and on again"
    assert torch.equal(on, again)
    assert _err(on, _eager64_step(True)) <= ABS_TOL_STRICT and _err(off, _eager64_step(False)) <= ABS_TOL_STRICT
    unet = hooks.compile_unet_from_state_dict(m.state_dict(), TINY, DT, gpu, cuda_graph=False, controlnet=True)
    args, kw = _call_args(gpu, DT)
    with torch.no_grad():
        same = unet(*args, **kw, down_block_additional_residuals=res[:9], mid_block_additional_residual=res[9])[0]
    # (not bit for bit: this test builds y's Fourier features in torch, the Diffusers entry's graph with the timestep kernel)
    diff = float((on - same).abs().max())
    print(f"ComfyUI entry vs Diffusers entry with the same residuals: max abs diff {diff:.2e}")
    assert diff <= ABS_TOL_STRICT and float((on - off).abs().max()) > 10 * ABS_TOL_STRICT
    with pytest.raises(NotImplementedError, match="T2I-Adapter residuals"):
        adapter(lat, t, ehs, y, control={"input": [res[0]], "middle": [], "output": []})
