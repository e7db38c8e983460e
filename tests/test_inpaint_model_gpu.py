"""A nine-channel inpainting UNet (TINY with in_channels = 9), fp32, compiled and in the captured loop: conv_in runs on st_conv_stem,
a 9-channel sample through the hooks' path, the loop's 4-channel x_in plus the condition buffer through the loop's.  References: the
eager float64 CPU module, and tests/inpaint_util.loop64 around it fed cat([x * in_scale, mask, masked latent]) (its own blend off: a
mask of ones).  Gate: ABS_TOL_STRICT of tests/test_inpaint_loop_gpu.py, the project's gate for this network and schedule."""
import dataclasses
import functools

import pytest
import torch

from stabletriton_amd import synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import inpaint_util as IU
from tests import tiles_util as TU
from tests.test_inpaint_loop_gpu import ABS_TOL_STRICT, G, HW, KEYS, N

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(dev):
    m = UNet2DConditionModel(dataclasses.replace(TINY, in_channels=9)).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double() if dev == "cpu" else optimize_model(m.to(dev), cuda_graph=False)


@functools.lru_cache(maxsize=None)
def _inputs():
    return synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


def _condition(other=False):
    """(mask, masked-image latent): the right half repainted and blanked in the image; `other`: the left half."""
    mask = 1.0 - IU.half_mask(HW) if other else IU.half_mask(HW)
    return mask, IU.init_latent(HW) * (1.0 - mask)[:, None]


@functools.lru_cache(maxsize=None)
def _ref(other=False):
    mask, masked = _condition(other)
    cond = torch.cat([mask[:, None], masked], dim=1).double()
    unet64 = lambda x, *args: _model("cpu")(torch.cat([x, cond.expand(x.shape[0], -1, -1, -1)], dim=1), *args)
    return IU.loop64(unet64, _inputs(), TU.canvas_noise(HW), euler_discrete_tables(N), torch.zeros((1, 4) + HW), torch.ones((1,) + HW), g=G)


def _loop(dev, **kw):
    x = _inputs()
    loop = DenoiseLoop(_model("cuda:0"), 1, HW, torch.float32, dev, euler_discrete_tables(N), cross_dim=TINY.cross_dim,
                       pooled_dim=TINY.pooled_dim, guidance_scale=G, **kw)
    loop.set_conditioning(*(x[k][1:2].to(dev) for k in KEYS), *(x[k][0:1].to(dev) for k in KEYS))
    return loop


_err = lambda out, ref: float((out.double().cpu() - ref).abs().max())


def test_nine_channel_forward_matches_float64(gpu):
    """Fails without the stem kernel: st_conv2d refuses K = 81 ("neither a multiple of 64 ... nor thin").  Measured on an MI355X:
    1.59e-06 from the float64 module (|ref| max 1.98); gate 1e-3."""
    x = _inputs()
    mask, masked = _condition()
    args = [torch.cat([x["latent"][:1], mask[:, None], masked], dim=1), torch.tensor(500.0), x["encoder_hidden_states"][:1],
            {k: x[k][:1] for k in ("text_embeds", "time_ids")}]
    to = lambda f: [{k: f(v) for k, v in a.items()} if isinstance(a, dict) else f(a) for a in args]
    with torch.no_grad():
        err = _err(_model("cuda:0")(*to(lambda t: t.to(gpu)))[0], _model("cpu")(*to(torch.Tensor.double))[0])
    print(f"nine-channel TINY fp32, one forward: max abs err vs the float64 module {err:.2e}")
    assert err <= ABS_TOL_STRICT


def test_loop_matches_the_float64_loop(gpu):
    """Measured on an MI355X: 3.57e-05 from the float64 loop (|latent| max 42.2; another condition ends 29.31 away); gate 1e-3."""
    with torch.no_grad():
        loop = _loop(gpu)
        assert tuple(loop.x_in.shape) == (2, 4) + HW
        with pytest.raises(RuntimeError, match="set_inpaint_condition"):
            loop.denoise(TU.canvas_noise(HW))
        loop.set_inpaint_condition(*_condition())
        err = _err(loop.denoise(TU.canvas_noise(HW)), _ref())
    moved = float((_ref() - _ref(other=True)).abs().max())
    print(f"nine-channel loop fp32: max abs err vs the float64 loop {err:.2e}; another condition ends {moved:.2f} away")
    assert moved > 100 * ABS_TOL_STRICT, "the condition must matter for this check to mean anything"
    assert err <= ABS_TOL_STRICT


def test_condition_after_capture_and_with_the_blend(gpu):
    noise = TU.canvas_noise(HW)
    with torch.no_grad():
        loop = _loop(gpu)
        loop.capture()
        graph = loop.graph
        loop.set_inpaint_condition(*_condition(other=True))
        first = loop.denoise(noise).cpu()
        loop.set_inpaint_condition(*_condition())
        late = loop.denoise(noise).cpu()
        assert graph is not None and loop.graph is graph and not torch.equal(first, late)
        assert torch.equal(loop.denoise(noise).cpu(), late), "a second identical run must repeat its bits"
        fresh, both = _loop(gpu), _loop(gpu, inpaint=True)
        for l in (fresh, both):
            l.set_inpaint_condition(*_condition())
        both.set_inpaint(IU.init_latent(HW), torch.ones(HW))      # the post-step blend composes: a mask of ones writes nothing
        assert torch.equal(fresh.denoise(noise).cpu(), late), "the bits of a loop that had the condition before its capture"
        assert torch.equal(both.denoise(noise).cpu(), late), "inpaint=True with a mask of ones must give the bits of the loop without it"
    assert _err(late, _ref()) <= ABS_TOL_STRICT
