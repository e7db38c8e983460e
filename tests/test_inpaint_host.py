"""Masked inpainting on the host: the binding and the entry point's argument validation, the CPU route of inpaint.blend against the
tests' own float64 statement (tests/inpaint_util.py), prepare_mask and differential_thresholds, what DenoiseLoop refuses, and the
float64 loop itself (a kept region ends on the init latent; a wrong blend ends outside the loop gate).  No GPU."""
import functools
import math
import os
import re

import pytest
import torch

from stabletriton_amd import _C, inpaint as I, synth
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import inpaint_util as IU
from tests import tiles_util as TU

ABS_TOL_STRICT = 1e-3
G = 5.0


# ------------------------------------------------------------------------------------------------ 1. the binding
def test_binding_header_and_validation(lib):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stabletriton_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int st_inpaint_blend\((.*?)\);", text, flags=re.S)
    assert decl is not None and len(decl.group(1).split(",")) == len(_C.SIGNATURES["st_inpaint_blend"][1]) == 17
    assert hasattr(lib, "st_inpaint_blend")
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    # argument validation happens on the host, before any launch: exercise it without a GPU
    f32, bf = _C.ST_F32, _C.ST_BF16
    # never dereferenced: every call below is rejected first.  latent 2 * 35 * 4 fp32 = 1120 bytes, next_in 2 blocks of that = 2240
    LAT, NXT, INI, NOI, MSK, THR, SIG, SCL, STP = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 30, (1 << 30) + 4096, (1 << 30) + 8192, 1 << 31

    def call(latent=LAT, next_in=NXT, init=INI, noise=NOI, mask=MSK, thr=THR, sigma_next=SIG, in_scale=SCL, step=STP, batch=2, blocks=2,
             HW=35, C=4, mask_rows=1, n_steps=10, dtype=f32):
        return lib.st_inpaint_blend(latent, next_in, init, noise, mask, thr, sigma_next, in_scale, step, batch, blocks, HW, C, mask_rows,
                                    n_steps, dtype, None)

    bad = lambda msg, **kw: call(**kw) != 0 and msg in lib.st_last_error()
    for name in ("latent", "next_in", "init", "noise", "mask", "sigma_next", "in_scale", "step"):
        assert bad(b"null pointer", **{name: None}), name
    assert bad(b"multiple of 4", thr=None, C=6), "thr may be NULL: the call fails on its channel count, not on a null pointer"
    assert bad(b"unsupported dtype", dtype=_C.ST_F32S) and bad(b"unsupported dtype", dtype=7)
    assert bad(b"bad shape", batch=0) and bad(b"bad shape", HW=0) and bad(b"bad shape", C=0) and bad(b"bad shape", n_steps=0)
    assert bad(b"bad shape", batch=-2) and bad(b"bad shape", HW=-35)
    assert bad(b"multiple of 4", C=6) and bad(b"multiple of 4", C=2)
    assert bad(b"must be 1 or the batch", mask_rows=3) and bad(b"must be 1 or the batch", mask_rows=0)
    assert bad(b"must be 1 or the batch", mask_rows=2, batch=4)
    assert bad(b"at least 1", blocks=0) and bad(b"at least 1", blocks=-1)
    for name, at in (("latent", LAT), ("next_in", NXT), ("init", INI), ("noise", NOI)):
        assert bad(b"16 bytes", **{name: at + 8}) and bad(b"16 bytes", **{name: at + 4}), name
    assert bad(b"16 bytes", next_in=NXT + 8, dtype=bf), "next_in is 16-byte aligned in every type"
    for name, at in (("mask", MSK), ("thr", THR), ("sigma_next", SIG), ("in_scale", SCL), ("step", STP)):
        assert bad(b"4 bytes", **{name: at + 2}) and bad(b"4 bytes", **{name: at + 1}), name
    # byte ranges: the same address, one beginning inside the other from either side
    assert bad(b"overlap init", init=LAT) and bad(b"overlap init", init=LAT + 1104) and bad(b"overlap init", init=LAT - 1104)
    assert bad(b"overlap noise", noise=LAT) and bad(b"overlap noise", noise=LAT + 16) and bad(b"overlap noise", noise=LAT - 1104)
    assert bad(b"overlap mask", mask=LAT + 64) and bad(b"overlap mask", mask=LAT - 136) and bad(b"overlap mask", mask=LAT + 1116)
    assert bad(b"overlap mask", mask=LAT - 276, mask_rows=2), "a per-sample mask is batch * HW floats"
    assert bad(b"overlap next_in", next_in=LAT) and bad(b"overlap next_in", next_in=LAT + 1104) and bad(b"overlap next_in", next_in=LAT - 2224)
    assert bad(b"overlap next_in", next_in=LAT - 1104, dtype=bf), "two blocks of bf16: 1120 bytes"
    big = (1 << 31) - 1
    assert bad(b"too large", batch=big, blocks=big, HW=1 << 40) and bad(b"too large", batch=1, blocks=1, HW=1 << 46)
    assert bad(b"too large", batch=big, blocks=1, HW=1 << 12, C=big - 3 - (big - 3) % 4)


def test_launcher_rejects_cpu_tensors():
    from stabletriton_amd import ops
    lat = torch.zeros(1, 4, 5, 7).contiguous(memory_format=torch.channels_last)
    tab = torch.zeros(3)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.inpaint_blend(lat, lat.clone(), lat.clone(), lat.clone(), torch.ones(1, 5, 7), tab, tab, torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ 2. the CPU route
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["ones", "zeros", "binary", "soft", "levels"])
@pytest.mark.parametrize("shape", list(IU.SHAPES))
def test_cpu_route_against_float64(shape, kind, dtype):
    hw, blocks, mask_rows, C = IU.SHAPES[shape]
    for step in (0, IU.N_STEPS - 1):
        case = IU.blend_case(hw, blocks, mask_rows, C, kind, dtype)
        lat, nxt = case[0].clone(), case[1].clone()
        I.blend(lat, nxt, case[2], case[3], case[4], IU.SIGMA_NEXT, IU.IN_SCALE, torch.tensor([step], dtype=torch.int32), case[5])
        IU.check_blend(lat, nxt, case, step, dtype, f"cpu {shape} {kind} {dtype} step {step}")
    if kind == "levels":                                       # a NaN entry of the table: no threshold at that step, the map is the weight
        case = IU.blend_case(hw, blocks, mask_rows, C, kind, dtype)
        lat, nxt = case[0].clone(), case[1].clone()
        I.blend(lat, nxt, case[2], case[3], case[4], IU.SIGMA_NEXT, IU.IN_SCALE, 1, torch.full((IU.N_STEPS,), math.nan))
        IU.check_blend(lat, nxt, case[:5] + (None,), 1, dtype, f"cpu {shape} NaN threshold {dtype}")


def test_cpu_route_errors():
    case = IU.blend_case((5, 7), 2, 1, 4, "binary", torch.float32)
    with pytest.raises(ValueError, match="x_step"):
        I.blend(case[0], case[1][:3], case[2], case[3], case[4], IU.SIGMA_NEXT, IU.IN_SCALE, 0)
    with pytest.raises(ValueError, match="mask"):
        I.blend(case[0], case[1], case[2], case[3], torch.ones(3, 5, 7), IU.SIGMA_NEXT, IU.IN_SCALE, 0)


# ------------------------------------------------------------------------------------------------ 3. masks and thresholds
def test_prepare_mask():
    m = torch.rand(5, 7, generator=torch.Generator().manual_seed(2))
    for given, rows in ((m, 1), (m[None], 1), (m[None, None], 1), (m[None].repeat(3, 1, 1), 3), (m[None, None].repeat(3, 1, 1, 1), 3)):
        out = I.prepare_mask(given, 3, (5, 7))
        assert out.dtype == torch.float32 and tuple(out.shape) == (rows, 5, 7) and out.is_contiguous() and torch.equal(out[0], m)
    assert torch.equal(I.prepare_mask(m.double().numpy(), 1, (5, 7))[0], m.double().float())
    assert torch.equal(I.prepare_mask(torch.tensor([[0, 1], [1, 0]], dtype=torch.bool), 1, (2, 2)), torch.tensor([[[0.0, 1.0], [1.0, 0.0]]]))
    for bad, match in ((torch.ones(7, 5), "not resampled"), (torch.ones(40, 56), "not resampled"), (torch.ones(2, 5, 7), "not resampled"),
                       (torch.ones(3, 2, 5, 7), "not resampled"), (torch.ones(5), "not resampled"),
                       (torch.full((5, 7), math.nan), "finite"), (torch.full((5, 7), math.inf), "finite"),
                       (torch.full((5, 7), -0.1), r"\[0, 1\]"), (torch.full((5, 7), 1.5), r"\[0, 1\]")):
        with pytest.raises(ValueError, match=match):
            I.prepare_mask(bad, 3, (5, 7))
    doc = " ".join(I.__doc__.split())
    assert "unpinned" in doc and "StableDiffusionXLInpaintPipeline" in doc and "Differential Diffusion" in doc
    assert "resampled" in " ".join(I.prepare_mask.__doc__.split())


def test_differential_thresholds():
    for n in (1, 4, 10, 50):
        thr = I.differential_thresholds(n)
        assert thr.dtype == torch.float32 and tuple(thr.shape) == (n,) and float(thr[-1]) == 0.0
        want = torch.tensor([1.0 - (i + 1) / n for i in range(n)], dtype=torch.float64)
        assert float((thr.double() - want).abs().max()) <= 2.0 ** -24
        assert bool((thr[1:] < thr[:-1]).all()) or n == 1
    # a pixel of change-map value m is free (m > thr[i]) for about the last m * n steps; m == 0 never
    thr = I.differential_thresholds(10)
    assert [int((m > thr).sum()) for m in (0.0, 0.25, 0.5, 1.0)] == [0, 3, 5, 10]
    for bad in (0, -3):
        with pytest.raises(ValueError, match="at least 1"):
            I.differential_thresholds(bad)


# ------------------------------------------------------------------------------------------------ 4. the loop's buffers and refusals
def _loop(hw=(16, 16), batch=1, tables=None, **kw):
    return DenoiseLoop(lambda *a, **k: None, batch, hw, torch.float32, "cpu", tables or euler_discrete_tables(4), cross_dim=TINY.cross_dim,
                       pooled_dim=TINY.pooled_dim, mode="eager", **kw)


def test_loop_buffers_and_refusals():
    plain = _loop(guidance_scale=5.0)
    assert plain.inpaint_init is plain.inpaint_noise is plain.inpaint_mask is plain.inpaint_thr is plain.sigma_next is None
    with pytest.raises(ValueError, match="inpaint=True"):
        plain.set_inpaint(torch.zeros(1, 4, 16, 16), torch.ones(16, 16))
    with pytest.raises(ValueError, match="inpaint=True"):
        plain.set_inpaint(None)
    tables = dpmpp_2m_tables(4)
    loop = _loop((16, 24), batch=2, tables=tables, guidance_scale=5.0, tile_hw=16, inpaint=True)
    cl = torch.channels_last
    for t in (loop.inpaint_init, loop.inpaint_noise):           # the canvas, as the latent
        assert tuple(t.shape) == (2, 4, 16, 24) and t.dtype == torch.float32 and t.is_contiguous(memory_format=cl) and not bool(t.any())
    assert tuple(loop.inpaint_mask.shape) == (2, 16, 24) and bool((loop.inpaint_mask == 1).all())
    assert tuple(loop.inpaint_thr.shape) == (4,) and bool(torch.isnan(loop.inpaint_thr).all())
    assert torch.equal(loop.sigma_next, torch.tensor(tables.sigmas[1:], dtype=torch.float32)) and float(loop.sigma_next[-1]) == 0.0
    # in-place writes
    at = [t.data_ptr() for t in (loop.inpaint_init, loop.inpaint_mask, loop.inpaint_thr)]
    init, mask = IU.init_latent((16, 24)), IU.half_mask((16, 24))
    loop.set_inpaint(init, mask)
    assert at == [t.data_ptr() for t in (loop.inpaint_init, loop.inpaint_mask, loop.inpaint_thr)]
    assert torch.equal(loop.inpaint_init, init.expand(2, -1, -1, -1)) and torch.equal(loop.inpaint_mask, mask.expand(2, -1, -1))
    assert bool(torch.isnan(loop.inpaint_thr).all())
    loop.set_inpaint(init, mask[0], differential=True)
    assert torch.equal(loop.inpaint_thr, I.differential_thresholds(4))
    loop.set_inpaint(init, mask[None], differential=True, thresholds=[0.9, 0.5, 0.5, 0.0])
    assert torch.equal(loop.inpaint_thr, torch.tensor([0.9, 0.5, 0.5, 0.0]))
    # refused arguments leave the state as it was
    for args, kw, match in (((init, torch.ones(8, 8)), {}, "not resampled"), ((init, torch.full((16, 24), 2.0)), {}, r"\[0, 1\]"),
                            ((init, torch.full((16, 24), math.nan)), {}, "finite"), ((init[:, :, :8], mask), {}, "init_latent"),
                            ((init.repeat(3, 1, 1, 1), mask), {}, "init_latent"), ((init,), {}, "mask is needed"),
                            ((init, mask), dict(thresholds=[0.5] * 4), "differential=True"),
                            ((init, mask), dict(differential=True, thresholds=[0.5] * 3), "4 values"),
                            ((init, mask), dict(differential=True, thresholds=[0.5, 0.5, 0.5, 1.5]), r"\[0, 1\]"),
                            ((init, mask), dict(differential=True, thresholds=[0.5, math.nan, 0.5, 0.0]), "finite"),
                            ((None, mask), {}, "or None")):
        with pytest.raises(ValueError, match=match):
            loop.set_inpaint(*args, **kw)
    assert torch.equal(loop.inpaint_thr, torch.tensor([0.9, 0.5, 0.5, 0.0])) and torch.equal(loop.inpaint_mask, mask.expand(2, -1, -1))
    loop.set_inpaint(None)
    assert bool((loop.inpaint_mask == 1).all()) and bool(torch.isnan(loop.inpaint_thr).all())


def test_start_noise_is_kept():
    noise = TU.canvas_noise((16, 16), seed=3)
    loop = _loop(inpaint=True)
    loop.set_noise(noise)
    assert torch.equal(loop.inpaint_noise, noise) and torch.equal(loop.latent, noise * loop.tables.init_noise_sigma)
    other = TU.canvas_noise((16, 16), seed=4)
    init = IU.init_latent((16, 16))
    left = loop.set_image(init, other, 0.5)
    assert left == 2 and torch.equal(loop.inpaint_noise, other)
    assert torch.equal(loop.latent, init + other * float(loop.tables.sigmas[2]))
    with pytest.raises(ValueError, match="mode='step' or 'eager'"):
        DenoiseLoop(lambda *a, **k: None, 1, 16, torch.float32, "cpu", euler_discrete_tables(4), inpaint=True).set_image(init, other, 0.5)


# ------------------------------------------------------------------------------------------------ 5. the float64 loop itself
@functools.lru_cache(maxsize=None)
def _model64():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double()


def test_float64_loop_keeps_init_and_tells_a_wrong_blend():
    """Euler 10 steps, g = 5, 16 x 16, the left half kept: loop64's kept half ends exactly on init.  The two distances from loop64:
    the wrong blend (the known region re-noised at sigma[i] instead of sigma[i + 1]) ends 3.85e+00 away in float64 (on the kept half
    alone 1.37e-01, sigma[n - 1] |noise|); the right blend, run in fp32 on an MI355X, ends 4.19e-05 away
    (tests/test_inpaint_loop_gpu.py).  The loop gate ABS_TOL_STRICT = 1e-3 lies between the two, 24 x above the one and 137 x below
    the other at its smallest."""
    hw = (16, 16)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    noise, init, mask = TU.canvas_noise(hw), IU.init_latent(hw), IU.half_mask(hw)
    tables = euler_discrete_tables(10)
    right = IU.loop64(_model64(), x, noise, tables, init, mask, g=G)
    wrong = IU.loop64(_model64(), x, noise, tables, init, mask, g=G, wrong=True)
    plain = IU.loop64(_model64(), x, noise, tables, init, torch.ones(1, 16, 16), g=G)
    kept = (mask == 0)[:, None].expand_as(right)
    assert torch.equal(right[kept], init.double()[kept]), "the kept half must end exactly on init"
    assert float((right - plain)[~kept].abs().max()) > 100 * ABS_TOL_STRICT, "the kept half must matter to the repainted one"
    apart, apart_kept = float((wrong - right).abs().max()), float((wrong - right)[kept].abs().max())
    print(f"float64 inpainting loop: the wrong blend ends {apart:.2e} away (kept half {apart_kept:.2e}); gate {ABS_TOL_STRICT:.0e}")
    assert apart > 10 * ABS_TOL_STRICT and apart_kept > 10 * ABS_TOL_STRICT
    # all ones is the plain loop, all zeros is init
    zeros = IU.loop64(_model64(), x, noise, tables, init, torch.zeros(1, 16, 16), g=G)
    assert torch.equal(zeros, init.double())
