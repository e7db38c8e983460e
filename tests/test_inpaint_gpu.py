"""The inpainting blend kernel (csrc/inpaint.hip) alone, in guarded buffers, per element against the tests' float64 statement
(tests/inpaint_util.py): nothing is written where w == 1 (latent and next_in are NaN-poisoned there beforehand and compared bit for
bit), w == 0 at sigma 0 gives init bit for bit, everything else stays inside the format-derived bounds (latent: 2^-22 (|init| +
|s noise| + |latent_in|); next_in: one ulp of its type at the float64 value plus the latent's bound times the scale), all row blocks of
next_in are equal, the guard regions behind the buffers are intact, and two launches give the same bits."""
import math

import pytest
import torch

from stabletriton_amd import inpaint as I, ops
from tests import inpaint_util as IU
from tests.edge_util import assert_margins_intact, guarded

pytestmark = pytest.mark.gpu


def _launch(case, step, dtype, gpu, thr="case"):
    """One launch on guarded copies of the case: (latent, its buffer, next_in, its buffer).  Where w == 1 the latent handed to the
    kernel is NaN (a read-modify-write there would store NaN arithmetic, a skipped pixel keeps the NaN's bits), and next_in is NaN
    everywhere."""
    lat, nxt, init, noise, mask, case_thr = case
    thr = case_thr if thr == "case" else thr
    B = lat.shape[0]
    i = step
    w = IU.weight64(mask, None if thr is None or math.isnan(float(thr[i])) else float(thr[i]))
    poisoned = torch.where((w == 1).expand_as(lat), torch.full_like(lat, math.nan), lat)
    glat, lbuf = guarded(tuple(lat.shape), torch.float32, gpu, channels_last=True)
    glat.copy_(poisoned)
    gnext, nbuf = guarded(tuple(nxt.shape), dtype, gpu, channels_last=True)
    dev = lambda t: None if t is None else t.to(gpu)
    cl = lambda t: t.to(gpu).contiguous(memory_format=torch.channels_last)
    ops.inpaint_blend(glat, gnext, cl(init), cl(noise), dev(mask), dev(IU.SIGMA_NEXT), dev(IU.IN_SCALE),
                      torch.tensor([step], dtype=torch.int32, device=gpu), dev(thr))
    torch.cuda.synchronize()
    return glat, lbuf, gnext, nbuf, poisoned


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("kind", ["ones", "zeros", "binary", "soft", "levels"])
@pytest.mark.parametrize("shape", list(IU.SHAPES))
def test_kernel_against_float64(gpu, shape, kind, dtype):
    hw, blocks, mask_rows, C = IU.SHAPES[shape]
    case = IU.blend_case(hw, blocks, mask_rows, C, kind, dtype)
    worst = [0.0, 0.0]
    for step in (0, IU.N_STEPS - 1):                            # the last step: in_scale clamps, sigma_next is 0
        what = f"{shape} {kind} {dtype} step {step}"
        glat, lbuf, gnext, nbuf, poisoned = _launch(case, step, dtype, gpu)
        assert_margins_intact(lbuf, f"{what} latent")
        assert_margins_intact(nbuf, f"{what} next_in")
        got = glat.cpu()
        w = IU.weight64(case[4], None if case[5] is None else float(case[5][step]))
        repaint = (w == 1).expand_as(got)
        assert bool(torch.isnan(got[repaint]).all()), f"{what}: latent written where w == 1"
        assert torch.equal(got[repaint].view(torch.int32), poisoned[repaint].view(torch.int32)), f"{what}: the bits where w == 1 changed"
        # the values the kernel did not touch are the sampler's: put them back for the per-element check
        fl, fn = IU.check_blend(torch.where(repaint, case[0], got), gnext, case, step, dtype, what)
        worst = [max(worst[0], fl), max(worst[1], fn)]
        again = _launch(case, step, dtype, gpu)
        assert torch.equal(again[0].cpu()[~repaint], got[~repaint]) and torch.equal(again[2].cpu()[~repaint.repeat(blocks, 1, 1, 1)],
                                                                                   gnext.cpu()[~repaint.repeat(blocks, 1, 1, 1)])
    if kind == "ones":
        assert bool(repaint.all()), "mask all ones: the launch writes nothing at all"
    print(f"inpaint_blend {shape} {kind} {dtype}: worst fractions of the bounds: latent {worst[0]:.3f}, next_in {worst[1]:.3f}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_threshold_forms(gpu, dtype):
    """thr == NULL and a table of NaN are the same launch result (the mask is the weight); a real table thresholds the map; *step and
    the tables are read when the kernel runs."""
    hw, blocks, mask_rows, C = IU.SHAPES["257x1_b3_mB"]
    case = IU.blend_case(hw, blocks, mask_rows, C, "levels", dtype)
    nan_table = torch.full((IU.N_STEPS,), math.nan)
    null = _launch(case, 1, dtype, gpu, thr=None)
    nans = _launch(case, 1, dtype, gpu, thr=nan_table)
    soft_case = case[:5] + (None,)
    IU.check_blend(torch.where(torch.isnan(null[0].cpu()), case[0], null[0].cpu()), null[2], soft_case, 1, dtype, "thr NULL")
    assert torch.equal(null[0].cpu().view(torch.int32), nans[0].cpu().view(torch.int32))
    assert torch.equal(null[2].cpu().view(torch.int16 if dtype != torch.float32 else torch.int32),
                       nans[2].cpu().view(torch.int16 if dtype != torch.float32 else torch.int32))
    hard = _launch(case, 1, dtype, gpu)                         # thr[1] = 0.5: the 0.5 band is frozen, bit-equal to "keep"
    assert not torch.equal(hard[0].cpu().view(torch.int32), null[0].cpu().view(torch.int32))
    IU.check_blend(torch.where(torch.isnan(hard[0].cpu()), case[0], hard[0].cpu()), hard[2], case, 1, dtype, "thr table")


def test_route_through_inpaint_module_and_refusals(gpu):
    hw, blocks, mask_rows, C = IU.SHAPES["5x7_b2_mB"]
    case = IU.blend_case(hw, blocks, mask_rows, C, "soft", torch.bfloat16)
    dev = [t.to(gpu) for t in case[:5]]
    dev[1].zero_()
    cpu = [t.clone() for t in case[:5]]
    cpu[1].zero_()
    step = torch.tensor([2], dtype=torch.int32)
    I.blend(*dev, IU.SIGMA_NEXT.to(gpu), IU.IN_SCALE.to(gpu), step.to(gpu))
    I.blend(*cpu, IU.SIGMA_NEXT, IU.IN_SCALE, step)
    # the CPU route restates the kernel's arithmetic: fused multiply-adds but for a double rounding 2^-29 below the fp32 ulp
    assert float((dev[0].cpu() - cpu[0]).abs().max()) <= 2.0 ** -22 * float(case[0].abs().max())
    assert float((dev[1].cpu().double() - cpu[1].double()).abs().max()) <= float(IU.ulp(cpu[1].double(), torch.bfloat16).max())
    lat, nxt, init, noise, mask = (t.to(gpu) for t in case[:5])
    sig, scl, st = IU.SIGMA_NEXT.to(gpu), IU.IN_SCALE.to(gpu), step.to(gpu)
    with pytest.raises(ops.BackendError, match="channels_last"):
        ops.inpaint_blend(lat.contiguous(), nxt, init, noise, mask, sig, scl, st)
    with pytest.raises(ops.BackendError, match="init must be"):
        ops.inpaint_blend(lat, nxt, init[:1], noise, mask, sig, scl, st)
    with pytest.raises(ops.BackendError, match="next_in must be"):
        ops.inpaint_blend(lat, nxt[:3], init, noise, mask, sig, scl, st)
    with pytest.raises(ops.BackendError, match="mask must be"):
        ops.inpaint_blend(lat, nxt, init, noise, mask.half(), sig, scl, st)
    with pytest.raises(ops.BackendError, match="thr must be"):
        ops.inpaint_blend(lat, nxt, init, noise, mask, sig, scl, st, sig[:3])
    with pytest.raises(ops.BackendError, match="int32"):
        ops.inpaint_blend(lat, nxt, init, noise, mask, sig, scl, st.long())
    with pytest.raises(ops.BackendError, match="overlap init"):
        ops.inpaint_blend(lat, nxt, lat, noise, mask, sig, scl, st)
