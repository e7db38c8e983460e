"""Self-attention guidance's kernels against float64: the column sums of the softmax matrix (csrc/attention_colsum.hip), the
degrade launch (csrc/sag.hip) and the SAG form of the three sampler updates (csrc/runtime.hip).

Tolerances.  Neither kernel has a closed error bound (fp32 score accumulation, fp32 exp2, fp32 sums in another order than any
reference's), so each is gated at 4x the worst gap between float64 and a plain fp32 torch evaluation of the SAME formula on the same
rounded inputs, taken over all cases of the test - a number that comes from the references alone, printed with the kernel's own
figure.  The degrade output is one rounding away from its float64 value: 1 ulp of the output type on top."""
import functools

import pytest
import torch

from stabletriton_amd import ops, sag
from tests import pag_util as PU
from tests.test_pag_gpu import ROUND, ULP, _Case, _seeds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# the kernel's only tile is 64 rows / 64 keys: one tile; a one-key tail; tails of 2 and of 1 behind 2 and 4 tiles; 7 tiles + 1 with
# three batch entries; and 40, the boundary this tiling adds: fewer keys than a tile, lanes whose keys all lie past T
COLSUM_SHAPES = [(2, 64, 1), (2, 65, 3), (1, 130, 2), (1, 257, 3), (3, 449, 1), (1, 40, 2)]
DTYPES = [torch.bfloat16, torch.float16]


def _qk(shape, dtype, gain):
    """q and k as column slices of one fused (B, T, 3 H D) buffer, unit normal times `gain` (4: peaked rows)."""
    B, T, H = shape
    gen = torch.Generator().manual_seed(1000 * T + 10 * H + B)
    qkv = (torch.randn((B, T, 3 * H * 64), generator=gen) * gain).to(DEV, dtype)
    return qkv[..., :H * 64], qkv[..., H * 64:2 * H * 64]


def _colsum64(q, k, H):
    B, T, _ = q.shape
    heads = lambda t: t.double().reshape(B, T, H, 64).transpose(1, 2)
    return torch.softmax(heads(q) @ heads(k).transpose(-2, -1) * 0.125, dim=-1).sum(dim=2).mean(dim=1)


@functools.lru_cache(maxsize=None)
def _colsum_gap():
    """The worst relative gap of the fp32 torch evaluation (sag.colsum_reference) from float64 over every case."""
    worst = 0.0
    for shape in COLSUM_SHAPES:
        for dtype in DTYPES:
            for gain in (1.0, 4.0):
                q, k = _qk(shape, dtype, gain)
                ref = _colsum64(q, k, shape[2])
                worst = max(worst, float(((sag.colsum_reference(q, k, shape[2], 0.125).double() - ref).abs() / ref).max()))
    return worst


@pytest.mark.parametrize("gain", [1.0, 4.0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", COLSUM_SHAPES)
def test_attention_colsum_vs_float64(gpu, shape, dtype, gain):
    B, T, H = shape
    q, k = _qk(shape, dtype, gain)
    ref = _colsum64(q, k, H)
    gate = 4.0 * _colsum_gap()
    out = ops.attention_colsum(q, k, H, 0.125)
    assert torch.equal(out, ops.attention_colsum(q, k, H, 0.125)), "two calls differ"
    err = float(((out.double() - ref).abs() / ref).max())
    total = float((out.double().sum(dim=1) - T).abs().max() / T)
    print(f"colsum {shape} {dtype} gain {gain}: max rel err {err:.2e}, |sum - T| / T {total:.2e}, gate {gate:.2e} (fp32 torch gap {gate / 4:.2e})")
    assert err <= gate and total <= gate
    if B > 1:                                       # rows < B: the entries at or past `rows` are left alone
        keep = torch.full((B, T), -7.0, device=DEV)
        ops.attention_colsum(q, k, H, 0.125, rows=B - 1, out=keep)
        assert torch.equal(keep[:B - 1], out[:B - 1]) and bool((keep[B - 1:] == -7.0).all())


DEGRADE_CASES = [((8, 8), (2, 2)), ((12, 20), (3, 5)), ((32, 32), (8, 8))]
STEP, N_STEPS, THRESHOLD = 3, 6, 1.0


def _degrade_inputs(hw, grid, batch=2):
    gen = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    cl = torch.channels_last
    x = (torch.randn((batch, 4, *hw), generator=gen) * 3.0).to(DEV).contiguous(memory_format=cl)
    e = torch.randn((batch, 4, *hw), generator=gen)
    amap = torch.where(torch.rand((batch, grid[0] * grid[1]), generator=gen) < 0.5, 0.25, 1.75).to(DEV)      # no cell near the threshold
    sigmas = torch.linspace(9.0, 0.5, N_STEPS, device=DEV)
    in_scale = 1.0 / (sigmas ** 2 + 1.0).sqrt()
    return x, e, amap, sigmas, in_scale


@functools.lru_cache(maxsize=None)
def _degrade_gap():
    """The worst absolute gap of the fp32 torch evaluation of sag.degrade_reference from float64 over every case (16-bit eps)."""
    worst = 0.0
    for hw, grid in DEGRADE_CASES:
        for blur in (0.5, 2.0):
            x, e, amap, sigmas, in_scale = _degrade_inputs(hw, grid)
            e = e.to(DEV, torch.bfloat16)
            args = (amap, grid, float(sigmas[STEP]), float(in_scale[STEP]), THRESHOLD, blur)
            worst = max(worst, float((sag.degrade_reference(x, e.float(), *args)[0].double()
                                      - sag.degrade_reference(x.double(), e.double(), *args)[0]).abs().max()))
    return worst


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32])
@pytest.mark.parametrize("blur", [0.5, 2.0])
@pytest.mark.parametrize("case", DEGRADE_CASES)
def test_sag_degrade_vs_float64(gpu, case, blur, dtype):
    hw, grid = case
    x, e, amap, sigmas, in_scale = _degrade_inputs(hw, grid)
    e = e.to(DEV, dtype).contiguous(memory_format=torch.channels_last)
    step = torch.tensor([STEP], dtype=torch.int32, device=DEV)
    params = torch.tensor([THRESHOLD, blur], device=DEV)
    out = torch.full_like(e, float("nan"))
    mask = torch.full((x.shape[0], *hw), -1.0, device=DEV)
    ops.sag_degrade(x, e, amap, grid, sigmas, in_scale, step, params, out, mask)
    ref, ref_mask = sag.degrade_reference(x.double(), e.double(), amap, grid, float(sigmas[STEP]), float(in_scale[STEP]), THRESHOLD, blur)
    assert torch.equal(mask, ref_mask.float()), "the written mask differs from the reference mask"
    assert 0.0 < float(mask.mean()) < 1.0
    rel, absolute = ROUND[dtype]
    err = (out.double() - ref).abs()
    gate = 4.0 * _degrade_gap()
    print(f"degrade {case} blur {blur} {dtype}: max abs err {float(err.max()):.2e}; fp32 torch gap {gate / 4:.2e}")
    assert float((err - rel * ref.abs() - absolute - gate).max()) <= 0.0


@pytest.mark.parametrize("dtype", DTYPES + [torch.float32])
@pytest.mark.parametrize("phi", [None, 0.7])
@pytest.mark.parametrize("kind", ["euler", "dpm_first", "dpm_second", "sde"])
def test_sag_step_kernels(gpu, kind, phi, dtype):
    """sag = 0: the two-way kernel's latent, next_in and history bit for bit; sag = 0.5: the float64 formula at the tolerance of the
    existing update tests (tests/test_pag_gpu.py)."""
    case = _Case(kind, gpu)
    n, i, batch = case.n, case.i, 2
    shape = (batch, 4, 12, 20)
    cl = torch.channels_last
    gen = torch.Generator().manual_seed(7)
    lat0 = (torch.randn(shape, generator=gen) * 2.0).to(gpu).contiguous(memory_format=cl)
    hist0 = (torch.randn(shape, generator=gen) * 1.5).to(gpu).contiguous(memory_format=cl)
    eps = torch.randn((2 * batch, *shape[1:]), generator=gen).to(gpu, dtype).contiguous(memory_format=cl)
    e_sag = (eps[:batch].float() * 0.8 + 0.3 * torch.randn(shape, generator=gen).to(gpu)).to(dtype).contiguous(memory_format=cl)
    guidance = torch.linspace(1.0, 9.0, n, device=gpu)
    rescale = torch.full((n,), phi, device=gpu) if phi is not None else None
    seed_vals = [12345, 12352]
    seeds = _seeds(seed_vals, gpu)

    def run(table):
        lat, hist, nxt = lat0.clone(), hist0.clone(), torch.zeros_like(eps)
        if table is None:
            case.launch(lat, eps, nxt, hist, seeds, guidance, rescale, None)
        elif kind == "euler":
            ops.sag_euler_step(lat, eps, e_sag, nxt, case.dsigma, case.in_scale, guidance, table, case.step, rescale=rescale)
        elif kind == "sde":
            ops.sag_sde_step(lat, eps, e_sag, nxt, hist, case.coef, case.in_scale, case.step, case.start, seeds, table, guidance, rescale=rescale)
        else:
            ops.sag_dpmpp2m_step(lat, eps, e_sag, nxt, hist, case.coef, case.in_scale, case.step, case.start, table, guidance, rescale=rescale)
        return lat, hist, nxt

    for got, want in zip(run(torch.zeros(n, device=gpu)), run(None)):
        assert torch.equal(got, want), "sag = 0 differs from the two-way kernel"
    lat, hist, nxt = run(torch.full((n,), 0.5, device=gpu))
    e_neg, e_pos = eps.float().cpu().split(batch)
    g, diff = float(guidance[i]), e_neg.double() - e_sag.float().cpu().double()
    e = PU.guide64(e_neg, e_pos, e_pos, g, 0.0, phi) + 0.5 * diff
    emag = PU.guide_magnitude(e_neg, e_pos, e_pos, g, 0.0, phi) + 0.5 * diff.abs()
    z = None
    if kind == "sde":
        from stabletriton_amd import rng
        z = torch.from_numpy(rng.normal(seed_vals, i + 1, 4 * 12 * 20)).view(batch, 12, 20, 4).permute(0, 3, 1, 2)
    ref, d, xmag, dmag = case.restated(lat0.cpu(), e, emag, hist0.cpu(), z)
    err = (lat.cpu().double() - ref).abs()
    print(f"sag {kind} phi {phi} {dtype}: latent max abs err vs float64 {float(err.max()):.2e}")
    assert float((err - 8 * ULP * xmag).max()) <= 0.0
    if d is not None:
        assert float(((hist.cpu().double() - d).abs() - 8 * ULP * dmag).max()) <= 0.0
    rel, absolute = ROUND[dtype]
    want = ref * case.sc
    assert torch.equal(nxt[:batch], nxt[batch:])
    assert float(((nxt[:batch].cpu().double() - want).abs() - rel * want.abs() - absolute - 8 * ULP * xmag * case.sc).max()) <= 0.0
