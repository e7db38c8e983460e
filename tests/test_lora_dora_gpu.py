"""The DoRA form of the grouped merge (st_lora_merge with a norm pass, through ops.lora_plan / ops.lora_merge) against float64:

    V_j = B + s_j Up_j Down_j,   g_j[n] = m_j[n] / ||V_j[n]||  (1 for a plain segment),   W64 = B + sum_j (g_j V_j - B).

Every element must satisfy

    |W - W64| <= 1/2 spacing_dtype(W64)
               + sum_j |g_j| ( (r_j + 3) u magV_j + eg_j |V_j| )
               + (J + 2) u ( |B| + sum_j |g_j| |V_j| )
    u = 2^-24,   magV_j = |B| + |s_j| (|Up_j| . |Down_j|),
    eg_j[n] = ( (r_j + 3) ||magV_j[n]|| / ||V_j[n]|| + K / 2 + 4 ) u  for a DoRA segment, 0 for a plain one

- test_lora_gpu.py's bound (final rounding plus an fp32 dot product of r + 1 terms per segment) with each segment scaled by its
gain, the relative error eg of the gain (the error of V carried into its norm, a K-term fp32 sum of squares in any order,
the square root and the division), and the J + 2 roundings of the gain-weighted sum - with no element left out.  Three
adapters at ranks 16 / 8 / 32, scales 0.75 / -1.5 / 0.3, slots 5 / 0 / 2; the first and third are DoRA.  Also: memory
outside a weight is untouched, two merges give equal bits, all scales zero gives the base's bits (-0.0 included), a grouped
plan equals single-target plans bit for bit, a plan without a magnitude is the plain merge, bad magnitudes are refused."""
import pytest
import torch

from stabletriton_amd import ops

pytestmark = pytest.mark.gpu

# (mantissa bits with the implicit one, exponent of the smallest normal)
FORMAT = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SHAPES = [(72, 328),        # partial tiles both ways, 3 K-tiles
          (50, 77),         # odd K: the elementwise path
          (40, 36),         # conv_in-like
          (96, 576),        # a 3x3 conv of 64 channels
          (1000, 640),
          (130, 2304)]      # 18 K-tiles: the cross-tile reduction
RANKS, SCALES, SLOTS, DORA = [16, 8, 32], [0.75, -1.5, 0.3], [5, 0, 2], [True, False, True]
PAD = 64          # guard elements on each side of a weight
U = 2.0 ** -24


def spacing(x64: torch.Tensor, dtype) -> torch.Tensor:
    """Gap between adjacent values of `dtype` at |x|, never below the subnormal spacing."""
    p, emin = FORMAT[dtype]
    _, e = torch.frexp(x64.abs())                       # |x| = m 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    e = torch.where(x64 == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(x64), e - (p - 1))


def _guarded(shape, dtype, dev, fill, pad=PAD):
    n = shape[0] * shape[1]
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    return buf[pad:pad + n].view(shape), buf


def _margins_intact(buf, fill, pad=PAD):
    return bool(torch.all(buf[:pad] == fill) and torch.all(buf[-pad:] == fill))


def _same_bits(a, b) -> bool:
    bits = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def _padded(up, down, dtype):
    """(Up (N, rp), DownT (K, rp)) as the kernel takes them: ranks zero-padded, the down factor transposed."""
    mult = ops.lora_rank_multiple(dtype)
    r = down.shape[0]
    rp = -(-r // mult) * mult
    up_p = torch.zeros((up.shape[0], rp), dtype=dtype, device=up.device)
    down_t = torch.zeros((down.shape[1], rp), dtype=dtype, device=up.device)
    up_p[:, :r] = up
    down_t[:, :r] = down.t()
    return up_p, down_t


class Case:
    """One target: seeded base (0.05 N(0,1)) and factors (0.2 N(0,1)) rounded to dtype, garbage in the live weight, magnitudes
    m[n] = ||V64[n]|| * U(0.5, 1.5) as fp32 for the DoRA segments; the float64 result and its bound, computed once."""

    def __init__(self, shape, dtype, dev, gen):
        n, k = shape
        self.shape, self.dtype = shape, dtype
        self.base = (torch.randn(shape, generator=gen, device=dev) * 0.05).to(dtype)
        self.w, self.buf = _guarded(shape, dtype, dev, 7.0)
        self.w.fill_(-3.0)
        self.facs = [((torch.randn((n, r), generator=gen, device=dev) * 0.2).to(dtype), (torch.randn((r, k), generator=gen, device=dev) * 0.2).to(dtype))
                     for r in RANKS]
        b = self.base.double()
        self.mags, w64, segs, weighted = [], b.clone(), torch.zeros_like(b), b.abs().clone()
        self.norm_ratio = 0.0
        for (u, d), s, r, dora in zip(self.facs, SCALES, RANKS, DORA):
            v = b + s * (u.double() @ d.double())
            mag_v = b.abs() + abs(s) * (u.double().abs() @ d.double().abs())
            if dora:
                m = (v.norm(dim=1) * (0.5 + torch.rand(n, generator=gen, device=dev).double())).float()
                gain = (m.double() / v.norm(dim=1))[:, None]
                ratio = mag_v.norm(dim=1) / v.norm(dim=1)
                self.norm_ratio = max(self.norm_ratio, float(ratio.max()))
                eg = (((r + 3) * ratio + k / 2 + 4) * U)[:, None]
            else:
                m, gain, eg = None, 1.0, 0.0
            self.mags.append(m)
            w64 = w64 + gain * v - b
            segs = segs + abs(gain) * ((r + 3) * U * mag_v + eg * v.abs())
            weighted = weighted + abs(gain) * v.abs()
        self.w64 = w64
        self.bound = 0.5 * spacing(w64, dtype) + segs + (len(RANKS) + 2) * U * weighted

    def entry(self, dora=True):
        facs = [(*_padded(u, d, self.dtype), slot, *([m] if dora else [])) for (u, d), slot, m in zip(self.facs, SLOTS, self.mags)]
        return (self.w, self.base, facs)


def _table(dev, scales=SCALES):
    table = torch.zeros(8, dtype=torch.float32, device=dev)
    for s, v in zip(SLOTS, scales):
        table[s] = v
    return table


_cases = {}


def _cases_of(dtype, dev):
    """The six targets of one dtype, shared by the tests below (their references are never modified)."""
    if dtype not in _cases:
        gen = torch.Generator(device=dev).manual_seed(2024)
        _cases[dtype] = [Case(shape, dtype, dev, gen) for shape in SHAPES]
    return _cases[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_dora_merge_vs_float64(gpu, dtype):
    table = _table(gpu)
    for c in _cases_of(dtype, gpu):
        what = f"{dtype} {c.shape}"
        plan = ops.lora_plan([c.entry()])
        assert plan.dora and plan.segments.shape[1] == ops.LORA_FORM_WORDS
        c.w.fill_(-3.0)
        ops.lora_merge(plan, table)
        torch.cuda.synchronize()
        assert _margins_intact(c.buf, 7.0), f"{what}: wrote outside the weight"
        err = (c.w.double() - c.w64).abs()
        worst = float((err / c.bound).max())
        print(f"{what}: worst |W - W64| / bound = {worst:.3f}, max abs err {float(err.max()):.3e}, max ||magV|| / ||V|| = {c.norm_ratio:.2f}")
        bad = int((~(err <= c.bound)).sum())                   # (a NaN is outside the bound)
        assert bad == 0, f"{what}: {bad} of {err.numel()} elements outside the bound (worst {worst:.3f} of it)"
        first = c.w.clone()
        c.w.fill_(11.0)
        plan.workspace.fill_(float("nan"))                     # nothing may survive from the first merge
        ops.lora_merge(plan, table)
        assert _same_bits(c.w, first), f"{what}: two merges differ"
        assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_scales_zero_gives_the_base_bits(gpu, dtype):
    gen = torch.Generator(device=gpu).manual_seed(7)
    zeros = torch.zeros(8, dtype=torch.float32, device=gpu)
    for shape in SHAPES:
        c = Case(shape, dtype, gpu, gen)
        c.base[::3, ::5] = -0.0
        plan = ops.lora_plan([c.entry()])
        ops.lora_merge(plan, zeros)
        assert _same_bits(c.w, c.base), f"{dtype} {shape}: all scales zero must give the base's bits"
        # only the plain adapter live: the magnitudes of the adapters at scale 0 play no part
        ops.lora_merge(plan, _table(gpu, [0.0, SCALES[1], 0.0]))
        dora_off = c.w.clone()
        ops.lora_merge(ops.lora_plan([(c.w, c.base, c.entry(dora=False)[2][1:2])]), _table(gpu))
        assert _same_bits(c.w, dora_off), f"{dtype} {shape}: DoRA adapters at scale 0 must be skipped whole"
        assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_plan_equals_single_target_plans(gpu, dtype):
    cases = _cases_of(dtype, gpu)
    table = _table(gpu)
    for c in cases:
        c.w.fill_(9.0)
    ops.lora_merge(ops.lora_plan([c.entry() for c in cases]), table)
    grouped = [c.w.clone() for c in cases]
    for c in cases:
        assert _margins_intact(c.buf, 7.0)
        c.w.fill_(9.0)
        ops.lora_merge(ops.lora_plan([c.entry()]), table)
    for c, g in zip(cases, grouped):
        assert _same_bits(c.w, g), f"{dtype} {c.shape}: grouped and single plans differ"
        assert _margins_intact(c.buf, 7.0)
    # a plan that mixes targets with and without DoRA segments: the plain ones get the plain merge's bits
    plain = cases[0]
    ops.lora_merge(ops.lora_plan([plain.entry(dora=False)]), table)
    want = plain.w.clone()
    plain.w.fill_(9.0)
    plan = ops.lora_plan([plain.entry(dora=False), cases[5].entry()])
    assert plan.dora
    ops.lora_merge(plan, table)
    assert _same_bits(plain.w, want) and _same_bits(cases[5].w, grouped[5])


@pytest.mark.parametrize("dtype", DTYPES)
def test_plan_without_a_magnitude_is_the_plain_merge(gpu, dtype):
    cases = _cases_of(dtype, gpu)
    table = _table(gpu)
    entries = [c.entry(dora=False) for c in cases]
    parent_form = ops.lora_plan(entries)
    ops.lora_merge(parent_form, table)
    want = [c.w.clone() for c in cases]
    for c in cases:
        c.w.fill_(9.0)
    plan = ops.lora_plan([(w, b, [(u, d, s, None) for u, d, s in f]) for w, b, f in entries])
    assert not plan.dora and not parent_form.dora and plan.segments.shape == parent_form.segments.shape
    assert plan.segments.shape[1] == ops.LORA_FORM_WORDS
    ops.lora_merge(plan, table)
    for c, g in zip(cases, want):
        assert _same_bits(c.w, g), f"{dtype} {c.shape}"
        assert _margins_intact(c.buf, 7.0)


def test_bad_magnitudes_are_refused_and_nothing_is_written(gpu):
    dtype = torch.bfloat16
    w = torch.full((64, 128), 5.0, dtype=dtype, device=gpu)
    base = torch.zeros_like(w)
    up, down_t = torch.zeros((64, 32), dtype=dtype, device=gpu), torch.zeros((128, 32), dtype=dtype, device=gpu)
    mag = torch.ones(64, dtype=torch.float32, device=gpu)
    with pytest.raises(ops.BackendError, match="magnitude"):
        ops.lora_plan([(w, base, [(up, down_t, 0, mag[:63])])])                   # the wrong length
    with pytest.raises(ops.BackendError, match="magnitude"):
        ops.lora_plan([(w, base, [(up, down_t, 0, mag.to(dtype))])])              # not fp32
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.lora_plan([(w, base, [(up, down_t, 0, mag.cpu())])])                  # not on the device
    plan = ops.lora_plan([(w, base, [(up, down_t, 7, mag.view(64, 1))])])
    with pytest.raises(ops.BackendError, match="at least 8 slots"):
        ops.lora_merge(plan, torch.zeros(4, dtype=torch.float32, device=gpu))
    torch.cuda.synchronize()
    assert bool(torch.all(w == 5.0)), "a refused call must not write"
    ops.lora_merge(plan, torch.zeros(8, dtype=torch.float32, device=gpu))
    assert _same_bits(w, base)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_row_takes_gain_zero(gpu, dtype):
    """A row of V = B + s Up Down that is exactly zero (zero base row, zero up row) has no norm to divide by: its gain is
    defined as 0, the row stays zero and finite, and its neighbours are renormalised as usual.  (72, 328): the vector path
    with partial tiles; (50, 77): the elementwise path."""
    gen = torch.Generator(device=gpu).manual_seed(5)
    for shape in SHAPES[:2]:
        c = Case(shape, dtype, gpu, gen)
        dead = [0, 17, shape[0] - 1]
        c.base[dead] = 0
        u0 = c.facs[0][0].clone()
        u0[dead] = 0
        up_p, down_t = _padded(u0, c.facs[0][1], dtype)
        mag = torch.full((shape[0],), 2.0, dtype=torch.float32, device=gpu)
        ops.lora_merge(ops.lora_plan([(c.w, c.base, [(up_p, down_t, SLOTS[0], mag)])]), _table(gpu))
        torch.cuda.synchronize()
        assert _margins_intact(c.buf, 7.0)
        assert bool(torch.isfinite(c.w).all()), f"{dtype} {shape}: a zero row produced inf / NaN"
        assert bool((c.w[dead] == 0).all()), f"{dtype} {shape}: a zero row must stay zero"
        live = torch.ones(shape[0], dtype=torch.bool, device=gpu)
        live[dead] = False
        # every other row has norm m = 2 up to the rounding of its elements (relative 2^-p each, so 2^-p for the norm) and the
        # gain's relative error eg of the module docstring, with r = 16 and ||magV|| / ||V|| < 5 at these inputs
        tol = 2.0 * (2.0 ** -FORMAT[dtype][0] + (shape[1] / 2 + 100) * U)
        assert float((c.w.double().norm(dim=1)[live] - 2.0).abs().max()) <= tol
