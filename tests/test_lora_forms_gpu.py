"""The LoHa and LoKr segment kinds of the grouped merge (st_lora_merge with `forms` set, through ops.lora_plan / ops.lora_merge) against
float64 restatements written here.  Per segment, from the tables the kernel reads (factor pairs rounded to the dtype, LoKr's
two fp32 tables):

    plain  D = Up Down                      M = |Up| |Down|                            c = r + 1
    LoHa   D = (Up1 Down1) (.) (Up2 Down2)   M = (|Up1| |Down1|) (.) (|Up2| |Down2|)    c = r1 + r2 + 4
    LoKr   D[i c + p, col(j, q, tap)] = W1[i, j] W2[p, q, tap]      M = |D|            c = 2

Without a magnitude every element must satisfy, with u = 2^-24 and J segments,

    |W - W64| <= 1/2 spacing(W64) + u sum_j |s_j| c_j M_j + (J + 2) u (|B| + sum_j |s_j| M_j),      W64 = B + sum_j s_j D_j

(c_j roundings on the way to a segment's scaled delta - the dot products, their product, the fma - and J + 2 for the sums).
With DoRA magnitudes the bound is test_lora_dora_gpu.py's, c_j standing where it has r_j + 3 and magV_j = |B| + |s_j| M_j:

    V_j = B + s_j D_j,  g_j[n] = m_j[n] / ||V_j[n]||,  W64 = B + sum_j (g_j V_j - B)
    |W - W64| <= 1/2 spacing(W64) + sum_j |g_j| (c_j u magV_j + eg_j |V_j|) + (J + 2) u (|B| + sum_j |g_j| |V_j|)
    eg_j[n] = (c_j ||magV_j[n]|| / ||V_j[n]|| + K / 2 + 4) u  for a DoRA segment, 0 otherwise

No element is left out.  Three adapters on one weight: plain rank 16, LoHa ranks 8 and 24, LoKr with w2 = a rank-8 product,
at scales 0.75 / -1.5 / 0.3 in slots 5 / 0 / 2.  Shapes are the smallest that take each path (SHAPES).  Also the bit
identities that tie the kernels that form every kind to the lean ones, the lean kernels' skip of a row they cannot form, guard
margins, and refused tables.

Worst |W - W64| / bound measured on an MI355X: see DESIGN.md section 4 (the adapter forms)."""
import pytest
import torch

from stabletriton_amd import _C, ops

pytestmark = pytest.mark.gpu

FORMAT = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (N, K), LoKr (a, b), taps, layout
SHAPES = [((72, 328), (4, 8), 1, 0),         # partial tiles both ways, 3 K-tiles, d = 41: the elementwise index path
          ((50, 77), (5, 7), 1, 0),          # odd K: no 16-byte path
          ((192, 1152), (8, 16), 9, 1),      # a 3x3 conv over 128 channels, channels_last: d = 8, the vector path
          ((192, 1152), (8, 16), 9, 0),      # the same conv, contiguous: d taps = 72
          ((130, 36), (2, 4), 1, 0),         # conv_in-like: K below one tile
          ((64, 2304), None, 1, 0)]          # 18 K-tiles: the DoRA reduction (no LoKr segment)
R_PLAIN, R_HADA, R_KRON = 16, (8, 24), 8
SCALES, SLOTS = [0.75, -1.5, 0.3], [5, 0, 2]
PAD = 64
U = 2.0 ** -24


def spacing(x64, dtype):
    p, emin = FORMAT[dtype]
    _, e = torch.frexp(x64.abs())
    e = torch.where(x64 == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(x64), e - (p - 1))


def _guarded(shape, dtype, dev, fill, pad=PAD):
    n = shape[0] * shape[1]
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    return buf[pad:pad + n].view(shape), buf


def _margins_intact(buf, fill, pad=PAD):
    return bool(torch.all(buf[:pad] == fill) and torch.all(buf[-pad:] == fill))


def _same_bits(a, b):
    bits = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def _padded(up, down, dtype):
    mult = ops.lora_rank_multiple(dtype)
    r = down.shape[0]
    rp = -(-r // mult) * mult
    up_p = torch.zeros((up.shape[0], rp), dtype=dtype, device=up.device)
    down_t = torch.zeros((down.shape[1], rp), dtype=dtype, device=up.device)
    up_p[:, :r] = up
    down_t[:, :r] = down.t()
    return up_p, down_t


def kron64(w1, w2, taps, layout):
    """float64 D[i c + p, k] = W1[i, j] W2[p, col]; k = tap (b d) + j d + q, col = tap d + q (layout 1) or k = (j d + q) taps
    + tap, col = q taps + tap (layout 0) - written with explicit index tensors, not with the code under test's reshapes."""
    (a, b), c, d = w1.shape, w2.shape[0], w2.shape[1] // taps
    k = torch.arange(b * d * taps, device=w1.device)
    if layout:
        tap, ch = k // (b * d), k % (b * d)
        j, col = ch // d, tap * d + ch % d
    else:
        ch, tap = k // taps, k % taps
        j, col = ch // d, (ch % d) * taps + tap
    n = torch.arange(a * c, device=w1.device)
    return w1.double()[(n // c)[:, None], j[None, :]] * w2.double()[(n % c)[:, None], col[None, :]]


class Case:
    """One target: seeded base (0.05 N(0,1)) and factor pairs (0.2 N(0,1)) rounded to dtype, LoKr tables W1 = 0.5 N(0,1) and
    W2 = the fp32 product of two 0.2 N(0,1) rank-8 factors; garbage in the live weight; the float64 results and their bounds,
    with and without magnitudes m[n] = ||V64[n]|| U(0.5, 1.5), computed once."""

    def __init__(self, spec, dtype, dev, gen):
        shape, ab, taps, layout = spec
        n, k = shape
        self.shape, self.dtype, self.what = shape, dtype, f"{dtype} {shape} layout {layout}"
        rn = lambda *s: torch.randn(s, generator=gen, device=dev)                     # noqa: E731
        self.base = (rn(n, k) * 0.05).to(dtype)
        self.w, self.buf = _guarded(shape, dtype, dev, 7.0)
        self.w.fill_(-3.0)
        pair = lambda r: ((rn(n, r) * 0.2).to(dtype), (rn(r, k) * 0.2).to(dtype))       # noqa: E731
        plain, h1, h2 = pair(R_PLAIN), pair(R_HADA[0]), pair(R_HADA[1])
        ad = lambda u, d: u.double().abs() @ d.double().abs()                          # noqa: E731
        pr = lambda u, d: u.double() @ d.double()                                      # noqa: E731
        # (factor tuple without slot and magnitude, D64, M, c)
        self.segs = [((*_padded(*plain, dtype),), pr(*plain), ad(*plain), R_PLAIN + 1),
                     (("hada", *_padded(*h1, dtype), *_padded(*h2, dtype)), pr(*h1) * pr(*h2), ad(*h1) * ad(*h2), sum(R_HADA) + 4)]
        if ab is not None:
            a, b = ab
            c, d = n // a, k // (b * taps)
            w1 = (rn(a, b) * 0.5).contiguous()
            w2 = ((rn(c, R_KRON) * 0.2) @ (rn(R_KRON, d * taps) * 0.2)).contiguous()
            d64 = kron64(w1, w2, taps, layout)
            self.segs.append((("kron", w1, w2, taps, layout), d64, d64.abs(), 2))
        b64 = self.base.double()
        nseg = len(self.segs)
        # without magnitudes
        w64, m_sum, c_sum = b64.clone(), b64.abs().clone(), torch.zeros_like(b64)
        for (_, d64, m, c), s in zip(self.segs, SCALES):
            w64 += s * d64
            m_sum += abs(s) * m
            c_sum += abs(s) * c * m
        self.w64 = w64
        self.bound = 0.5 * spacing(w64, dtype) + U * c_sum + (nseg + 2) * U * m_sum
        # DoRA over every segment
        self.mags, w64, segs, weighted = [], b64.clone(), torch.zeros_like(b64), b64.abs().clone()
        self.norm_ratio = 0.0
        for (_, d64, m, c), s in zip(self.segs, SCALES):
            v = b64 + s * d64
            mag_v = b64.abs() + abs(s) * m
            mag = (v.norm(dim=1) * (0.5 + torch.rand(n, generator=gen, device=dev).double())).float()
            gain = (mag.double() / v.norm(dim=1))[:, None]
            ratio = mag_v.norm(dim=1) / v.norm(dim=1)
            self.norm_ratio = max(self.norm_ratio, float(ratio.max()))
            eg = ((c * ratio + k / 2 + 4) * U)[:, None]
            self.mags.append(mag)
            w64 = w64 + gain * v - b64
            segs = segs + gain.abs() * (c * U * mag_v + eg * v.abs())
            weighted = weighted + gain.abs() * v.abs()
        self.w64_dora = w64
        self.bound_dora = 0.5 * spacing(w64, dtype) + segs + (nseg + 2) * U * weighted

    def entry(self, dora=False, only=None):
        facs = []
        for i, ((f, _, _, _), slot, m) in enumerate(zip(self.segs, SLOTS, self.mags)):
            if only is None or i in only:
                facs.append((*f, slot, *([m] if dora else [])))
        return (self.w, self.base, facs)


def _table(dev, scales=SCALES):
    table = torch.zeros(8, dtype=torch.float32, device=dev)
    for s, v in zip(SLOTS, scales):
        table[s] = v
    return table


_cases = {}


def _cases_of(dtype, dev):
    if dtype not in _cases:
        gen = torch.Generator(device=dev).manual_seed(2025)
        _cases[dtype] = [Case(spec, dtype, dev, gen) for spec in SHAPES]
    return _cases[dtype]


@pytest.mark.parametrize("dora", [False, True], ids=["plain", "dora"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_forms_merge_vs_float64(gpu, dtype, dora):
    table = _table(gpu)
    for c in _cases_of(dtype, gpu):
        plan = ops.lora_plan([c.entry(dora)])
        assert plan.forms and plan.dora == dora and plan.segments.shape[1] == ops.LORA_FORM_WORDS
        c.w.fill_(-3.0)
        ops.lora_merge(plan, table)
        torch.cuda.synchronize()
        assert _margins_intact(c.buf, 7.0), f"{c.what}: wrote outside the weight"
        w64, bound = (c.w64_dora, c.bound_dora) if dora else (c.w64, c.bound)
        err = (c.w.double() - w64).abs()
        worst = float((err / bound).max())
        print(f"{c.what} dora={dora}: worst |W - W64| / bound = {worst:.3f}, max abs err {float(err.max()):.3e}"
              + (f", max ||magV|| / ||V|| = {c.norm_ratio:.2f}" if dora else ""))
        bad = int((~(err <= bound)).sum())                     # (a NaN is outside the bound)
        assert bad == 0, f"{c.what}: {bad} of {err.numel()} elements outside the bound (worst {worst:.3f} of it)"
        first = c.w.clone()
        c.w.fill_(11.0)
        if dora:
            plan.workspace.fill_(float("nan"))                 # nothing may survive from the first merge
        ops.lora_merge(plan, table)
        assert _same_bits(c.w, first), f"{c.what}: two merges differ"
        assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_plain_tables_through_the_new_entry_point_keep_their_bits(gpu, dtype):
    """Plain segments through the kernels that form every kind (`forms`) give the lean kernels' bits, with and without magnitudes."""
    table = _table(gpu)
    for c in _cases_of(dtype, gpu):
        for dora in (False, True):
            entry = c.entry(dora, only=[0])
            old = ops.lora_plan([entry])
            assert not old.forms and old.dora == dora
            ops.lora_merge(old, table)
            want = c.w.clone()
            c.w.fill_(9.0)
            new = ops.lora_plan([entry], forms=True)
            assert new.forms and new.dora == dora
            ops.lora_merge(new, table)
            assert _same_bits(c.w, want), f"{c.what} dora={dora}"
            assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lean_kernels_skip_a_row_that_is_not_plain(gpu, dtype):
    """st_lora_merge with forms = 0 over a table that holds a HADA row: the lean kernels drop the row and give the bits of the plan
    that holds the plain segment alone, without and with a magnitude on it.  HADA only: the row's first pair is a valid plain
    factor pair, so a missing guard shows as wrong bits (the product of that pair is added), never as a read out of bounds."""
    table = _table(gpu)
    lib = _C.load()
    for c in _cases_of(dtype, gpu):
        if c.shape not in ((50, 77), (72, 328)):
            continue
        for dora in (False, True):
            ops.lora_merge(ops.lora_plan([c.entry(dora, only=[0])]), table)
            want = c.w.clone()
            plan = ops.lora_plan([(c.w, c.base, [c.entry(dora, only=[0])[2][0], c.entry(only=[1])[2][0]])])
            assert plan.forms and plan.dora == dora and plan.n_segments == 2
            ops.lora_merge(plan, table)
            assert not _same_bits(c.w, want), f"{c.what} dora={dora}: the HADA row is live when the table's flag is right"
            c.w.fill_(9.0)
            norm, ws = plan.norm_tiles, plan.workspace
            rc = lib.st_lora_merge(plan.targets.data_ptr(), plan.n_targets, plan.segments.data_ptr(), plan.n_segments, plan.max_rank,
                                   plan.tiles.data_ptr(), plan.n_tiles, None if norm is None else norm.data_ptr(),
                                   0 if norm is None else norm.shape[0], table.data_ptr(), table.numel(),
                                   None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4,
                                   _C.dtype_code(dtype), 0, _C.stream_ptr())
            assert rc == 0, lib.st_last_error()
            torch.cuda.synchronize()
            assert _same_bits(c.w, want), f"{c.what} dora={dora}: forms = 0 must drop the HADA row and nothing else"
            assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_hada_with_a_pair_of_ones_is_the_plain_segment(gpu, dtype):
    """(Up Down) (.) (1 1^T) = Up Down: rank-1 factors of ones, zero-padded, make the second product exactly 1."""
    table = _table(gpu)
    for c in _cases_of(dtype, gpu):
        n, k = c.shape
        up, down_t = c.segs[0][0]
        ops.lora_merge(ops.lora_plan([(c.w, c.base, [(up, down_t, SLOTS[0])])]), table)
        want = c.w.clone()
        c.w.fill_(9.0)
        ones_u, ones_d = _padded(torch.ones((n, 1), dtype=dtype, device=gpu), torch.ones((1, k), dtype=dtype, device=gpu), dtype)
        plan = ops.lora_plan([(c.w, c.base, [("hada", up, down_t, ones_u, ones_d, SLOTS[0])])])
        assert plan.forms
        ops.lora_merge(plan, table)
        assert _same_bits(c.w, want), c.what
        assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_kron_with_unit_w1_adds_w2_rounded_once(gpu, dtype):
    gen = torch.Generator(device=gpu).manual_seed(11)
    ones = torch.ones(8, dtype=torch.float32, device=gpu)
    for c in _cases_of(dtype, gpu):
        n, k = c.shape
        w2 = (torch.randn(c.shape, generator=gen, device=gpu) * 0.1).contiguous()
        w1 = torch.ones((1, 1), dtype=torch.float32, device=gpu)
        c.w.fill_(9.0)
        ops.lora_merge(ops.lora_plan([(c.w, c.base, [("kron", w1, w2, 1, 0, 3)])]), ones)
        assert _same_bits(c.w, (c.base.float() + w2).to(dtype)), c.what
        assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_plan_equals_single_target_plans(gpu, dtype):
    cases = _cases_of(dtype, gpu)
    table = _table(gpu)
    for dora in (False, True):
        for c in cases:
            c.w.fill_(9.0)
        ops.lora_merge(ops.lora_plan([c.entry(dora) for c in cases]), table)
        grouped = [c.w.clone() for c in cases]
        for c in cases:
            assert _margins_intact(c.buf, 7.0)
            c.w.fill_(9.0)
            ops.lora_merge(ops.lora_plan([c.entry(dora)]), table)
        for c, g in zip(cases, grouped):
            assert _same_bits(c.w, g), f"{c.what} dora={dora}: grouped and single plans differ"
            assert _margins_intact(c.buf, 7.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_scales_zero_gives_the_base_bits(gpu, dtype):
    gen = torch.Generator(device=gpu).manual_seed(7)
    zeros = torch.zeros(8, dtype=torch.float32, device=gpu)
    for spec in SHAPES[:3]:
        c = Case(spec, dtype, gpu, gen)
        c.base[::3, ::5] = -0.0
        for dora in (False, True):
            c.w.fill_(9.0)
            plan = ops.lora_plan([c.entry(dora)])
            ops.lora_merge(plan, zeros)
            assert _same_bits(c.w, c.base), f"{c.what} dora={dora}: all scales zero must give the base's bits"
            # only the LoHa adapter live: whatever the others hold, magnitudes included, plays no part
            ops.lora_merge(plan, _table(gpu, [0.0, SCALES[1], 0.0]))
            got = c.w.clone()
            ops.lora_merge(ops.lora_plan([c.entry(dora, only=[1])]), _table(gpu))
            assert _same_bits(c.w, got), f"{c.what} dora={dora}: adapters at scale 0 must be skipped whole"
            assert _margins_intact(c.buf, 7.0)


def test_bad_tables_are_refused_and_nothing_is_written(gpu):
    dtype = torch.bfloat16
    w = torch.full((64, 128), 5.0, dtype=dtype, device=gpu)
    base = torch.zeros_like(w)
    up, down_t = torch.zeros((64, 32), dtype=dtype, device=gpu), torch.zeros((128, 32), dtype=dtype, device=gpu)
    w1, w2 = torch.zeros((4, 8), device=gpu), torch.zeros((16, 16), device=gpu)
    bad = [("hada", up, down_t, up, down_t[:, :16].contiguous(), 0),           # second pair: rank no multiple of 32
           ("hada", up, down_t, up[:32], down_t, 0),                            # second pair: wrong rows
           ("hada", up, down_t, up.float(), down_t.float(), 0),                 # second pair: wrong dtype
           ("hada", up, down_t, up, 0),                                         # a pair missing
           ("kron", w1, w2[:15].contiguous(), 1, 0, 0),                         # a c != N
           ("kron", w1, w2[:, :15].contiguous(), 1, 0, 0),                      # b d != K
           ("kron", w1, w2, 3, 0, 0),                                           # taps do not divide w2's columns
           ("kron", w1, w2, 1, 2, 0),                                           # no such layout
           ("kron", w1.to(dtype), w2, 1, 0, 0),                                 # tables are fp32
           ("kron", w1, w2.t(), 1, 0, 0),                                       # not contiguous
           ("kron", w1, torch.zeros(16 * 16 + 1, device=gpu)[1:].view(16, 16), 1, 0, 0),      # not 16-byte aligned
           ("tucker", up, down_t, 0)]                                           # no such kind
    for fac in bad:
        with pytest.raises(ops.BackendError, match="lora_plan"):
            ops.lora_plan([(w, base, [fac])])
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.lora_plan([(w, base, [("kron", w1.cpu(), w2, 1, 0, 0)])])
    with pytest.raises(ops.BackendError, match="magnitude"):
        ops.lora_plan([(w, base, [("kron", w1, w2, 1, 0, 0, torch.ones(63, device=gpu))])])
    plan = ops.lora_plan([(w, base, [("kron", w1, w2, 1, 0, 7)])])
    assert plan.forms and plan.max_rank == 0
    with pytest.raises(ops.BackendError, match="at least 8 slots"):
        ops.lora_merge(plan, torch.zeros(4, dtype=torch.float32, device=gpu))
    torch.cuda.synchronize()
    assert bool(torch.all(w == 5.0)), "a refused call must not write"
    ops.lora_merge(plan, torch.ones(8, dtype=torch.float32, device=gpu))
    assert _same_bits(w, base)
