"""The grouped LoRA merge kernel (st_lora_merge, ops.lora_plan / ops.lora_merge) against a float64 merge computed here.

Every element must satisfy

    |W - W64| <= 1/2 spacing_dtype(W64) + (sum r + 3) 2^-24 ( |Base| + sum_j |s_j| (|Up_j| . |Down_j|) )

- the final rounding to the storage dtype (spacing with the subnormal spacing as its floor) plus the textbook bound of an
fp32 dot product of sum r + 1 terms - with no share of elements left out.  Also: two launches give equal bits, all scales
zero gives the base's bits, memory just outside each weight is untouched, and one grouped launch over 40 mixed targets
equals 40 single-target launches bit for bit."""
import pytest
import torch

from stabletriton_amd import ops

pytestmark = pytest.mark.gpu

# (mantissa bits with the implicit one, exponent of the smallest normal)
FORMAT = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}
SHAPES = [(1280, 2048), (10240, 1280), (640, 640), (1000, 640), (72, 328), (50, 77)]
PAD = 64          # guard elements on each side of a weight


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


def _target(shape, dtype, ranks, dev, gen, pad=PAD):
    """Seeded base, garbage in the live weight, one (up, down) pair per rank; all values exactly representable in dtype."""
    n, k = shape
    base = (torch.randn(shape, generator=gen, device=dev) * 0.05).to(dtype)
    w, buf = _guarded(shape, dtype, dev, 7.0, pad)
    w.fill_(-3.0)
    facs = [((torch.randn((n, r), generator=gen, device=dev) * 0.2).to(dtype), (torch.randn((r, k), generator=gen, device=dev) * 0.2).to(dtype))
            for r in ranks]
    return w, buf, base, facs


def _entry(w, base, facs, slots, dtype):
    return (w, base, [(*_padded(u, d, dtype), s) for (u, d), s in zip(facs, slots)])


def _check_against_float64(w, base, facs, scales, dtype, what):
    w64 = base.double()
    mag = base.double().abs()
    for (u, d), s in zip(facs, scales):
        w64 = w64 + float(s) * (u.double() @ d.double())
        mag = mag + abs(float(s)) * (u.double().abs() @ d.double().abs())
    sum_r = sum(d.shape[0] for _, d in facs)
    bound = 0.5 * spacing(w64, dtype) + (sum_r + 3) * 2.0 ** -24 * mag
    err = (w.double() - w64).abs()
    worst = float((err / bound).max())
    print(f"{what}: worst |W - W64| / bound = {worst:.3f}, max abs err {float(err.max()):.3e}")
    bad = int((err > bound).sum())
    assert bad == 0, f"{what}: {bad} of {err.numel()} elements outside the bound (worst {worst:.3f} of it)"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("rank", [4, 16, 64, 128])
@pytest.mark.parametrize("adapters", [1, 3])
def test_merge_kernel_vs_float64(gpu, dtype, rank, adapters):
    gen = torch.Generator(device=gpu).manual_seed(1000 * rank + adapters)
    all_scales = [0.75, -1.5, 0.3]
    for shape in SHAPES:
        ranks = [rank] * adapters
        scales = all_scales[:adapters]
        w, buf, base, facs = _target(shape, dtype, ranks, gpu, gen)
        table = torch.zeros(8, dtype=torch.float32, device=gpu)
        slots = [5, 0, 2][:adapters]                     # slots need not be dense or ordered
        for s, v in zip(slots, scales):
            table[s] = v
        plan = ops.lora_plan([_entry(w, base, facs, slots, dtype)])
        ops.lora_merge(plan, table)
        torch.cuda.synchronize()
        what = f"{dtype} {shape} rank {rank} x {adapters}"
        assert _margins_intact(buf, 7.0), f"{what}: wrote outside the weight"
        _check_against_float64(w, base, facs, table[slots].tolist(), dtype, what)
        first = w.clone()
        w.fill_(11.0)
        ops.lora_merge(plan, table)
        assert torch.equal(w, first), f"{what}: two launches differ"
        table.zero_()
        ops.lora_merge(plan, table)
        assert _same_bits(w, base), f"{what}: all scales zero must give the base's bits"
        assert _margins_intact(buf, 7.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_zero_scales_keep_negative_zero_and_unaligned_weights_work(gpu, dtype):
    """A base holding -0.0 comes back with its sign (the bits are copied, not 0 added); a weight that is not 16-byte
    aligned (and an odd K) takes the elementwise path and meets the same bound."""
    gen = torch.Generator(device=gpu).manual_seed(5)
    for shape, pad in (((96, 256), 64), ((96, 256), 3), ((33, 45), 1)):
        w, buf, base, facs = _target(shape, dtype, [8, 20], gpu, gen, pad)
        base[::3, ::5] = -0.0
        table = torch.tensor([0.0, 0.0, 1.25, -0.5], dtype=torch.float32, device=gpu)
        plan = ops.lora_plan([_entry(w, base, facs, [0, 1], dtype)])
        ops.lora_merge(plan, table)
        assert _same_bits(w, base), f"{dtype} {shape} pad {pad}"
        plan = ops.lora_plan([_entry(w, base, facs, [2, 3], dtype)])
        ops.lora_merge(plan, table)
        assert _margins_intact(buf, 7.0, pad)
        _check_against_float64(w, base, facs, [1.25, -0.5], dtype, f"{dtype} {shape} pad {pad}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_grouped_launch_equals_single_launches(gpu, dtype):
    gen = torch.Generator(device=gpu).manual_seed(77)
    host = torch.Generator().manual_seed(77)
    shapes = [(640, 640), (1280, 320), (320, 1280), (200, 136), (64, 128), (130, 72), (17, 33), (1280, 2048)]
    rank_choices = [1, 4, 16, 33, 64, 128]
    table = torch.tensor([0.6, -1.1, 0.0, 2.0, 0.25, 0.0, 0.0, 0.0], dtype=torch.float32, device=gpu)
    cases = []
    for i in range(40):
        shape = shapes[int(torch.randint(len(shapes), (1,), generator=host))]
        n_ad = 1 + int(torch.randint(3, (1,), generator=host))
        ranks = [rank_choices[int(torch.randint(len(rank_choices), (1,), generator=host))] for _ in range(n_ad)]
        slots = torch.randperm(5, generator=host)[:n_ad].tolist()
        w, buf, base, facs = _target(shape, dtype, ranks, gpu, gen)
        cases.append((w, buf, base, facs, slots))
    entries = [_entry(w, base, facs, slots, dtype) for w, _, base, facs, slots in cases]
    ops.lora_merge(ops.lora_plan(entries), table)
    grouped = [c[0].clone() for c in cases]
    for c in cases:
        assert _margins_intact(c[1], 7.0)
        c[0].fill_(9.0)
    for e in entries:
        ops.lora_merge(ops.lora_plan([e]), table)
    for i, (c, g) in enumerate(zip(cases, grouped)):
        assert torch.equal(c[0], g), f"target {i} {tuple(g.shape)}: grouped and single launches differ"
        assert _margins_intact(c[1], 7.0)
    # and a target listed without factors is restored to its base
    w, buf, base, _ = _target((100, 200), dtype, [], gpu, gen)
    ops.lora_merge(ops.lora_plan([(w, base, [])] + entries[:2]), table)
    assert torch.equal(w, base) and _margins_intact(buf, 7.0)


def test_lora_ops_reject_bad_arguments(gpu):
    dtype = torch.bfloat16
    w = torch.zeros((64, 128), dtype=dtype, device=gpu)
    base = torch.zeros_like(w)
    up, down_t = torch.zeros((64, 32), dtype=dtype, device=gpu), torch.zeros((128, 32), dtype=dtype, device=gpu)
    table = torch.zeros(8, dtype=torch.float32, device=gpu)
    with pytest.raises(ops.BackendError, match="aliases"):
        ops.lora_plan([(w, w, [(up, down_t, 0)])])
    with pytest.raises(ops.BackendError, match="multiple of 32"):
        ops.lora_plan([(w, base, [(up[:, :16].contiguous(), down_t[:, :16].contiguous(), 0)])])
    with pytest.raises(ops.BackendError, match="down_t"):
        ops.lora_plan([(w, base, [(up, down_t.t().contiguous(), 0)])])
    with pytest.raises(ops.BackendError, match="base must match"):
        ops.lora_plan([(w, base.float(), [(up, down_t, 0)])])
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.lora_plan([(w.cpu(), base.cpu(), [])])
    plan = ops.lora_plan([(w, base, [(up, down_t, 7)])])
    with pytest.raises(ops.BackendError, match="at least 8 slots"):
        ops.lora_merge(plan, table[:4])
    with pytest.raises(ops.BackendError, match="scales"):
        ops.lora_merge(plan, table.double())
    ops.lora_merge(plan, table)
