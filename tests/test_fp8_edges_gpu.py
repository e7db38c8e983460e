"""The e4m3 GEMM family (gemm_dispatch<f8, false>: st_linear_fp8, st_linear_fp8x) gated per element against float64: every tile the
dispatch offers e4m3 operands with a partial last M tile and a partial last N tile (plain, GEGLU, LayerNorm folded), fewer K tiles
than ring stages, in-launch K splits with slices of unequal length, row and per-tensor scales, the e4m3 copy of the output bit for
bit, row statistics at ragged edges, the eight-phase kernel at its smallest shapes - and the two quantiser kernels of
csrc/fp8.hip per element.  The GEMM's operands are bytes and scales made on the host (no GEMM test depends on a quantiser kernel);
they sit in poisoned memory (bytes: the e4m3 NaN, scales: NaN) and every output in a guarded buffer.  Budgets, case lists and the
restated dispatcher: tests/edge_util.py; the CPU proof that the gate bites on this family's arithmetic: tests/test_fp8_gate_host.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

from stabletriton_amd import _C, ops
from tests import edge_util as eu
from tests.test_dma_edges_gpu import _factor
from tests.test_edges_gpu import _dev, _name, _report

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EPS = 1e-5
FAMILIES = eu.FP8_FAMILIES


def _id(v):
    if isinstance(v, tuple):
        return "-".join(_name(e) or str(e) for e in v)
    return _name(v)


@functools.lru_cache(maxsize=2)
def _problem(M, K, rows, family, per_tensor=False):
    """Bytes, scales, bias and float64 products: computed once per problem, shared by the tests that launch it with different epilogues."""
    return eu.Fp8Problem(M, K, rows, family, per_tensor)


class _Operands:
    """A problem's operands on the device, each inside poisoned memory; the activation's rows apart by a gap of NaN bytes."""

    def __init__(self, p, gpu, bias=True, row_gap=eu.ROW_GAP_U8):
        self.xq, self.rs = eu.poisoned(p.xq.to(gpu), row_gap=row_gap), eu.poisoned(p.rs.to(gpu))
        self.wq, self.cs = eu.poisoned(p.wq.to(gpu)), eu.poisoned(p.cs.to(gpu))
        self.bias = _dev(p.bias, gpu, BF16) if bias else None


def _check(gpu, M, K, N, family, *, bias=True, silu=False, geglu=False, residual=False, sk=1, per_tensor=False, shape3d=None, group):
    """Launch twice into guarded outputs (equal bits, margins intact), gate every element.  Row scales: st_linear_fp8; one scale for
    the tensor: st_linear_fp8x; shape3d: ops.linear_fp8 on a 3-D activation with a 3-D residual."""
    p = _problem(M, K, 2 * N if geglu else N, family, per_tensor)
    r = p.residual(N) if residual else None
    o = _Operands(p, gpu, bias, row_gap=0 if shape3d else eu.ROW_GAP_U8)
    rg = None if r is None else _dev(r if shape3d is None else r.view(*shape3d, N), gpu, BF16, row_gap=eu.ROW_GAP)
    what = f"{family} {(M, K, N)}" + ("+bias" if bias else "") + ("+silu" if silu else "") + ("+geglu" if geglu else "") + \
           ("+residual" if residual else "") + ("(3-D)" if shape3d else "") + (" per-tensor scale" if per_tensor else "")

    def launch():
        if shape3d is not None:
            return ops.linear_fp8(ops.Fp8Rows(o.xq, o.rs, (*shape3d, K)), o.wq, o.cs, o.bias, silu=silu, geglu=geglu, residual=rg).reshape(M, N)
        out, buf = eu.guarded((M, N), BF16, gpu)
        if per_tensor:
            eu.linear_fp8x_into(out, o.xq, o.rs, o.wq, o.cs, o.bias, geglu=geglu, residual=rg)
        else:
            eu.linear_fp8_into(out, o.xq, o.rs, o.wq, o.cs, o.bias, silu=silu, geglu=geglu, residual=rg)
        eu.assert_margins_intact(buf, what)
        return out
    out, again = launch(), launch()
    assert torch.equal(out, again), "two launches of the same problem differ"
    ref, mag, extra, n_terms = eu.fp8_expect(p, bias=bias, silu=silu, geglu=geglu, residual=r, sk=sk)
    _report(f"{group}-{family}", BF16, what, eu.assert_elementwise(out, ref, mag, n_terms, BF16, what, extra))
    return out, o, p


def test_workspace_is_what_the_plan_assumed():
    assert ops.GEMM_WORKSPACE_BYTES == eu.FP8_WORKSPACE_BYTES


# ================================================================================================ tiles
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", eu.FP8_PLAIN, ids=_id)
def test_tile_edges(gpu, case, family):
    """One K tile (one MFMA step per accumulator tile, a single ring stage issued), a partial last M tile and a partial last N
    tile on every tile, a scale per row: the last M tile's rows read their own scales, the last N tile's columns theirs."""
    _check(gpu, *case[1], family, group="fp8-tiles")


@pytest.mark.parametrize("case", eu.FP8_GEGLU, ids=_id)
def test_tile_edges_geglu(gpu, case):
    """Value rows scaled by cs[n], gate rows by cs[N + n]; a partial last tile ends inside both halves."""
    _check(gpu, *case[1], "normal", geglu=True, group="fp8-geglu")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", eu.fp8_ring(), ids=_id)
def test_ring_start_up_and_wrap(gpu, case, family):
    """Two, three, four and five K tiles against rings of four (256 x 128: three) stages: odd and even trip counts of a loop that
    runs two trips an iteration."""
    _check(gpu, *case[1], family, group="fp8-ring")


@pytest.mark.parametrize("family,epi", [(f, e) for f in FAMILIES for e in ("none", "bias+silu", "bias+residual") if not (f == "exact" and "silu" in e)])
@pytest.mark.parametrize("case", eu.fp8_wide(), ids=_id)
def test_wide_tile_epilogues(gpu, case, family, epi):
    """The staged epilogue of the wide tiles with scales: bare product, SiLU, residual (on a 3-D activation through ops.linear_fp8)."""
    M, K, N = case[1]
    _check(gpu, M, K, N, family, bias=epi != "none", silu=epi == "bias+silu", residual=epi == "bias+residual",
           shape3d=_factor(M) if epi == "bias+residual" else None, group="fp8-epilogues")


# ================================================================================================ K split
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", eu.FP8_UNEVEN_SPLITS, ids=_id)
def test_uneven_k_split(gpu, case, family):
    """nk % sk != 0: the first nk_rem slices are one K tile longer; the scales meet the combined sum, not the slabs."""
    sk, _, (M, K, N) = case
    _check(gpu, M, K, N, family, residual=True, sk=sk, group="fp8-k-split")


# ================================================================================================ per-tensor scale, LayerNorm fold
def _producer(gpu, ctx, x0, site):
    """The activation as the transformer block hands it over: the bf16 tensor, its row partials and its e4m3 copy out of an
    identity GEMM, after two passes that settle the copy's delayed scale."""
    K = x0.shape[1]
    xg0, eye = _dev(x0, gpu, BF16, row_gap=eu.ROW_GAP), torch.eye(K, device=gpu, dtype=BF16)
    for _ in range(2):
        ops.linear(xg0, eye, None, emit_stats=True, emit_q8=site)
        ctx.fp8.update()
    xg, stats, act = ops.linear(xg0, eye, None, emit_stats=True, emit_q8=site)
    assert int((act.q & 0x7F).max()) < 0x7E, "the e4m3 copy saturated"
    return xg, stats, act


def _check_fold(gpu, M, K, N, geglu, group):
    rows = 2 * N if geglu else N
    x0, g, be, w, b = eu.fp8_ln_operands(M, K, rows)
    with ops.ExecContext(hints=False) as ctx:
        xg, stats, act = _producer(gpu, ctx, x0, ("t", 1))
        wq, ws, c, d = ops.fold_layer_norm_fp8(g.to(gpu, BF16), be.to(gpu, BF16), w.to(gpu, BF16), b.to(gpu, BF16))
        wqp, wsp, cp, dp = eu.poisoned(wq), eu.poisoned(ws), eu.poisoned(c), eu.poisoned(d)
        out = ops.linear_fp8x(act, wqp, wsp, None, geglu=geglu, ln=(stats, cp, dp, EPS))
        again = ops.linear_fp8x(act, wqp, wsp, None, geglu=geglu, ln=(stats, cp, dp, EPS))
        assert torch.equal(out, again), "two launches of the same problem differ"
        scale = ctx.fp8.scale[act.index].cpu()
    ref, mag, extra, n_terms = eu.fp8_ln_reference(xg.cpu(), act.q.cpu(), scale, wq.cpu(), ws.cpu(), c.cpu(), d.cpu(), EPS, geglu)
    what = f"ln fold {(M, K, N)}" + ("+geglu" if geglu else "")
    _report(group, BF16, what, eu.assert_elementwise(out, ref, mag, n_terms, BF16, what, extra))


@pytest.mark.parametrize("case", eu.fp8_ln(), ids=_id)
def test_ln_fold_per_tensor_scale(gpu, case):
    """st_linear_fp8x as the fp8 plan calls it: the activation's e4m3 copy under ONE delayed scale (a_scale_stride = 0), the
    LayerNorm folded from the producer's row partials, on every tile, plain and GEGLU, K = 256 and 1280, ragged M and N."""
    _, (M, K, N), geglu = case
    _check_fold(gpu, M, K, N, geglu, "fp8-ln-fold")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("residual", [False, True], ids=["bias", "bias+residual"])
@pytest.mark.parametrize("case", eu.fp8_per_tensor(), ids=_id)
def test_per_tensor_scale_without_fold(gpu, case, residual, family):
    _check(gpu, *case[1], family, residual=residual, per_tensor=True, group="fp8-per-tensor")


# ================================================================================================ the e4m3 copy of the output
@pytest.mark.parametrize("geglu,case", [(False, c) for c in eu.FP8_PLAIN] + [(True, c) for c in eu.FP8_GEGLU], ids=_id)
def test_e4m3_copy_out_of_the_fp8_gemm(gpu, geglu, case):
    """EPI_F_Q8 on ragged tiles: the copy is e4m3(clamp(stored bf16 * inv_scale)) bit for bit inside guard margins, the amax slots
    hold max |stored|, the bf16 output keeps the bits of the launch without the copy, and the form without y (GEGLU only) leaves
    the same bytes."""
    M, K, N = case[1]
    p = _problem(M, K, 2 * N if geglu else N, "normal")
    o = _Operands(p, gpu)
    ref = eu.fp8_expect(p, geglu=geglu)[0]
    inv = eu.poisoned(eu.fp8_delayed_scale(ref.abs().max())[1].reshape(1).to(gpu))          # margin 2: nothing saturates
    plain, _ = eu.guarded((M, N), BF16, gpu)
    eu.linear_fp8x_into(plain, o.xq, o.rs, o.wq, o.cs, o.bias, geglu=geglu)
    forms = [True, False] if geglu else [True]
    copies = []
    for want_out in forms:
        out, obuf = eu.guarded((M, N), BF16, gpu)
        q8, qbuf = eu.guarded((M, N), torch.uint8, gpu)
        amax = torch.zeros(ops.FP8_AMAX_SLOTS, dtype=torch.int32, device=gpu)
        eu.linear_fp8x_into(out if want_out else None, o.xq, o.rs, o.wq, o.cs, o.bias, geglu=geglu, q8=q8, q8_inv_scale=inv, q8_amax=amax)
        eu.assert_margins_intact(qbuf, f"e4m3 copy {case[1]}")
        eu.assert_margins_intact(obuf, f"output beside the e4m3 copy {case[1]}")
        if want_out:
            assert torch.equal(out, plain), "emitting the e4m3 copy changed the output"
        else:
            assert bool(torch.isnan(out).all()), "the launch without y stored through it"
        want = (plain.float() * inv).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(q8, want), f"{int((q8 != want).sum())} bytes of the copy differ from e4m3(stored * inv_scale)"
        assert float(amax.view(torch.float32).max()) == float(plain.float().abs().max())
        copies.append(q8)
    assert all(torch.equal(copies[0], c) for c in copies)


# ================================================================================================ statistics, guarded outputs
@pytest.mark.parametrize("case", eu.FP8_STATS, ids=_id)
def test_statistics_at_ragged_edges(gpu, case):
    """Row partials out of st_linear_fp8x against float64 sums of the STORED output, inside the fp32 summation bound
    N * 2^-24 * sum |terms| (the bound of the 16-bit gate); the output keeps the plain launch's bits."""
    M, K, N = case[1]
    p = _problem(M, K, N, "normal")
    o = _Operands(p, gpu)
    plain, _ = eu.guarded((M, N), BF16, gpu)
    eu.linear_fp8x_into(plain, o.xq, o.rs, o.wq, o.cs, o.bias)
    out, obuf = eu.guarded((M, N), BF16, gpu)
    stats, sbuf = eu.guarded((M, min(ops.STATS_MAX_CHUNKS, (N + 63) // 64), 2), torch.float32, gpu)
    chunks = eu.linear_fp8x_into(out, o.xq, o.rs, o.wq, o.cs, o.bias, row_stats=stats)
    eu.assert_margins_intact(obuf, f"output {case[1]}")
    eu.assert_margins_intact(sbuf, f"row partials {case[1]}")
    assert torch.equal(out, plain), "emitting the row partials changed the output"
    assert chunks == -(-N // int(case[0].split("x")[1])), f"{chunks} partials a row: not the tile the case is labelled with"
    s = stats.view(-1)[:M * chunks * 2].view(M, chunks, 2).double().sum(1).cpu()
    assert torch.isfinite(s).all(), "a row partial is not finite"
    od = out.double().cpu()
    bound = N * eu.U_ACC
    r1 = float(((s[:, 0] - od.sum(1)).abs() / (bound * od.abs().sum(1)).clamp_min(1e-300)).max())
    r2 = float(((s[:, 1] - (od * od).sum(1)).abs() / (bound * (od * od).sum(1)).clamp_min(1e-300)).max())
    _report("fp8-row-stats", BF16, f"{case[1]} sum", r1)
    _report("fp8-row-stats", BF16, f"{case[1]} sum of squares", r2)
    assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("case", eu.FP8_PLAIN, ids=_id)
def test_stays_inside_its_output(gpu, case):
    M, K, N = case[1]
    p = _problem(M, K, N, "normal")
    o = _Operands(p, gpu, row_gap=0)
    out, buf = eu.guarded((M, N), BF16, gpu)
    eu.linear_fp8_into(out, o.xq, o.rs, o.wq, o.cs, o.bias)
    eu.assert_margins_intact(buf, f"linear_fp8 {case[1]}")
    assert torch.isfinite(out.float()).all(), "an output element was never stored (or a poisoned read leaked)"
    assert torch.equal(out, ops.linear_fp8(ops.Fp8Rows(o.xq, o.rs, (M, K)), o.wq, o.cs, o.bias))


# ================================================================================================ eight-phase kernel
@pytest.mark.parametrize("family,case", [(f, c) for c in eu.FP8_GEMM8P for f in FAMILIES if f == "normal" or not c[2]], ids=_id)
def test_eight_phase_smallest_shapes(gpu, family, case):
    """gemm8p_kernel on e4m3 operands takes whole tiles only: its two tiles at the two-K-tile minimum and at five K tiles, plain
    (a scale per row), GEGLU, and the plan's form - LayerNorm folded, GEGLU, one scale for the tensor."""
    _, (M, K, N), geglu, ln = case
    if ln:
        _check_fold(gpu, M, K, N, geglu, "fp8-gemm8p")
    else:
        _check(gpu, M, K, N, family, geglu=geglu, group="fp8-gemm8p")


# ================================================================================================ the quantisers (csrc/fp8.hip)
# One wave a row, four rows a block, NV vectors of 8 (16 bit) / 4 (fp32) values a lane: C / VEC one under, at and one over a
# multiple of 64 (a partly filled last register column; the NV switch), the widest row (NV = 12, partly filled and full), and
# rows % 4 in {1, 2, 3}.
_QUANT_VECTORS = (63, 64, 65, 193, 767, 768)
_QUANT = [(d, (5 + i % 3, v * (4 if d == torch.float32 else 8))) for d in eu.DTYPES for i, v in enumerate(_QUANT_VECTORS)]


def _quant_input(rows, C):
    x = eu.normal(f"8.q{rows}.{C}", (rows, C)) * torch.logspace(-2, 2, rows)[:, None] + 0.3
    x[1] = 0.0                                          # an all-zero row: scale 1e-12 / 448, bytes 0
    return x


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("dtype,shape", _QUANT, ids=_id)
def test_quantize_rows_per_element(gpu, dtype, shape, strided):
    """st_quantize_fp8: scale == max(amax, 1e-12) / 448 in fp32, every byte == e4m3(fp32(x) * (1.0f / scale)); bytes and scales
    stay inside their buffers; a row stride (ldx) other than C."""
    rows, C = shape
    xg = _dev(_quant_input(rows, C), gpu, dtype, row_gap=eu.ROW_GAP if strided else 0)
    q, qbuf = eu.guarded((rows, C), torch.uint8, gpu)
    s, sbuf = eu.guarded((rows,), torch.float32, gpu)
    _C.check(_C.load().st_quantize_fp8(xg.data_ptr(), xg.stride(0), q.data_ptr(), s.data_ptr(), rows, C, _C.dtype_code(dtype), _C.stream_ptr()),
             "quantize_fp8")
    eu.assert_margins_intact(qbuf, f"quantize_fp8 {shape} bytes")
    eu.assert_margins_intact(sbuf, f"quantize_fp8 {shape} scales")
    xf = xg.float().cpu()
    scale = xf.abs().amax(1).clamp_min(1e-12) / torch.tensor(448.0)
    assert torch.equal(s.cpu(), scale), "scale != max(amax, 1e-12) / 448 in fp32"
    want = (xf * (torch.tensor(1.0) / scale)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q.cpu(), want), f"{int((q.cpu() != want).sum())} bytes differ from e4m3(x * (1 / scale))"
    assert int(q[1].max()) == 0


@pytest.mark.parametrize("dtype,shape", _QUANT, ids=_id)
def test_layer_norm_quantize_per_element(gpu, dtype, shape):
    """st_layer_norm_quantize_fp8: the dequantised value within half an e4m3 step of the float64 LayerNorm y of the values the
    kernel sees - max(2^-4 |y|, scale * 2^-10) - plus the fp32 error e of the normalisation itself, to first order:
        mean   a C-term fp32 sum and a division: (C + 1) 2^-24 mean|x|
        var    C squares of fp32 differences summed, each difference off by d_mean: (C + 3) 2^-24 var + 2 sd d_mean
        rstd   rho (d_var / 2 (var + eps) + RSQRT_ULPS 2^-24)
        y      |g| (rho (d_mean + 2^-24 |x - mu|) + |x - mu| d_rstd) + 4 * 2^-24 (|x - mu| rho |g| + |b|)      (four roundings)
    The scale is the row's max |y| / 448 within e as well."""
    rows, C = shape
    x = _quant_input(rows, C)
    g, b = eu.normal(f"8.qg{C}", (C,)) * 0.2 + 1.0, eu.normal(f"8.qb{C}", (C,)) * 0.2
    xg, gg, bg = _dev(x, gpu, dtype), _dev(g, gpu, dtype), _dev(b, gpu, dtype)
    q, qbuf = eu.guarded((rows, C), torch.uint8, gpu)
    s, sbuf = eu.guarded((rows,), torch.float32, gpu)
    _C.check(_C.load().st_layer_norm_quantize_fp8(xg.data_ptr(), gg.data_ptr(), bg.data_ptr(), q.data_ptr(), s.data_ptr(), rows, C, EPS,
                                                  _C.dtype_code(dtype), _C.stream_ptr()), "layer_norm_quantize_fp8")
    eu.assert_margins_intact(qbuf, f"layer_norm_quantize_fp8 {shape} bytes")
    eu.assert_margins_intact(sbuf, f"layer_norm_quantize_fp8 {shape} scales")
    xd, gd, bd = eu.r64(x, dtype), eu.r64(g, dtype), eu.r64(b, dtype)
    y = F.layer_norm(xd, (C,), gd, bd, EPS)
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rho, dev = (var + EPS).rsqrt(), (xd - mu).abs()
    d_mean = (C + 1) * eu.U_ACC * xd.abs().mean(1, keepdim=True)
    d_var = (C + 3) * eu.U_ACC * var + 2.0 * var.sqrt() * d_mean
    d_rstd = rho * (0.5 * d_var / (var + EPS) + eu.RSQRT_ULPS * eu.U_ACC)
    e = gd.abs() * (rho * (d_mean + eu.U_ACC * dev) + dev * d_rstd) + 4.0 * eu.U_ACC * (dev * rho * gd.abs() + bd.abs())
    scale = s.double().cpu()[:, None]
    assert bool(torch.isfinite(scale).all()) and bool((scale > 0).all())
    amax = y.abs().amax(1, keepdim=True)
    assert bool(((scale * 448.0 - amax.clamp_min(1e-12)).abs() <= e.amax(1, keepdim=True) + 2.0 ** -22 * amax).all()), "scale != max |y| / 448"
    back = q.cpu().view(torch.float8_e4m3fn).double() * scale
    assert bool(torch.isfinite(back).all())
    bound = torch.maximum(2.0 ** -4 * (y.abs() + e), scale * 2.0 ** -10) * (1.0 + 2.0 ** -20) + e
    ratio = float(((back - y).abs() / bound).max())
    _report("fp8-ln-quantize", dtype, f"{shape}", ratio)
    assert ratio <= 1.0
