"""The LDS-DMA GEMM (csrc/gemm_dma.h) gated per element against float64: every production tile of gemm_dispatch with a partial
last M tile and a partial last N tile (plain, GEGLU, LayerNorm-folded), fewer K tiles than ring stages, in-launch K splits with
slices of unequal length, row / column statistics at ragged edges, guarded outputs, the eight-phase kernel at its smallest
shapes - in bf16, fp16 and on split fp32 operands.  Budgets and case lists: tests/edge_util.py; the CPU proof that the gate
bites on this kernel's arithmetic: tests/test_dma_gate_host.py.  Operands sit in NaN-poisoned memory (activation rows apart by
a NaN gap), so a read outside them that reaches a result shows as NaN."""
import functools

import pytest
import torch

from stabletriton_amd import ops
from tests import edge_util as eu
from tests.test_edges_gpu import _dev, _name, _report

pytestmark = pytest.mark.gpu
DTYPES = eu.DTYPES
EPS = 1e-5


def _cases(fn):
    return [(d, c) for d in DTYPES for c in fn(d)]


def _id(v):
    if isinstance(v, tuple) and isinstance(v[0], (str, int)) and not all(isinstance(e, int) for e in v):
        return "-".join(_name(e) or str(e) for e in v)
    return _name(v)


@functools.lru_cache(maxsize=2)
def _problem(M, K, rows, dtype):
    """(x, w, bias, (x @ w.T, |x| @ |w|.T) in float64 on the rounded operands): computed once per shape and type, shared by the
    tests that launch it with different epilogues."""
    x, w, b = eu.dma_operands(M, K, rows)
    xd, wd = eu.r64(x, dtype), eu.r64(w, dtype)
    return x, w, b, (xd @ wd.T, xd.abs() @ wd.abs().T)


def _residual(M, N):
    return eu.normal(f"d.r{M}.{N}", (M, N))


def _check(gpu, dtype, M, K, N, *, bias=True, silu=False, geglu=False, residual=False, shape3d=None, group):
    """Launch twice (equal bits), gate every element."""
    rows = 2 * N if geglu else N
    x, w, b, products = _problem(M, K, rows, dtype)
    r = _residual(M, N) if residual else None
    xg = _dev(x, gpu, dtype, row_gap=eu.ROW_GAP) if shape3d is None else _dev(x.view(*shape3d, K), gpu, dtype, row_gap=eu.ROW_GAP)
    wg, bg = _dev(w, gpu, dtype), (_dev(b, gpu, dtype) if bias else None)
    rg = None if r is None else _dev(r if shape3d is None else r.view(*shape3d, N), gpu, dtype, row_gap=eu.ROW_GAP)
    out = ops.linear(xg, wg, bg, silu=silu, geglu=geglu, residual=rg)
    again = ops.linear(xg, wg, bg, silu=silu, geglu=geglu, residual=rg)
    assert torch.equal(out, again), "two launches of the same problem differ"
    ref, mag, extra = eu.linear_ref64(x, w, b if bias else None, dtype, silu=silu, geglu=geglu, residual=r,
                                      split_operands=dtype == torch.float32, products=products)
    what = f"linear {(M, K, N)}" + ("+bias" if bias else "") + ("+silu" if silu else "") + ("+geglu" if geglu else "") + \
           ("+residual" if residual else "") + ("(3-D)" if shape3d else "")
    _report(group, dtype, what, eu.assert_elementwise(out.reshape(M, N), ref, mag, K, dtype, what, extra))
    return out, (xg, wg, bg)


# ================================================================================================ tiles
@pytest.mark.parametrize("dtype,case", _cases(eu.dma_plain), ids=_id)
def test_tile_edges(gpu, dtype, case):
    """One K tile (the ring's prologue issues a single stage), partial last M and N tiles on every production tile; the BN = 80,
    160 and 320 tiles deal ten, twenty and forty DMA pieces over eight waves (the dump-address branch of issue_one)."""
    _check(gpu, dtype, *case[1], group="dma-tiles")


@pytest.mark.parametrize("dtype,case", _cases(eu.dma_geglu), ids=_id)
def test_tile_edges_geglu(gpu, dtype, case):
    """Value rows in the first half of the LDS tile, gate rows (N further down in W) in the second: a partial last tile ends
    inside both halves."""
    _check(gpu, dtype, *case[1], geglu=True, group="dma-geglu")


@pytest.mark.parametrize("dtype,case", _cases(eu.dma_ring), ids=_id)
def test_ring_start_up_and_wrap(gpu, dtype, case):
    """Two, three, four and five K tiles against rings of four (256 x 128: three, 64 x 320: three, 128 x 320: two) stages."""
    _check(gpu, dtype, *case[1], group="dma-ring")


def _factor(M):
    f = next(p for p in range(2, M) if M % p == 0)
    return f, M // f


@pytest.mark.parametrize("epi", ["none", "bias+silu", "bias+residual"])
@pytest.mark.parametrize("dtype,case", _cases(eu.dma_wide), ids=_id)
def test_wide_tile_epilogues(gpu, dtype, case, epi):
    """The staged epilogue of the wide tiles: bare product, SiLU, residual (the residual case on a 3-D activation); +bias alone is
    test_tile_edges."""
    M, K, N = case[1]
    _check(gpu, dtype, M, K, N, bias=epi != "none", silu=epi == "bias+silu", residual=epi == "bias+residual",
           shape3d=_factor(M) if epi == "bias+residual" else None, group="dma-epilogues")


# ================================================================================================ K split
@pytest.mark.parametrize("dtype,case", _cases(eu.dma_splits), ids=_id)
def test_uneven_k_split(gpu, dtype, case):
    """nk % sk != 0: the first nk_rem slices are one K tile longer.  Slabs are summed in slice order by whichever block arrives
    last, which alone runs the epilogue (bias + residual): two launches give the same bits."""
    _check(gpu, dtype, *case[2], residual=True, group="dma-k-split")


# ================================================================================================ LayerNorm fold
@pytest.mark.parametrize("dtype,case", _cases(eu.dma_ln), ids=_id)
def test_ln_fold(gpu, dtype, case):
    """ops.ln_linear on every tile, plain and GEGLU, K = 128 and 640, ragged M (the partial loads of the last tile's rows are
    clamped to row M - 1).  The activation comes with its row partials out of an identity GEMM, as in the transformer block;
    the reference takes it as that GEMM stored it."""
    tile, (M, K, N), geglu = case
    f32 = dtype == torch.float32
    x, g, be, w, b = eu.dma_ln_operands(M, K, 2 * N if geglu else N)
    xg, stats = ops.linear(_dev(x, gpu, dtype, row_gap=eu.ROW_GAP), torch.eye(K, device=gpu, dtype=dtype), None, emit_stats=True)
    wf, c, d = ops.fold_layer_norm(g.to(gpu, dtype), be.to(gpu, dtype), w.to(gpu, dtype), b.to(gpu, dtype))
    wfp, cp, dp = eu.poisoned(wf), eu.poisoned(c), eu.poisoned(d)
    out = ops.ln_linear(xg, stats, wfp, cp, dp, EPS, geglu=geglu)
    assert torch.equal(out, ops.ln_linear(xg, stats, wfp, cp, dp, EPS, geglu=geglu)), "two launches of the same problem differ"
    c_seen = ops._split_weight(wfp, want_rowsum=True)[1] if f32 else c          # (split operands: ln_linear takes c from the weight's image)
    ref, mag, extra = eu.ln_linear_ref64(xg.cpu(), wf.cpu(), c_seen.cpu(), d.cpu(), dtype, EPS, geglu=geglu, split_operands=f32)
    what = f"ln_linear {(M, K, N)}" + ("+geglu" if geglu else "")
    _report("dma-ln-fold", dtype, what, eu.assert_elementwise(out, ref, mag, K, dtype, what, extra))


# ================================================================================================ statistics
@pytest.mark.parametrize("dtype,case", _cases(eu.dma_stats), ids=_id)
def test_statistics_at_ragged_edges(gpu, dtype, case):
    """Row partials (one float2 per row and N tile) summed over the tiles against float64 sums of the STORED output, inside the
    fp32 summation bound N * 2^-24 * sum|terms|: a padding column or a poisoned read that enters a partial shows as NaN or as a
    sum that is off.  The output keeps the plain launch's bits.  Column partials need tile rows that do not straddle images;
    with a ragged M they cannot be emitted (None, plain bits) - where a launch does emit them they are held to the same bound."""
    M, K, N = case[1]
    x, w, b, _ = _problem(M, K, N, dtype)
    xg, wg, bg = _dev(x, gpu, dtype, row_gap=eu.ROW_GAP), _dev(w, gpu, dtype), _dev(b, gpu, dtype)
    plain = ops.linear(xg, wg, bg)
    out, stats = ops.linear(xg, wg, bg, emit_stats=True)
    assert torch.equal(out, plain), "emitting the row partials changed the output"
    o = out.double().cpu()
    s = stats.buf.double().sum(1).cpu()
    assert torch.isfinite(s).all(), "a row partial is not finite"
    bound = N * eu.U_ACC
    e1, b1 = (s[:, 0] - o.sum(1)).abs(), bound * o.abs().sum(1)
    e2, b2 = (s[:, 1] - (o * o).sum(1)).abs(), bound * (o * o).sum(1)
    r1, r2 = float((e1 / b1.clamp_min(1e-300)).max()), float((e2 / b2.clamp_min(1e-300)).max())
    _report("dma-row-stats", dtype, f"linear {(M, K, N)} sum", r1)
    _report("dma-row-stats", dtype, f"linear {(M, K, N)} sum of squares", r2)
    assert r1 <= 1.0 and r2 <= 1.0
    outc, cs = ops.linear(_dev(x.view(1, M, K), gpu, dtype, row_gap=eu.ROW_GAP), wg, bg, emit_colstats=True)
    assert torch.equal(outc.view(M, N), plain), "the column-partial request changed the output"
    if cs is not None:
        sc = cs.buf.double().sum(0).cpu()
        assert torch.isfinite(sc).all()
        assert bool(((sc[:, 0] - o.sum(0)).abs() <= M * eu.U_ACC * o.abs().sum(0)).all())
        assert bool(((sc[:, 1] - (o * o).sum(0)).abs() <= M * eu.U_ACC * (o * o).sum(0)).all())


# ================================================================================================ guarded outputs
@pytest.mark.parametrize("dtype,case", _cases(eu.dma_plain), ids=_id)
def test_stays_inside_its_output(gpu, dtype, case):
    M, K, N = case[1]
    x, w, b, _ = _problem(M, K, N, dtype)
    xg, wg, bg = _dev(x, gpu, dtype, row_gap=eu.ROW_GAP), _dev(w, gpu, dtype), _dev(b, gpu, dtype)
    out, buf = eu.guarded((M, N), dtype, gpu)
    eu.linear_into(out, xg, wg, bg)
    eu.assert_margins_intact(buf, f"linear {case[1]}")
    assert torch.isfinite(out.float()).all(), "an output element was never stored (or a poisoned read leaked)"
    assert torch.equal(out, ops.linear(xg, wg, bg))


# ================================================================================================ eight-phase kernel
@pytest.mark.parametrize("dtype,case", _cases(eu.gemm8p), ids=_id)
def test_eight_phase_smallest_shapes(gpu, dtype, case):
    """gemm8p takes whole tiles only: its two tiles at the two-K-tile minimum and at five K tiles."""
    _check(gpu, dtype, *case[1], group="gemm8p")
