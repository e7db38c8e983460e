"""The conv family gated per element against float64: every instantiation of the halo conv (csrc/conv_halo.h) at two channel
slices, with an image row above and below a tile, ragged channel tiles and both upsampling forms, its K split over channel
slices (even, uneven, more than eight slices); the implicit-GEMM conv (csrc/gemm_dma.h, CONV = true) on every tile a conv can
reach, at the geometries of the UNet's odd levels (W = 12, 24, stride 2, pad 0, upsampling, tiles that straddle two images) and
with K splits whose slices begin inside a filter tap; the two-source 1x1 conv; the plain-fp32 path - in bf16, fp16 and fp32
(split operands), on two operand families: normal operands inside the derived budget, exact-sum operands inside the store
rounding alone (fp32: equality), which shows a single wrong term at any K.  Case lists, labels and budgets: tests/edge_util.py;
the CPU proof that the gate bites on both loops' arithmetic: tests/test_conv_gate_host.py.  Operands sit in NaN-poisoned
channels_last memory, so a read outside them that reaches a result shows as NaN.

Worst ratio to the budget per group, CPU emulation / MI355X (bf16, fp16, fp32) - the pass mark is the gate itself, ratio <= 1:
    normal operands   halo            0.877 / 0.877   0.494 / 0.494   0.001 / 0.001
                      halo K split    0.704 / 0.704   0.289 / 0.289   0.000 / 0.000
                      igemm tiles     0.992 / 0.992   0.970 / 0.970   0.059 / 0.040
                      igemm geometry  0.951 / 0.951   0.884 / 0.884   0.013 / 0.009
                      igemm K split   0.854 / 0.854   0.458 / 0.458   0.001 / 0.001
                      conv2d_cat      0.977 / 0.977   0.892 / 0.892   0.011 / 0.009
                      plain fp32                                      0.002 / 0.006
                      column partials 0.018 / 0.054   0.024 / 0.061   0.020 / 0.042
    exact operands    every group: the same three digits on both sides (0.996 / 0.998 at most in bf16 / fp16 where a spot makes
                      the store round, 0 elsewhere); fp32 and every column partial: 0, i.e. equality.
Where the two sides differ: in fp32 the emulation sums the 32 k of a K tile in one fp32 matmul and the split images' cross
products per K tile, the MFMAs in four-k steps in their own order (all far inside the accumulation term); the column partials
are added per thread over a strided set of the tile's rows and then over the row slots, the emulation adds 16 rows at a time.
A kernel trace of this file shows every labelled instantiation: conv_halo_kernel<T, WL2, TH, BN, 4, 2, UPS> as <4,16,128>,
<5,8,128>, <6,4,128>, <7,1,128>, <7,1,160>, <6,4,160,ups>, <7,2,160,ups> in bf16 and fp16, <5,8,64>, <5,8,128>, <6,4,64>,
<6,4,128>, <7,1,64>, <6,4,64,ups>, <6,4,128,ups>, <7,2,64,ups> on split fp32; gemm_dma_kernel<T, BM, BN, ..., CONV = true> as
64x64, 64x128, 128x64, 128x80, 128x128, 128x160 in all three, 256x128, 128x320, 64x320 in bf16 and fp16, <float, 64, 64> for the
plain-fp32 path; and the grid of every split case is tiles x sk of its label (halo: 2x2, 2x3, 2x2 / 4x2 as split fp32, 2x3, 1x9;
implicit GEMM: 108x2, 1x3, 1x4, 1x6, 1x8, 18x8, 36x6, 54x4, 54x4, 25x4, the geometry cases 6x4, 18x4, 2x4, 4x4; cat: 2x3, 4x4)."""
import functools

import pytest
import torch

from stabletriton_amd import ops
from tests import edge_util as eu
from tests.test_edges_gpu import _dev, _name, _report

pytestmark = pytest.mark.gpu
DTYPES = eu.DTYPES
F32 = torch.float32


def _cases(group):
    return [(d, lab, cfg) for d in DTYPES for lab, cfg in eu.conv_cases(d, group)]


def _id(v):
    return _name(v) if not isinstance(v, str) else v.replace("<", "_").replace(">", "").replace(",", ".").replace("/", "-")


@functools.lru_cache(maxsize=4)
def _problem(cfg, dtype, family, sk, plain=False):
    """Operands and the float64 products of a case, type and family: computed once, shared by the tests that launch it."""
    return eu.ConvCase(cfg, dtype, family, sk=sk, split_operands=False if plain else None)


def _check(gpu, dtype, label, cfg, group, c0=None, plain=False):
    """Both operand families; plain (+bias) and with row bias + residual (conv2d_cat: residual); a K split twice, equal bits."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    sk = eu.label_sk(label)
    for family in eu.CONV_FAMILIES:
        case = _problem(cfg, dtype, family, sk, plain)
        xg, wg, bg = _dev(case.x, gpu, dtype, cl=True), _dev(case.w, gpu, dtype, cl=not plain), _dev(case.b, gpu, dtype)
        rbg, rg = _dev(case.rb, gpu, dtype), _dev(case.res, gpu, dtype, cl=True)
        if c0 is not None:
            x0, x1 = _dev(case.x[:, :c0], gpu, dtype, cl=True), _dev(case.x[:, c0:], gpu, dtype, cl=True)
        for epi in (("bias", "res") if c0 is not None else ("bias", "full")):
            if c0 is not None:
                run = lambda: ops.conv2d_cat(x0, x1, wg, bg, residual=rg if epi == "res" else None)
            else:
                run = lambda: ops.conv2d(xg, wg, bg, stride, pad, upsample2x=ups, rowbias=rbg if epi == "full" else None,
                                         residual=rg if epi == "full" else None)
            out = run()
            what = f"conv {cfg} {label} {family} {epi}"
            assert out.is_contiguous(memory_format=torch.channels_last)
            if sk > 1:
                assert torch.equal(out, run()), f"{what}: two launches of the same K split differ"
            if c0 is not None:
                same = ops.conv2d(torch.cat([x0, x1], 1), wg, bg, 1, 0, residual=rg if epi == "res" else None)
                assert torch.equal(out, same), f"{what}: conv2d_cat and conv2d(torch.cat(...)) differ"
            _report(f"conv-{group}-{family}", dtype, what, case.gate(out, epi, what))


def test_workspace_is_the_one_the_labels_assume():
    assert ops.GEMM_WORKSPACE_BYTES == eu.CONV_WORKSPACE_BYTES


# ================================================================================================ halo conv
@pytest.mark.parametrize("dtype,label,cfg", _cases("halo"), ids=_id)
def test_halo_conv(gpu, dtype, label, cfg):
    """Two channel slices (the second patch lands in the other buffer while the first is read; the weight tiles issued at taps
    7 and 8 belong to the next slice), tiles with real image rows above and below, a whole image per tile beside another image,
    H = 2 and 3 at 128-pixel rows, ragged last channel tiles, 160-channel tiles (twenty weight pieces over eight waves)."""
    _check(gpu, dtype, label, cfg, "halo")


@pytest.mark.parametrize("dtype,label,cfg", _cases("halo-k-split"), ids=_id)
def test_halo_conv_k_split(gpu, dtype, label, cfg):
    """Channel slices dealt to 2, 3 and 9 blocks a tile, evenly and with the first slices one longer; slabs summed in slice order
    by the last block to arrive."""
    _check(gpu, dtype, label, cfg, "halo-k-split")


# ================================================================================================ implicit GEMM
@pytest.mark.parametrize("dtype,label,cfg", _cases("igemm-tiles"), ids=_id)
def test_implicit_gemm_tiles(gpu, dtype, label, cfg):
    """Every tile of the candidate list as a 1x1 conv with a partial last M tile and a partial last N tile."""
    _check(gpu, dtype, label, cfg, "igemm-tiles")


@pytest.mark.parametrize("dtype,label,cfg", _cases("igemm-geometry"), ids=_id)
def test_implicit_gemm_geometry(gpu, dtype, label, cfg):
    _check(gpu, dtype, label, cfg, "igemm-geometry")


@pytest.mark.parametrize("dtype,label,cfg", _cases("igemm-k-split"), ids=_id)
def test_implicit_gemm_k_split(gpu, dtype, label, cfg):
    """Slices of unequal length that begin inside a filter tap (k0 / Cin, the running (tap, channel) position)."""
    _check(gpu, dtype, label, cfg, "igemm-k-split")


@pytest.mark.parametrize("dtype,label,cfg,c0", [(d,) + c for d in DTYPES for c in eu.conv_cat_cases(d)], ids=_id)
def test_conv2d_cat(gpu, dtype, label, cfg, c0):
    """Two sources of unequal width; the boundary between them inside a K slice.  Bit-equal to the conv of the concatenation."""
    _check(gpu, dtype, label, cfg, "cat", c0=c0)


@pytest.mark.parametrize("label,cfg", eu.CONV_PLAIN_F32, ids=_id)
def test_plain_fp32_conv(gpu, label, cfg):
    """fp32 with a weight that is not channels_last: no split image, the exact fp32 MFMA on 64 x 64 tiles."""
    _check(gpu, F32, label, cfg, "plain-fp32", plain=True)


# ================================================================================================ column partials
_ALL = [(d, lab, cfg) for g in eu.CONV_GROUPS for (d, lab, cfg) in _cases(g)]


@pytest.mark.parametrize("dtype,label,cfg", _ALL, ids=_id)
def test_column_partials(gpu, dtype, label, cfg):
    """emit_colstats: (sum, sum of squares) per tile row and channel against float64 sums of the stored output, inside
    2 (BM + 8) 2^-24 of the sums of magnitudes (exact operands: equal); ColStats.rows is the BM of the label - the piece of the
    dispatch a test can see.  Tiles whose rows would straddle images emit nothing; the output keeps the plain launch's bits."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    Ho, Wo, M, _ = eu.conv_geometry(cfg)
    bm = eu.label_bm(label)
    for family in eu.CONV_FAMILIES:
        x, w, b, rb, res = eu.conv_operands(cfg, family, dtype)
        xg, wg, bg = _dev(x, gpu, dtype, cl=True), _dev(w, gpu, dtype, cl=True), _dev(b, gpu, dtype)
        for epi in ("bias", "full"):
            kw = dict(upsample2x=ups, rowbias=_dev(rb, gpu, dtype) if epi == "full" else None,
                      residual=_dev(res, gpu, dtype, cl=True) if epi == "full" else None)
            plain = ops.conv2d(xg, wg, bg, stride, pad, **kw)
            out, stats = ops.conv2d(xg, wg, bg, stride, pad, emit_colstats=True, **kw)
            what = f"conv {cfg} {label} {family} {epi}"
            assert torch.equal(out, plain), f"{what}: the column-partial request changed the output"
            if (Ho * Wo) % bm != 0:
                assert stats is None, f"{what}: column partials over tile rows that straddle images"
                continue
            assert stats is not None and stats.channels == Cout, f"{what}: no column partials"
            r1, r2 = eu.colstats_ratios(stats.buf, stats.rows, out, bm, family == "exact", what)
            _report(f"conv-column-partials-{family}", dtype, what + " sum", r1)
            _report(f"conv-column-partials-{family}", dtype, what + " sum of squares", r2)


# ================================================================================================ guarded outputs
_GUARDED = [("halo", "halo<5,8,128>/sk1"), ("halo", "halo<5,8,64>/sk1"), ("halo-k-split", "halo<5,8,128>/sk2"), ("igemm-tiles", "igemm<128x64>/sk1")]


@pytest.mark.parametrize("dtype,label,cfg", [(d, lab, cfg) for g, want in _GUARDED for (d, lab, cfg) in _cases(g) if lab == want], ids=_id)
def test_conv_stays_inside_its_output(gpu, dtype, label, cfg):
    """A halo case with a ragged channel tile, a split halo case, an implicit-GEMM case with ragged M and ragged N: the output
    sits between guard margins."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    Ho, Wo, _, _ = eu.conv_geometry(cfg)
    x, w, b, rb, res = eu.conv_operands(cfg, "normal", dtype)
    xg, wg, bg = _dev(x, gpu, dtype, cl=True), _dev(w, gpu, dtype, cl=True), _dev(b, gpu, dtype)
    out, buf = eu.guarded((N, Cout, Ho, Wo), dtype, gpu, channels_last=True)
    eu.conv2d_into(out, xg, wg, bg, stride, pad, upsample2x=ups)
    eu.assert_margins_intact(buf, f"conv {cfg} {label}")
    assert torch.isfinite(out.float()).all(), "an output element was never stored (or a poisoned read leaked)"
    assert torch.equal(out, ops.conv2d(xg, wg, bg, stride, pad, upsample2x=ups))
