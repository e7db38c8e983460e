"""CPU proof that the per-element gate bites on the LDS-DMA GEMM (csrc/gemm_dma.h), as tests/test_edge_gate_host.py proves it for
the register-staged one: an fp32 emulation of THIS kernel's arithmetic - accumulation K tile by K tile, the slabs of a K split
summed in slice order, the LayerNorm fold of gemm_args.h (two FMAs on a mean and an rstd formed in fp32 from partial sums),
the three-product image arithmetic of split fp32 operands, one rounding to the stored type - passes the gate at every shape
tests/test_dma_edges_gpu.py launches, and every mutation a kernel bug would amount to fails it.  The two budget terms this
kernel adds (tests/edge_util.py: split_term, ln_stat_bounds) are measured here.  No GPU, no operator library."""
import functools

import pytest
import torch

from tests import edge_util as eu
from tests.test_edge_gate_host import _truncate

HALF = [torch.bfloat16, torch.float16]
EPS = 1e-5


def _name(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, (tuple, list)):
        return "-".join(_name(e) or str(e) for e in v)
    return None


def _bn(tile):
    return int(tile.split("x")[1])


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
def _fma(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 values is exact in float64, the sum rounds at 53 bits and again at 24."""
    return (a.double() * b.double() + c.double()).float()


def _images(t, dtype):
    """What the matrix pipe multiplies: the value rounded to the 16-bit type, or (hi, lo) of the split fp32 image."""
    if dtype != torch.float32:
        return (t.to(dtype).float(),)
    hi = t.half().float()
    return hi, ((t - hi) * 2048.0).half().float()


def _slice_sum(xi, wi, tiles, kb, mutation):
    """fp32 accumulators of one block over its K tiles, in order (an MFMA's own 16 / 32 k are summed by the fp32 matmul)."""
    acc = torch.zeros(xi[0].shape[0], wi[0].shape[0])
    corr = torch.zeros_like(acc) if len(xi) == 2 else None
    for n, t in enumerate(tiles):
        src = tiles[0] if (mutation == "stale_stage" and n == 1) else t       # the second K tile read from the first ring buffer
        ks = slice(src * kb, (src + 1) * kb)
        acc = acc + xi[0][:, ks] @ wi[0][:, ks].T
        if corr is not None:
            corr = corr + xi[0][:, ks] @ wi[1][:, ks].T
            corr = corr + xi[1][:, ks] @ wi[0][:, ks].T
    return acc if corr is None else _fma(corr, torch.tensor(2.0 ** -11), acc)


def emulate_stats(xr, chunk=64):
    """(mean, rstd, a2 / K) as the consumer forms them: fp32 row sums per producer N tile, the tiles added in order."""
    K = xr.shape[1]
    a1, a2 = torch.zeros(xr.shape[0]), torch.zeros(xr.shape[0])
    for c0 in range(0, K, chunk):
        a1 = a1 + xr[:, c0:c0 + chunk].sum(1)
        a2 = a2 + (xr[:, c0:c0 + chunk] * xr[:, c0:c0 + chunk]).sum(1)
    mean = a1 / K
    q = a2 / K
    rstd = torch.rsqrt((q - mean * mean).clamp_min(0.0) + EPS)
    return mean, rstd, q


def _shift4_last_tile(v, N, bno):
    """The entries of the last (partial) N tile taken four columns to the left."""
    n0 = (N - 1) // bno * bno
    assert n0 >= 4
    v = v.clone()
    v[n0:N] = v[n0 - 4:N - 4].clone()
    return v


def emulate(x, w, b, dtype, *, sk=1, silu=False, geglu=False, residual=None, ln=None, bn=64, mutation=None):
    """ops.linear / ops.ln_linear (ln = (c, d)) as gemm_dma_kernel computes them; x is what the kernel reads (for the fold: what
    its producer stored)."""
    kb = 32 if dtype == torch.float32 else 64
    M, K = x.shape
    assert K % kb == 0
    rows = w.shape[0]
    N = rows // 2 if geglu else rows
    xr = x.to(dtype).float()
    xsrc = x
    if mutation == "drop_one_k":
        xsrc = x.clone()
        xsrc[:, K // 2] = 0.0
    elif mutation == "last_row_from_neighbour":
        xsrc = x.clone()
        xsrc[M - 1] = x[M - 2]
    xi, wi = _images(xsrc, dtype), _images(w, dtype)
    nk = K // kb
    base, rem = divmod(nk, sk)
    slabs, lo = [], 0
    for s in range(sk):
        n = base + (1 if s < rem else 0)
        tiles = list(range(lo, lo + n))
        lo += n
        if mutation == "slice_short" and s == 0:
            tiles = tiles[:-1]
        if mutation == "drop_k_tile" and s == 0:
            del tiles[len(tiles) // 2]
        slabs.append(_slice_sum(xi, wi, tiles, kb, mutation))
    if mutation == "slab_left_out":
        slabs = slabs[:-1]
    acc = slabs[0] if sk == 1 else functools.reduce(lambda a, sl: a + sl, slabs, torch.zeros_like(slabs[0]))
    bno = bn // 2 if geglu else bn
    if ln is not None:
        c, d = ln
        mean, rstd, _ = emulate_stats(xr)
        if mutation == "mean_64ulp":
            mean = mean + 64.0 * 2.0 ** -23 * mean.abs()
        elif mutation == "rstd_from_neighbour":
            rstd = rstd.roll(1)
        elif mutation == "ln_c_shift":
            c = _shift4_last_tile(c, N, bno)
        elif mutation == "ln_d_shift":
            d = _shift4_last_tile(d, N, bno)
        acc = _fma(rstd[:, None], _fma(-mean[:, None], c[None, :], acc), d[None, :])
    if b is not None:
        br = b.to(dtype).float()
        if mutation == "bias_shift":
            br = _shift4_last_tile(br, N, bno)
        acc = acc + br
    if geglu:
        g0 = N - 8 if mutation == "gate_rows_minus8" else N
        acc = acc[:, :N] * eu.gelu64(acc[:, g0:g0 + N].double()).float()
    elif silu:
        acc = eu.silu64(acc.double()).float()
    if residual is not None:
        acc = acc + residual.to(dtype).float()
    return _truncate(acc, dtype) if mutation == "truncate" else acc.to(dtype)


def _ln_case(M, K, N, dtype, geglu):
    """(x as its producer stored it, folded weight, c, d) - the fold as ops.fold_layer_norm has it (split operands: c of the image)."""
    x, g, be, w, b = eu.dma_ln_operands(M, K, 2 * N if geglu else N)
    xs = x.to(dtype).float()
    wd = w.to(dtype)
    wf = (wd.float() * g.to(dtype).float()[None, :]).to(dtype)
    if dtype == torch.float32:
        hi, lo = _images(wf, dtype)
        c = (hi.double().sum(1) + lo.double().sum(1) / 2048.0).float()
    else:
        c = wf.float().sum(1)
    d = wd.float() @ be.to(dtype).float() + b.to(dtype).float()
    return xs, wf.float(), c, d


def _gate(out, ref, mag, extra, K, dtype, what):
    return eu.assert_elementwise(out, ref, mag, K, dtype, what, extra)


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_emulation_passes_at_every_gpu_shape(dtype):
    """Worst ratios to the budget, per group (printed): 16-bit types use 0.9 and more of it at every group (the store's own
    rounding somewhere among thousands of elements); fp32 stays low because rounding errors of both signs add like sqrt(K)
    where the budget takes their worst case K."""
    f32 = dtype == torch.float32
    worst = {}

    def note(group, r):
        worst[group] = max(worst.get(group, 0.0), r)

    for tile, (M, K, N) in eu.dma_plain(dtype) + eu.dma_ring(dtype) + [c for c in eu.dma_stats(dtype) if c not in eu.dma_plain(dtype)]:
        x, w, b = eu.dma_operands(M, K, N)
        ref, mag, ex = eu.linear_ref64(x, w, b, dtype, split_operands=f32)
        note("plain+ring", _gate(emulate(x, w, b, dtype, bn=_bn(tile)), ref, mag, ex, K, dtype, f"emulated linear {(M, K, N)}"))
    for tile, (M, K, N) in eu.dma_geglu(dtype):
        x, w, b = eu.dma_operands(M, K, 2 * N)
        ref, mag, ex = eu.linear_ref64(x, w, b, dtype, geglu=True, split_operands=f32)
        note("geglu", _gate(emulate(x, w, b, dtype, geglu=True, bn=_bn(tile)), ref, mag, ex, K, dtype, f"emulated geglu {(M, K, N)}"))
    for tile, (M, K, N) in eu.dma_wide(dtype):
        x, w, b = eu.dma_operands(M, K, N)
        r = eu.normal(f"d.r{M}.{N}", (M, N))
        for bias, kw in ((None, {}), (b, {"silu": True}), (b, {"residual": r})):
            ref, mag, ex = eu.linear_ref64(x, w, bias, dtype, split_operands=f32, **kw)
            note("epilogues", _gate(emulate(x, w, bias, dtype, bn=_bn(tile), **kw), ref, mag, ex, K, dtype, f"emulated {(M, K, N)} {list(kw)}"))
    for sk, tile, (M, K, N) in eu.dma_splits(dtype):
        x, w, b = eu.dma_operands(M, K, N)
        r = eu.normal(f"d.r{M}.{N}", (M, N))
        assert (K // (32 if f32 else 64)) % sk != 0
        ref, mag, ex = eu.linear_ref64(x, w, b, dtype, residual=r, split_operands=f32)
        note("k-split", _gate(emulate(x, w, b, dtype, sk=sk, residual=r), ref, mag, ex, K, dtype, f"emulated split {sk} {(M, K, N)}"))
    for tile, (M, K, N), geglu in eu.dma_ln(dtype):
        xs, wf, c, d = _ln_case(M, K, N, dtype, geglu)
        ref, mag, ex = eu.ln_linear_ref64(xs, wf, c, d, dtype, EPS, geglu=geglu, split_operands=f32)
        note("ln-fold", _gate(emulate(xs, wf, None, dtype, geglu=geglu, ln=(c, d), bn=_bn(tile)), ref, mag, ex, K, dtype,
                              f"emulated ln_linear {(M, K, N)} geglu={geglu}"))
    for tile, (M, K, N) in eu.gemm8p(dtype):
        x, w, b = eu.dma_operands(M, K, N)
        ref, mag, ex = eu.linear_ref64(x, w, b, dtype, split_operands=f32)
        note("eight-phase", _gate(emulate(x, w, b, dtype), ref, mag, ex, K, dtype, f"emulated 8p {(M, K, N)}"))
    for group, r in worst.items():
        print(f"EMULATION {group} {_name(dtype)}: worst ratio {r:.3g}")
    assert f32 or worst["plain+ring"] > 0.5            # the gate is tight where the store's rounding leads: the emulation uses most of it


def test_emulated_row_statistics():
    """The fold's two measured constants.  Over every LayerNorm-fold shape and type: |mean - mu| in units of U_ACC * mean|x|,
    |a2 / K - q| and the rest of the variance's error in units of U_ACC * q.  edge_util's constants cover what is measured and
    are at most twice it."""
    mean_units = var_units = rstd_ratio = 0.0
    for dtype in eu.DTYPES:
        for tile, (M, K, N), geglu in eu.dma_ln(dtype):
            if geglu:
                continue
            xs = _ln_case(M, K, 8, dtype, False)[0]
            mean, rstd, q = emulate_stats(xs)
            x64 = xs.double()
            mu, rho, d_mean, d_rstd = eu.ln_stat_bounds(x64, EPS)
            m1, q64 = x64.abs().mean(1), (x64 * x64).mean(1)
            e_mean = (mean.double() - mu).abs()
            mean_units = max(mean_units, float((e_mean / (eu.U_ACC * m1)).max()))
            var = (q - mean * mean).double()
            e_var = ((var - (q64 - mu * mu)).abs() - 2.0 * mu.abs() * e_mean).clamp_min(0.0)
            var_units = max(var_units, float((e_var / (eu.U_ACC * q64)).max()))
            assert bool((e_mean <= d_mean).all())
            rstd_ratio = max(rstd_ratio, float(((rstd.double() - rho).abs() / d_rstd).max()))
    print(f"EMULATION row statistics: mean off by {mean_units:.2f} U_ACC mean|x| at most, variance by {var_units:.2f} U_ACC q "
          f"beyond the mean's share; rstd uses {rstd_ratio:.3f} of its bound")
    assert mean_units <= eu.LN_MEAN_ULPS <= 2.0 * mean_units
    assert var_units <= eu.LN_VAR_ULPS <= 2.0 * var_units
    assert rstd_ratio <= 1.0


# ------------------------------------------------------------------------------------------------ every mutation fails
def _fails(out, ref, mag, ex, K, dtype, what):
    with pytest.raises(AssertionError, match="x its budget"):
        eu.assert_elementwise(out, ref, mag, K, dtype, what, ex)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["drop_k_tile", "drop_one_k"])
def test_dropped_k_fails_at_k_1280(dtype, mutation):
    """One K tile of twenty (forty in fp32), or one k of 1280 - 0.7 % of max |ref|, which the suite's max-error check passes in bf16."""
    M, K, N = 70, 1280, 200
    x, w, b = eu.dma_operands(M, K, N)
    ref, mag, ex = eu.linear_ref64(x, w, b, dtype, split_operands=dtype == torch.float32)
    _gate(emulate(x, w, b, dtype), ref, mag, ex, K, dtype, "unmutated")
    _fails(emulate(x, w, b, dtype, mutation=mutation), ref, mag, ex, K, dtype, mutation)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["slice_short", "slab_left_out"])
@pytest.mark.parametrize("case", [0, 4, 8], ids=["sk-first", "sk-1088", "sk-2112"])
def test_k_split_mutations_fail(dtype, mutation, case):
    """A slice of an uneven split one K tile short (the `split < nk_rem` term lost), the last slab left out of the combine."""
    sk, tile, (M, K, N) = eu.dma_splits(dtype)[case]
    N = min(N, 200)
    x, w, b = eu.dma_operands(M, K, N)
    ref, mag, ex = eu.linear_ref64(x, w, b, dtype, split_operands=dtype == torch.float32)
    _gate(emulate(x, w, b, dtype, sk=sk), ref, mag, ex, K, dtype, "unmutated")
    _fails(emulate(x, w, b, dtype, sk=sk, mutation=mutation), ref, mag, ex, K, dtype, mutation)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_stale_ring_stage_fails_at_two_k_tiles(dtype):
    K = 64 if dtype == torch.float32 else 128
    M, N = 70, 200
    x, w, b = eu.dma_operands(M, K, N)
    ref, mag, ex = eu.linear_ref64(x, w, b, dtype, split_operands=dtype == torch.float32)
    _fails(emulate(x, w, b, dtype, mutation="stale_stage"), ref, mag, ex, K, dtype, "stale_stage")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["last_row_from_neighbour", "bias_shift"])
@pytest.mark.parametrize("tile,shape", [("64x64", (70, 64, 200)), ("128x160", (771, 64, 4648))], ids=_name)
def test_ragged_edge_mutations_fail(dtype, mutation, tile, shape):
    """Row M - 1 of a ragged M tile computed from row M - 2; the bias of the last, partial N tile four columns off."""
    M, K, N = shape
    x, w, b = eu.dma_operands(M, K, N)
    ref, mag, ex = eu.linear_ref64(x, w, b, dtype, split_operands=dtype == torch.float32)
    _fails(emulate(x, w, b, dtype, bn=_bn(tile), mutation=mutation), ref, mag, ex, K, dtype, mutation)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [(100, 64, 40), (134, 64, 3088)], ids=_name)
def test_geglu_gate_row_mutation_fails(dtype, shape):
    """Gate rows from n + N - 8 instead of n + N."""
    M, K, N = shape
    x, w, b = eu.dma_operands(M, K, 2 * N)
    ref, mag, ex = eu.linear_ref64(x, w, b, dtype, geglu=True, split_operands=dtype == torch.float32)
    _fails(emulate(x, w, b, dtype, geglu=True, mutation="gate_rows_minus8"), ref, mag, ex, K, dtype, "gate rows")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["rstd_from_neighbour", "ln_c_shift", "ln_d_shift"])
@pytest.mark.parametrize("tile,shape", [("64x64", (70, 128, 200)), ("128x80", (450, 640, 3368))], ids=_name)
def test_ln_fold_mutations_fail(dtype, mutation, tile, shape):
    """rstd of the row above; ln_c or ln_d of the last, partial N tile four columns off."""
    M, K, N = shape
    xs, wf, c, d = _ln_case(M, K, N, dtype, False)
    ref, mag, ex = eu.ln_linear_ref64(xs, wf, c, d, dtype, EPS, split_operands=dtype == torch.float32)
    _gate(emulate(xs, wf, None, dtype, ln=(c, d), bn=_bn(tile)), ref, mag, ex, K, dtype, "unmutated")
    _fails(emulate(xs, wf, None, dtype, ln=(c, d), bn=_bn(tile), mutation=mutation), ref, mag, ex, K, dtype, mutation)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("K", eu.DMA_LN_K)
def test_mean_off_by_64_ulp_fails_the_statistics_bound(dtype, K):
    """A mean 64 fp32 ulp (2^-17 of itself) off.  In an OUTPUT it moves rho |mu c| by 2^-17, and no per-element gate with the
    accumulation term 2 (K + 8) 2^-24 mag can see that from K = 56 on: mag holds rho |mu c| itself, and 2 * 64 * 2^-24 = 2^-17.
    (At K = 128 the mutated emulation passes the output gate: asserted below, so that nobody reads more into the gate.)  What
    catches it is the bound on the statistic, d_mean of ln_stat_bounds - the term the output budget is built from."""
    xs, wf, c, d = _ln_case(70, K, 200, dtype, False)
    mean, rstd, _ = emulate_stats(xs)
    mu, rho, d_mean, d_rstd = eu.ln_stat_bounds(xs.double(), EPS)
    assert bool(((mean.double() - mu).abs() <= d_mean).all())
    mutated = mean + 64.0 * 2.0 ** -23 * mean.abs()
    assert bool(((mutated.double() - mu).abs() > d_mean).any())
    ref, mag, ex = eu.ln_linear_ref64(xs, wf, c, d, dtype, EPS, split_operands=dtype == torch.float32)
    _gate(emulate(xs, wf, None, dtype, ln=(c, d), mutation="mean_64ulp"), ref, mag, ex, K, dtype, "mean 64 ulp off (masked in the output)")


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("shape", [(70, 64, 200), (259, 128, 4128)], ids=_name)
def test_truncating_store_fails_at_short_k(dtype, shape):
    """As in tests/test_edge_gate_host.py: visible while 2 (K + 8) 2^-24 mag stays under U_OUT |ref|, K <= 136."""
    M, K, N = shape
    x, w, b = eu.dma_operands(M, K, N)
    ref, mag, ex = eu.linear_ref64(x, w, b, dtype)
    _fails(emulate(x, w, b, dtype, mutation="truncate"), ref, mag, ex, K, dtype, "truncate")
