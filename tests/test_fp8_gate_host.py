"""CPU proof that the per-element gate bites on the e4m3 GEMM family (gemm_dispatch<f8, false>: st_linear_fp8, st_linear_fp8x), as
tests/test_dma_gate_host.py proves it for the 16-bit LDS-DMA GEMM: an fp32 emulation of the kernel's arithmetic - K tiles of 128
bytes summed in order, the slabs of a K split in slice order, v *= rs * cs[n], the LayerNorm fold, bias, activation, residual, one
rounding to bf16, the e4m3 copy taken from the stored value - passes the gate at every shape tests/test_fp8_edges_gpu.py launches,
in both operand families, and every mutation a kernel bug would amount to fails it.  Every case's label (tile, K split) is held
to the restated dispatcher, edge_util.fp8_plan.  No GPU, no operator library."""
import functools

import pytest
import torch

from tests import edge_util as eu
from tests.test_dma_gate_host import EPS, _fma, _shift4_last_tile, emulate_stats
from tests.test_edge_gate_host import _truncate

BF16 = torch.bfloat16
KB = eu.FP8_KB


def _name(v):
    if isinstance(v, (tuple, list)):
        return "-".join(str(e) for e in v)
    return None


def _bm(tile):
    return int(tile.split("x")[0])


def _bn(tile):
    return int(tile.split("x")[1])


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
def _slice_sum(xv, wv, tiles, mutation, hit):
    """fp32 accumulators of one block over its K tiles, in order (the 128 k of one MFMA step are summed by the fp32 matmul)."""
    acc = torch.zeros(xv.shape[0], wv.shape[0])
    for n, t in enumerate(tiles):
        src = tiles[0] if (mutation == "stale_stage" and n == 1) else t           # the second K tile read from the first ring buffer
        # the q + 4 chunks of one K tile left out: the upper half of every lane's 32 bytes, k 64 .. 127 of the tile
        ks = slice(src * KB, src * KB + (KB // 2 if (mutation == "drop_hi_chunks" and t == hit) else KB))
        acc = acc + xv[:, ks] @ wv[:, ks].T
    return acc


def emulate(xq, rs, wq, cs, b, *, sk=1, silu=False, geglu=False, residual=None, ln=None, tile="64x64", mutation=None, copy_inv=None):
    """st_linear_fp8 / st_linear_fp8x as the kernels compute them.  rs has M entries or one; ln = (mean, rstd, c, d) per row /
    column; copy_inv: also return the e4m3 copy under that inverse scale.  Returns the stored bf16 tensor [, the copy's bytes]."""
    M, K = xq.shape
    rows = wq.shape[0]
    N = rows // 2 if geglu else rows
    bm, bno = _bm(tile), (_bn(tile) // 2 if geglu else _bn(tile))
    xv, wv = xq.view(eu.E4M3).float(), wq.view(eu.E4M3).float()
    if mutation == "drop_one_k":
        xv = xv.clone()
        xv[:, K // 2] = 0.0
    elif mutation == "drop_one_term":                  # one non-zero activation of the middle row: one term of each of its outputs
        xv = xv.clone()
        xv[M // 2, int(xv[M // 2].abs().argmax())] = 0.0
    nk = K // KB
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
        slabs.append(_slice_sum(xv, wv, tiles, mutation, nk // 2))
    if mutation == "slab_left_out":
        slabs = slabs[:-1]
    acc = slabs[0] if sk == 1 else functools.reduce(lambda a, sl: a + sl, slabs, torch.zeros_like(slabs[0]))
    rsv = rs.float().expand(M).clone()
    csv = cs.float().clone()
    if mutation == "rs_stride0":
        rsv[:] = rsv[0]
    elif mutation == "row_scale_from_neighbour":       # the last, partial M tile reads row m - 1's scale
        m0 = (M - 1) // bm * bm
        assert 1 <= m0 < M - 1
        rsv[m0:] = rs.float()[m0 - 1:M - 1]
    elif mutation == "col_scale_shift4":
        csv[:N] = _shift4_last_tile(csv[:N], N, bno)
    elif mutation == "gate_scale_from_value":          # cs[n] where cs[Ng + n] belongs
        csv[N:] = csv[:N]
    acc = acc * (rsv[:, None] * csv[None, :])
    if ln is not None:
        mean, rstd, c, d = ln
        if mutation == "rstd_from_neighbour":
            rstd = rstd.roll(1)
        elif mutation == "ln_c_shift":
            c = torch.cat([_shift4_last_tile(c[:N], N, bno), c[N:]])
        elif mutation == "ln_d_shift":
            d = torch.cat([_shift4_last_tile(d[:N], N, bno), d[N:]])
        acc = _fma(rstd[:, None], _fma(-mean[:, None], c[None, :], acc), d[None, :])
    if b is not None:
        br = b.to(BF16).float()
        if mutation == "bias_shift":
            br = torch.cat([_shift4_last_tile(br[:N], N, bno), br[N:]])
        acc = acc + br
    if geglu:
        acc = acc[:, :N] * eu.gelu64(acc[:, N:].double()).float()
    elif silu:
        acc = eu.silu64(acc.double()).float()
    if residual is not None:
        acc = acc + residual.to(BF16).float()
    out = _truncate(acc, BF16) if mutation == "truncate" else acc.to(BF16)
    if copy_inv is None:
        return out
    return out, eu.e4m3_copy(acc if mutation == "copy_unrounded" else out, copy_inv)


@functools.lru_cache(maxsize=2)
def _problem(M, K, rows, family, per_tensor=False):
    return eu.Fp8Problem(M, K, rows, family, per_tensor)


def _run(M, K, N, family, *, tile, bias=True, silu=False, geglu=False, residual=False, sk=1, per_tensor=False, mutation=None):
    """(emulated output, (ref, mag, extra, n_terms)) of a case."""
    p = _problem(M, K, 2 * N if geglu else N, family, per_tensor)
    r = p.residual(N) if residual else None
    out = emulate(p.xq, p.rs, p.wq, p.cs, p.bias if bias else None, sk=sk, silu=silu, geglu=geglu, residual=r, tile=tile, mutation=mutation)
    return out, eu.fp8_expect(p, bias=bias, silu=silu, geglu=geglu, residual=r, sk=sk)


def _gate(out, expect, what):
    ref, mag, extra, n_terms = expect
    return eu.assert_elementwise(out, ref, mag, n_terms, BF16, what, extra)


def _fails(out, expect, what):
    ref, mag, extra, n_terms = expect
    with pytest.raises(AssertionError, match="x its budget"):
        eu.assert_elementwise(out, ref, mag, n_terms, BF16, what, extra)


@functools.lru_cache(maxsize=2)
def _ln_case(M, K, N, geglu):
    """The fold's operands as the GPU test meets them: x as its producer stored it (an identity GEMM: bf16(x)), its e4m3 copy
    under the delayed scale two settling passes leave (2 max |x| / 448), the folded weight's bytes, c, d - and the reference."""
    x, g, be, w, b = eu.fp8_ln_operands(M, K, 2 * N if geglu else N)
    xs = x.to(BF16)
    scale, inv = eu.fp8_delayed_scale(xs.float().abs().max())
    q = eu.e4m3_copy(xs, inv)
    assert int((q & 0x7F).max()) < 0x7E                    # nothing saturated
    wq, ws, c, d = eu.fp8_fold(g, be, w, b)
    return xs, q, scale, wq, ws, c, d, eu.fp8_ln_reference(xs, q, scale, wq, ws, c, d, EPS, geglu)


def _run_ln(M, K, N, geglu, tile, mutation=None):
    xs, q, scale, wq, ws, c, d, expect = _ln_case(M, K, N, geglu)
    mean, rstd, _ = emulate_stats(xs.float())
    return emulate(q, scale.reshape(1), wq, ws, None, geglu=geglu, ln=(mean, rstd, c, d), tile=tile, mutation=mutation), expect


# ------------------------------------------------------------------------------------------------ labels: the dispatcher restated
def test_restated_dispatcher_reproduces_the_16_bit_labels():
    """dense_plan at 64 k a K tile gives every label the LDS-DMA gate's lists carry (those were observed on the device through
    the statistics' tile rows): the restatement fp8_plan rests on is the dispatcher's."""
    for tile, (M, K, N) in eu.DMA_PLAIN:
        assert eu.dense_plan(M, K, N, kb=64, f8=False)[::3] == (tile, 1), (tile, M, K, N)
    for tile, (M, K, N) in eu.DMA_GEGLU:
        assert eu.dense_plan(M, K, N, True, kb=64, f8=False)[::3] == (tile, 1), (tile, M, K, N)
    for sk, tile, (M, K, N) in eu.DMA_UNEVEN_SPLITS:
        assert eu.dense_plan(M, K, N, kb=64, f8=False)[::3] == (tile, sk), (tile, M, K, N)
    for tile, (M, K, N) in eu.GEMM8P:
        assert eu.dense_plan(M, K, N, kb=64, f8=False)[::3] == (tile, 1), (tile, M, K, N)


def test_every_case_carries_the_label_fp8_plan_computes():
    seen = set()
    for tile, (M, K, N) in eu.FP8_PLAIN + eu.fp8_ring() + eu.fp8_wide() + eu.fp8_per_tensor() + eu.FP8_STATS:
        assert eu.fp8_plan(M, K, N)[::3] == (tile, 1), (tile, M, K, N)
        seen.add(tile)
    for tile, (M, K, N) in eu.FP8_GEGLU:
        assert eu.fp8_plan(M, K, N, geglu=True)[::3] == (tile, 1), (tile, M, K, N)
    for sk, tile, (M, K, N) in eu.FP8_UNEVEN_SPLITS:
        assert eu.fp8_plan(M, K, N)[::3] == (tile, sk) and (K // KB) % sk != 0, (tile, M, K, N)
    for tile, (M, K, N), geglu in eu.fp8_ln():
        assert eu.fp8_plan(M, K, N, geglu=geglu, ln=True)[::3] == (tile, 1), (tile, M, K, N, geglu)
    for tile, (M, K, N), geglu, ln in eu.FP8_GEMM8P:
        assert eu.fp8_plan(M, K, N, geglu=geglu, ln=ln)[::3] == (tile, 1), (tile, M, K, N, geglu, ln)
    # every tile the e4m3 GEMM is offered (no BN = 320) is reached, every shape has a partial last M tile and a partial last N tile
    assert seen == {c[0] for c in eu.IGEMM_CANDS if not c[0].endswith("320")}
    for tile, (M, K, N) in eu.FP8_PLAIN:
        assert M % _bm(tile) and N % _bn(tile) and N % 8 == 0
    for tile, (M, K, N) in eu.FP8_GEGLU:
        assert M % _bm(tile) and N % (_bn(tile) // 2) and N % 8 == 0
    assert eu.FP8_WORKSPACE_BYTES == eu.CONV_WORKSPACE_BYTES


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("family", eu.FP8_FAMILIES)
def test_emulation_passes_at_every_gpu_shape(family):
    """Worst ratios to the budget per group (printed).  Exact family: the emulation equals the rounded reference bit for bit."""
    exact = family == "exact"
    worst = {}

    def note(group, out, expect, what):
        worst[group] = max(worst.get(group, 0.0), _gate(out, expect, what))
        if exact:
            assert torch.equal(out.double(), expect[0].to(BF16).double()), f"{what}: exact operands, unequal bits"

    for tile, (M, K, N) in eu.FP8_PLAIN + eu.fp8_ring():
        note("tiles+ring", *_run(M, K, N, family, tile=tile), f"emulated linear_fp8 {(M, K, N)}")
    for tile, (M, K, N) in eu.fp8_wide():
        for kw in ({"bias": False}, {"silu": True}, {"residual": True}):
            if not (exact and "silu" in kw):
                note("epilogues", *_run(M, K, N, family, tile=tile, **kw), f"emulated linear_fp8 {(M, K, N)} {list(kw)}")
    for sk, tile, (M, K, N) in eu.FP8_UNEVEN_SPLITS:
        note("k-split", *_run(M, K, N, family, tile=tile, residual=True, sk=sk), f"emulated split {sk} {(M, K, N)}")
    for tile, (M, K, N) in eu.fp8_per_tensor():
        for res in (False, True):
            note("per-tensor", *_run(M, K, N, family, tile=tile, residual=res, per_tensor=True), f"emulated linear_fp8x {(M, K, N)}")
    for tile, (M, K, N), geglu, ln in eu.FP8_GEMM8P:
        if not geglu:
            note("eight-phase", *_run(M, K, N, family, tile=tile), f"emulated 8p {(M, K, N)}")
    if not exact:
        for tile, (M, K, N) in eu.FP8_GEGLU:
            note("geglu", *_run(M, K, N, family, tile=tile, geglu=True), f"emulated geglu {(M, K, N)}")
        for tile, (M, K, N), geglu in eu.fp8_ln():
            note("ln-fold", *_run_ln(M, K, N, geglu, tile), f"emulated fold {(M, K, N)} geglu={geglu}")
        for tile, (M, K, N), geglu, ln in eu.FP8_GEMM8P:
            if geglu:
                out, expect = _run_ln(M, K, N, True, tile) if ln else _run(M, K, N, family, tile=tile, geglu=True)
                note("eight-phase", out, expect, f"emulated 8p {(M, K, N)} geglu ln={ln}")
    for group, r in worst.items():
        print(f"EMULATION fp8 {group} {family}: worst ratio {r:.3g}")
    assert exact or worst["tiles+ring"] > 0.5          # the gate is tight where the store's rounding leads


# ------------------------------------------------------------------------------------------------ every mutation fails
@pytest.mark.parametrize("mutation", ["drop_k_tile", "drop_one_k", "drop_hi_chunks"])
def test_dropped_k_fails_at_k_1280(mutation):
    """One K tile of ten, one k of 1280, or the upper 64 k of one K tile (the q + 4 chunks of every lane's fragment)."""
    M, K, N = 70, 1280, 200
    _gate(*_run(M, K, N, "normal", tile="64x64"), "unmutated")
    _fails(*_run(M, K, N, "normal", tile="64x64", mutation=mutation), mutation)


def test_stale_ring_stage_fails_at_two_k_tiles():
    _fails(*_run(70, 256, 200, "normal", tile="64x64", mutation="stale_stage"), "stale_stage")


@pytest.mark.parametrize("family", eu.FP8_FAMILIES)
@pytest.mark.parametrize("mutation", ["slice_short", "slab_left_out"])
@pytest.mark.parametrize("case", [0, 4, 8], ids=["sk2-5504", "sk4-2176", "sk8-4224"])
def test_k_split_mutations_fail(family, mutation, case):
    sk, tile, (M, K, N) = eu.FP8_UNEVEN_SPLITS[case]
    N = min(N, 200)
    _gate(*_run(M, K, N, family, tile=tile, residual=True, sk=sk), "unmutated")
    _fails(*_run(M, K, N, family, tile=tile, residual=True, sk=sk, mutation=mutation), mutation)


@pytest.mark.parametrize("mutation", ["row_scale_from_neighbour", "col_scale_shift4", "bias_shift", "rs_stride0"])
@pytest.mark.parametrize("tile,shape", [("64x64", (70, 128, 200)), ("128x160", (771, 128, 4648))], ids=_name)
def test_scale_and_edge_mutations_fail(mutation, tile, shape):
    """The row scale of the neighbouring row in the last M tile, the column scale (the bias) of the last N tile four columns
    off, per-row scales read with stride 0."""
    _gate(*_run(*shape, "normal", tile=tile), "unmutated")
    _fails(*_run(*shape, "normal", tile=tile, mutation=mutation), mutation)


@pytest.mark.parametrize("mutation", ["row_scale_from_neighbour", "col_scale_shift4"])
def test_scale_mutations_fail_in_the_exact_family(mutation):
    """Powers of two that cycle with periods 7 and 5: a neighbour's scale is off by a factor of two at least."""
    _fails(*_run(70, 128, 200, "exact", tile="64x64", mutation=mutation), mutation)


@pytest.mark.parametrize("tile,shape", [("64x64", (1, 128, 8)), ("64x128", (134, 128, 3088))], ids=_name)
def test_gate_half_scaled_by_the_value_half_fails(tile, shape):
    _gate(*_run(*shape, "normal", tile=tile, geglu=True), "unmutated")
    _fails(*_run(*shape, "normal", tile=tile, geglu=True, mutation="gate_scale_from_value"), "gate scale")


@pytest.mark.parametrize("mutation", ["rstd_from_neighbour", "ln_c_shift", "ln_d_shift"])
@pytest.mark.parametrize("tile,shape", [("64x64", (70, 256, 200)), ("128x80", (450, 1280, 3368))], ids=_name)
def test_ln_fold_mutations_fail(mutation, tile, shape):
    _gate(*_run_ln(*shape, False, tile), "unmutated")
    _fails(*_run_ln(*shape, False, tile, mutation=mutation), mutation)


@pytest.mark.parametrize("shape", [(70, 128, 200), (259, 128, 4128)], ids=_name)
def test_truncating_store_fails_at_k_128(shape):
    _fails(*_run(*shape, "normal", tile="64x64", mutation="truncate"), "truncate")


def test_copy_taken_from_the_unrounded_value_differs():
    """A byte comparison: the copy is e4m3 of the STORED bf16 value; taken from the fp32 value in front of the store it differs
    wherever the two roundings do not commute."""
    p = _problem(70, 128, 200, "normal")
    inv = eu.fp8_delayed_scale(eu.fp8_expect(p)[0].abs().max())[1]
    out, copy = emulate(p.xq, p.rs, p.wq, p.cs, p.bias, copy_inv=inv)
    assert torch.equal(copy, eu.e4m3_copy(out, inv))
    _, mutated = emulate(p.xq, p.rs, p.wq, p.cs, p.bias, copy_inv=inv, mutation="copy_unrounded")
    assert not torch.equal(copy, mutated)


# ------------------------------------------------------------------------------------------------ the exact family
@pytest.mark.parametrize("sk,tile,shape", [c for c in eu.FP8_UNEVEN_SPLITS if c[2][1] == 8320][:2], ids=_name)
def test_exact_family_flags_one_dropped_term_at_k_8320(sk, tile, shape):
    M, K, N = shape
    out, expect = _run(M, K, N, "exact", tile=tile, residual=True, sk=sk)
    assert torch.equal(out.double(), expect[0].to(BF16).double())
    mutated, _ = _run(M, K, N, "exact", tile=tile, residual=True, sk=sk, mutation="drop_one_term")
    assert int((mutated != out).any(1).sum()) == 1          # one row's outputs lost one term each
    _fails(mutated, expect, "one dropped term")
