"""csrc/tome.hip against tome.py's plain-torch statement in float64 on tests/tome_util.py's sites: the discrete results exact, node_max
within 1e-4 (fp32 sums of C <= 1280 terms: about C * 2^-24), the rest per element against edge_util's budgets.  Merge budget: the mean's
fp32 error is a sum of C terms of size mean|x|: n_terms = C + members on ((|x| + mean|x|) * rstd * |gamma| + |beta|), the members' mean."""
import pytest
import torch

from stabletriton_amd import tome
from tests import edge_util as eu
from tests import tome_util as TU

pytestmark = pytest.mark.gpu
SITES = [((8, 8), 64), ((16, 24), 640), ((32, 32), 1280)]      # D = 16 / 96 (no tile multiple, non-square) / 256


@pytest.mark.parametrize("rand_off", [True, False], ids=["rand", "zero"])
@pytest.mark.parametrize("ratio", [0.5, 0.3, 0.75])
@pytest.mark.parametrize("grid,C", SITES, ids=[f"{g[0]}x{g[1]}x{c}" for g, c in SITES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_launches_against_float64(gpu, dtype, grid, C, ratio, rand_off):
    x_cpu, off_cpu = TU.site(grid, C, dtype, rand_off)
    nm64, ni64 = TU.match64(grid, C, dtype, rand_off)
    x, off = x_cpu.to(gpu), off_cpu.to(gpu)
    B, N, _ = x.shape
    S, r = N // 4 * 3, tome.merged_count(N, ratio)
    what = f"{dtype} {grid} C={C} ratio={ratio} r={r}"
    (node_max, node_idx), bufs = TU.match_into(x, grid, off)
    assert torch.equal(node_idx.cpu().long(), ni64), f"{what}: node_idx"
    err = float((node_max.cpu().double() - nm64).abs().max())
    assert err <= 1e-4, f"{what}: node_max max abs err {err:.2e}"
    where64, assign64, kept64 = tome.select_reference(nm64, ni64, grid, r, off_cpu[0])
    (where, assign, kept), sbufs = TU.select_into(node_max, node_idx, grid, r, off)
    assert torch.equal(where.cpu().long(), where64) and torch.equal(assign.cpu().long(), assign64), f"{what}: where / assign"
    assert torch.equal(kept.cpu().long()[:, :S - r], kept64) and bool((kept[:, S - r:] == -7).all()), f"{what}: kept"
    gamma, beta = (t.to(gpu) for t in TU.norm_affine(C, dtype))
    y, ybuf = TU.merge_into(x, gamma, beta, 1e-5, grid, r, assign, kept, off)
    x64, g64, b64 = x_cpu.double(), gamma.cpu().double(), beta.cpu().double()
    ref = tome.merge_reference(x64, g64, b64, 1e-5, grid, r, assign64, kept64, off_cpu[0])
    rstd = (x64.var(dim=-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    mag_tok = (x64.abs() + x64.abs().mean(dim=-1, keepdim=True)) * rstd * g64.abs() + b64.abs()      # per token; then the members' mean:
    mag = tome.merge_rows(mag_tok, grid, r, assign64, kept64, off_cpu[0])
    worst = eu.assert_elementwise(y, ref, mag, C + 1 + max(int(torch.bincount(a[a >= 0], minlength=1).max()) for a in assign64), dtype, f"{what}: merge_norm")
    y_in = torch.randn((B, N - r, C), generator=torch.Generator().manual_seed(r)).to(dtype).to(gpu)
    (out, stats), ubufs = TU.unmerge_into(x, y_in, where)
    y64 = y_in.cpu().double()
    w_un = eu.assert_elementwise(out, tome.unmerge_reference(x64, y64, where64), tome.unmerge_reference(x64.abs(), y64.abs(), where64), 2, dtype,
                                 f"{what}: unmerge_add")
    o64 = out.cpu().double().reshape(B * N, C)
    w_st = eu.assert_elementwise(stats, torch.stack([o64.sum(-1), (o64 * o64).sum(-1)], dim=-1), torch.stack([o64.abs().sum(-1), (o64 * o64).sum(-1)], dim=-1),
                                 C, torch.float32, f"{what}: row partials")
    print(f"{what}: node_max err {err:.2e}; worst ratio to budget merge {worst:.3f} unmerge {w_un:.3f} partials {w_st:.3f}")
    for buf in (*bufs, *sbufs, ybuf, *ubufs):
        eu.assert_margins_intact(buf, what)

