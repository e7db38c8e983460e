"""st_attention_windows / ops.attention_windows (csrc/attention_windows.hip): windowed self-attention, HyperTile.

Guard-margined buffers at B = 2, H = 2, D = 64, held to tests/edge_util.py's AttentionRef (float64) per window on the tests' own gathered
copies, under that file's attention budget.  The (grid, tiling) pairs sit where the address rule can break: 96-row windows with a 32-key
tail, tw = 8, two and three groups per grid row, a window as wide as the grid, the whole grid (the bits of ops.attention).  q, k, v are
column slices of one fused buffer, except with `forms`, which pins a block form the launch's own choice would not reach at this size."""
import functools

import pytest
import torch

from stabletriton_amd import _C, hypertile as ht, ops
from tests import edge_util as eu

pytestmark = pytest.mark.gpu
B, H, D = 2, 2, 64
SCALE = D ** -0.5
# (grid, tiling, row_forms mask or None = every form that divides the window)
CASES = [((24, 16), (2, 2), None), ((32, 16), (2, 2), None), ((32, 32), (2, 2), None), ((32, 32), (1, 2), None), ((32, 48), (1, 2), None),
         ((32, 48), (2, 1), None), ((32, 32), (1, 1), None), ((32, 32), (2, 2), 1), ((32, 48), (1, 2), 1), ((32, 48), (2, 1), 4)]


@functools.lru_cache(maxsize=None)
def _inputs(T):
    return eu.attention_inputs("normal", B, T, T, H, D)[:3]


def _dev(t, gpu, dtype):
    return eu.poisoned(t.to(gpu, dtype).contiguous(), row_gap=eu.ROW_GAP)


def _fused(q, k, v, gpu, dtype):
    qkv = _dev(torch.cat([q, k, v], dim=2), gpu, dtype)      # strided token rows, as the fused projection leaves them
    return qkv.chunk(3, dim=2)


def windows_into(out, q, k, v, grid, tiling, forms):
    """st_attention_windows into the caller's `out` (ops.attention_windows' argument plumbing); token strides as they are."""
    Tw = (grid[0] // tiling[0]) * (grid[1] // tiling[1])
    forms = forms or sum(1 << i for i, r in enumerate(ht.ROW_FORMS) if Tw % r == 0)
    _C.check(_C.load().st_attention_windows(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), q.shape[0], grid[0], grid[1], H, D,
                                            q.stride(1), k.stride(1), v.stride(1), out.stride(1), SCALE, tiling[0], tiling[1], None, None, 0,
                                            forms, _C.dtype_code(q.dtype), _C.stream_ptr()), "attention_windows")


def _gather(t, grid, tiling):
    """(B, gh * gw, C) -> window-major (B * nh * nw, th * tw, C): the tests' own statement of the address rule."""
    (gh, gw), (nh, nw) = grid, tiling
    return t.reshape(t.shape[0], nh, gh // nh, nw, gw // nw, -1).transpose(2, 3).reshape(t.shape[0] * nh * nw, gh * gw // (nh * nw), -1)


def _gate(out, q, k, v, grid, tiling, dtype, what):
    g = lambda t: _gather(t, grid, tiling)
    ratio = eu.AttentionRef(g(q), g(k), g(v), H, SCALE, dtype).gate(g(out.cpu()), what)
    print(f"RATIO attention-windows {what}: {ratio:.3f} of the budget")


@pytest.mark.parametrize("dtype", eu.ATT_HALF, ids=str)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_windows_against_float64_per_window(gpu, dtype, case):
    grid, tiling, forms = case
    T = grid[0] * grid[1]
    q, k, v = _inputs(T)
    qg, kg, vg = _fused(q, k, v, gpu, dtype) if forms is None else (_dev(t, gpu, dtype) for t in (q, k, v))
    what = f"{case} {dtype}"
    out, buf = eu.guarded((B, T, H * D), dtype, gpu)
    windows_into(out, qg, kg, vg, grid, tiling, forms)
    eu.assert_margins_intact(buf, what)
    _gate(out, q, k, v, grid, tiling, dtype, what)
    if tiling == (1, 1):
        assert torch.equal(out, ops.attention(qg, kg, vg, H, SCALE)), f"{what}: the whole grid is not the bits of ops.attention"
    assert torch.equal(ops.attention_windows(qg, kg, vg, H, SCALE, grid, tiling=tiling), out), f"{what}: ops.attention_windows gives other bits"
    # no window reads another's keys: NaN in window (0, 0)'s k and v stays in window (0, 0)'s outputs
    tok = torch.arange(T)
    first = ((tok // grid[1] < grid[0] // tiling[0]) & (tok % grid[1] < grid[1] // tiling[1])).expand(B, T)
    kn, vn = kg.clone(), vg.clone()
    kn[first.to(gpu)] = float("nan")
    vn[first.to(gpu)] = float("nan")
    out2, buf2 = eu.guarded((B, T, H * D), dtype, gpu)
    windows_into(out2, qg, _dev(kn, gpu, dtype), _dev(vn, gpu, dtype), grid, tiling, forms)
    eu.assert_margins_intact(buf2, what)
    nan_rows = torch.isnan(out2).all(dim=2).cpu()
    assert torch.equal(nan_rows, first) and torch.equal(torch.isnan(out2).any(dim=2).cpu(), first), f"{what}: NaN keys of window (0, 0) reached other rows"
    assert torch.equal(out2[~first.to(gpu)], out[~first.to(gpu)])


@pytest.mark.parametrize("dtype", eu.ATT_HALF, ids=str)
def test_device_table_is_read_at_every_replay_and_clamps(gpu, dtype):
    grid, T = (32, 32), 1024
    q, k, v = _inputs(T)
    qg, kg, vg = (_dev(t, gpu, dtype) for t in (q, k, v))
    host = {t: ops.attention_windows(qg, kg, vg, H, SCALE, grid, tiling=t, rows=128) for t in ((2, 2), (1, 2))}
    assert not torch.equal(host[(2, 2)], host[(1, 2)])
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    table = torch.tensor([[2, 2], [1, 2]], dtype=torch.int32, device=gpu)
    ops.attention_windows(qg, kg, vg, H, SCALE, grid, table=(step, table), rows=128)      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attention_windows(qg, kg, vg, H, SCALE, grid, table=(step, table), rows=128)
    for s, want in ((0, (2, 2)), (1, (1, 2)), (5, (1, 2)), (0, (2, 2))):
        step.fill_(s)
        graph.replay()
        assert torch.equal(out, host[want]), f"step {s}: not the bits of the host tiling {want}"
    table[0, 0] = 1                      # an in-place write of the row is followed
    graph.replay()
    assert torch.equal(out, host[(1, 2)])


@pytest.mark.parametrize("tag,dtype,grid,tiling,fused", [("forced", torch.bfloat16, (32, 16), (2, 2), False), ("fp32", torch.float32, (32, 16), (2, 2), None),
                                                       ("tw4", torch.float16, (32, 16), (2, 4), None)], ids=["forced", "fp32", "tw4"])
def test_slow_path(gpu, tag, dtype, grid, tiling, fused):
    T = grid[0] * grid[1]
    q, k, v = _inputs(T)
    qg, kg, vg = (t.to(gpu, dtype) for t in (q, k, v))
    if fused is None:
        with pytest.raises(ops.BackendError, match="attention_windows"):
            ops.attention_windows(qg, kg, vg, H, SCALE, grid, tiling=tiling, fused=True)
    out = ops.attention_windows(qg, kg, vg, H, SCALE, grid, tiling=tiling, fused=fused)
    _gate(out, q, k, v, grid, tiling, dtype, f"slow path {tag}")

