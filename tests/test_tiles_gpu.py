"""The tiled-denoising kernels (csrc/tiles.hip) alone, in guarded buffers, against the tests' float64 statement (tests/tiles_util.py):
st_tile_gather is a bit-exact copy; st_tile_blend returns a window's bits where one window covers a pixel and elsewhere stays inside
one rounding to the type at |ref| plus (2 n + 4) 2^-24 sum(w |e|) / sum(w)."""
import pytest
import torch

from stabletriton_amd import ops, tiles as T
from tests import tiles_util as TU
from tests.edge_util import assert_margins_intact, guarded

pytestmark = pytest.mark.gpu

# name: (rows, canvas, window, stride, wrap, C, weights)
CASES = {
    "a_single_window": (1, (4, 4), 4, 4, False, 4, "random"),        # n == 1 everywhere: the bits, whatever the weights
    "b_flush_overlap": (2, (6, 10), 4, 3, False, 4, "random"),       # flush last window; 2- and 4-fold overlap
    "c_wrap_seam": (1, (4, 10), 4, 3, True, 4, "random"),            # a window over the seam
    "d_gaussian": (3, (12, 20), 8, 4, False, 4, "gaussian"),
    "e_odd_canvas": (1, (7, 9), 4, 2, False, 4, "random"),
    "f_c8": (2, (6, 10), 4, 3, False, 8, "random"),
}


def _weights(kind, hw):
    if kind == "gaussian":
        return T.gaussian_weights(*hw)
    return torch.rand(hw, generator=torch.Generator().manual_seed(5)) + 0.5


def _nhwc(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_float64(gpu, name, dtype):
    rows, hw, win, stride, wrap, C, kind = CASES[name]
    grid = T.TileGrid(hw, win, stride, wrap_w=wrap)
    h, w = grid.tile_hw
    gen = torch.Generator().manual_seed(11)
    canvas = (torch.randn((rows, C) + hw, generator=gen) * 3).to(dtype)
    # ---- gather: a copy
    wins, wbuf = guarded((rows * grid.T, C, h, w), dtype, gpu, channels_last=True)
    ops.tile_gather(_nhwc(canvas, gpu), wins, grid.ys, grid.xs, wrap)
    assert_margins_intact(wbuf, f"{name} gather")
    assert torch.equal(wins.double().cpu(), TU.cut64(canvas, grid.ys, grid.xs, (h, w))), f"{name} {dtype}: gather must be bit exact"
    # ---- blend: windows of their own (overlapping windows disagree, as the UNet's predictions do)
    e = (torch.randn((rows * grid.T, C, h, w), generator=gen) * 3).to(dtype)
    wt = _weights(kind, (h, w))
    wt_dev = wt.to(gpu)
    out, obuf = guarded((rows, C) + hw, dtype, gpu, channels_last=True)
    ops.tile_blend(_nhwc(e, gpu), out, wt_dev, grid.ys, grid.xs, wrap)
    assert_margins_intact(obuf, f"{name} blend")
    ref, n, mag = TU.blend64(e, grid.ys, grid.xs, hw, wt)
    got = out.double().cpu()
    assert torch.isfinite(got).all(), f"{name} {dtype}: a canvas element was never stored"
    once = (n == 1).expand_as(ref)
    assert torch.equal(got[once], ref[once]), f"{name} {dtype}: a pixel under one window takes that window's bits"
    frac = 0.0
    if name == "a_single_window":
        assert bool(once.all())
    else:
        assert int(n.max()) >= (4 if name in ("b_flush_overlap", "d_gaussian", "e_odd_canvas", "f_c8") else 2)
        frac = float(((got - ref).abs() / TU.blend_bound(ref, n, mag, dtype).clamp_min(1e-300))[~once].max())
    print(f"tile_blend {name} {dtype}: worst fraction of the bound {frac:.3f} (coverage up to {int(n.max())})")
    assert frac <= 1.0
    # ---- two launches agree bit for bit
    again, abuf = guarded((rows, C) + hw, dtype, gpu, channels_last=True)
    ops.tile_blend(_nhwc(e, gpu), again, wt_dev, grid.ys, grid.xs, wrap)
    assert torch.equal(again, out)
    # ---- weights rewritten in place between two launches show in the second
    if name != "a_single_window":
        wt2 = wt.flip(0, 1) * 1.5 + 0.25
        wt_dev.copy_(wt2)
        ops.tile_blend(_nhwc(e, gpu), again, wt_dev, grid.ys, grid.xs, wrap)
        assert_margins_intact(abuf, f"{name} blend, new weights")
        ref2, _, mag2 = TU.blend64(e, grid.ys, grid.xs, hw, wt2)
        got2 = again.double().cpu()
        assert not torch.equal(got2, got)
        assert float(((got2 - ref2).abs() / TU.blend_bound(ref2, n, mag2, dtype).clamp_min(1e-300)).max()) <= 1.0


def test_route_through_tiles_module_and_refusals(gpu):
    grid = T.TileGrid((6, 10), 4, 3)
    canvas = _nhwc(torch.randn(2, 4, 6, 10, generator=torch.Generator().manual_seed(3)), gpu)
    wins = T.gather(canvas, grid)
    assert wins.is_cuda and torch.equal(wins.cpu(), T.gather(canvas.cpu(), grid))
    back = T.blend(wins, grid, torch.ones(4, 4))
    # windows cut from one canvas agree where they overlap: the mean of equal values, to one rounding of the division
    assert float((back - canvas).abs().max()) <= 2.0 ** -22 * float(canvas.abs().max())
    with pytest.raises(ops.BackendError, match="rows \\* 6"):
        ops.tile_gather(canvas, wins[:5], grid.ys, grid.xs)
    with pytest.raises(ops.BackendError, match="channels_last"):
        ops.tile_gather(canvas.contiguous(), wins, grid.ys, grid.xs)
    with pytest.raises(ops.BackendError, match="not covered"):
        ops.tile_gather(canvas, wins, [0, 2], [0, 1, 2])
    with pytest.raises(ops.BackendError, match=r"fp32 \(h, w\)"):
        ops.tile_blend(wins, canvas, torch.ones(4, 4, device=gpu, dtype=torch.float16), grid.ys, grid.xs)
