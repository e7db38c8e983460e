"""Tiled denoising on the host: the window grid, the weight maps, the CPU route of tiles.gather / tiles.blend against the tests' own
float64 statement (tests/tiles_util.py), the binding and the entry points' argument validation, and what DenoiseLoop refuses.  No GPU."""
import ctypes
import os
import re

import pytest
import torch
from torch import fx

from stabletriton_amd import _C, tiles as T
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import tiles_util as TU


# ------------------------------------------------------------------------------------------------ 1. the grid
@pytest.mark.parametrize("args,want", [((10, 4, 3), [0, 3, 6]), ((11, 4, 3), [0, 3, 6, 7]), ((10, 4, 3, True), [0, 3, 6, 9]),
                                       ((4, 4, 1), [0]), ((4, 4, 2), [0]), ((4, 4, 3), [0]), ((4, 4, 4), [0]),
                                       ((16, 16, 8), [0]), ((24, 16, 8), [0, 8]), ((24, 16, 8, True), [0, 8, 16]), ((28, 16, 6), [0, 6, 12]),
                                       ((20, 16, 4), [0, 4]), ((32, 16, 16), [0, 16]), ((19, 4, 1), list(range(16)))])
def test_tile_starts(args, want):
    assert T.tile_starts(*args) == want
    assert want == TU.starts(*args)


@pytest.mark.parametrize("args,match", [((3, 4, 2), "does not fit"), ((10, 4, 0), "at least 1"), ((10, 4, -2), "at least 1"),
                                        ((10, 4, 5), "gap"), ((20, 4, 1), "at most 16"), ((17, 4, 1, True), "at most 16"),
                                        ((1 << 40, 4, 1), "at most 16")])
def test_tile_starts_errors(args, match):
    with pytest.raises(ValueError, match=match):
        T.tile_starts(*args)


def test_tile_grid():
    g = T.TileGrid((20, 28), 16, (4, 6))
    assert (g.ys, g.xs, g.T) == ([0, 4], [0, 6, 12], 6)
    assert [g.window(t) for t in range(g.T)] == TU.windows_of(g.ys, g.xs) == [(0, 0), (0, 6), (0, 12), (4, 0), (4, 6), (4, 12)]
    g = T.TileGrid(24, (16, 16))                               # default stride: half the window
    assert (g.ys, g.xs, g.stride) == ([0, 8], [0, 8], (8, 8))
    g = T.TileGrid((16, 24), 16, wrap_w=True)                  # wrap applies to the width only
    assert (g.ys, g.xs) == ([0], [0, 8, 16])
    g = T.TileGrid((7, 9), 4, 2)                               # canvas sides are free
    assert (g.ys, g.xs) == ([0, 2, 3], [0, 2, 4, 5])
    for bad in (dict(tile_hw=6), dict(tile_hw=(16, 10)), dict(tile_hw=0)):
        with pytest.raises(ValueError, match="multiples of 4"):
            T.TileGrid((20, 28), **bad)
    with pytest.raises(ValueError, match="larger than the canvas"):
        T.TileGrid((16, 24), 32)
    with pytest.raises(ValueError, match="gap"):
        T.TileGrid((16, 64), 16, 20)


def test_weight_maps():
    g = T.gaussian_weights(8, 12)
    assert g.dtype == torch.float32 and tuple(g.shape) == (8, 12)
    assert float((g.double() - TU.gaussian64(8, 12)).abs().max()) <= 2.0 ** -24
    assert torch.equal(g, g.flip(0)) and torch.equal(g, g.flip(1)) and float(g[0, 0]) < float(g[3, 5])
    assert torch.equal(T.weight_map("uniform", (4, 8)), torch.ones(4, 8))
    assert torch.equal(T.weight_map("gaussian", (16, 16)), T.gaussian_weights(16, 16))
    assert "unpinned" in " ".join(T.__doc__.split())
    for bad, match in ((torch.ones(4, 4), r"\(h, w\)"), ("cosine", "uniform"), (torch.zeros(4, 8), "positive"),
                       (-torch.ones(4, 8), "positive"), (torch.full((4, 8), float("nan")), "finite"),
                       (torch.full((4, 8), float("inf")), "finite")):
        with pytest.raises(ValueError, match=match):
            T.weight_map(bad, (4, 8))


# ------------------------------------------------------------------------------------------------ 2. the CPU route
CASES = {"single": (1, (4, 4), 4, 4, False, 4), "overlap": (2, (6, 10), 4, 3, False, 4), "wrap": (1, (4, 10), 4, 3, True, 4),
         "gauss": (3, (12, 20), 8, 4, False, 4), "odd": (1, (7, 9), 4, 2, False, 4), "c8": (2, (6, 10), 4, 3, False, 8)}


def _weights(name, hw):
    if name == "gauss":
        return T.gaussian_weights(*hw)
    g = torch.Generator().manual_seed(5)
    return torch.rand(hw, generator=g) + 0.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CASES))
def test_cpu_route_against_float64(name, dtype):
    rows, hw, win, stride, wrap, C = CASES[name]
    grid = T.TileGrid(hw, win, stride, wrap_w=wrap)
    gen = torch.Generator().manual_seed(11)
    canvas = (torch.randn((rows, C) + hw, generator=gen) * 3).to(dtype).contiguous(memory_format=torch.channels_last)
    wins = T.gather(canvas, grid)
    assert wins.dtype == dtype and wins.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(wins.double(), TU.cut64(canvas, grid.ys, grid.xs, grid.tile_hw)), "gather is a copy"
    # windows of their own (not cut from one canvas: overlapping windows disagree, as the UNet's predictions do)
    e = (torch.randn(tuple(wins.shape), generator=gen) * 3).to(dtype).contiguous(memory_format=torch.channels_last)
    wt = _weights(name, grid.tile_hw)
    out = T.blend(e, grid, wt)
    ref, n, mag = TU.blend64(e, grid.ys, grid.xs, hw, wt)
    assert out.dtype == dtype and tuple(out.shape) == (rows, C) + hw
    once = (n == 1).expand_as(ref)
    assert torch.equal(out.double()[once], ref[once]), "a pixel under one window takes that window's bits"
    if name != "single":
        assert int(n.max()) >= 2
    err = (out.double() - ref).abs()
    frac = float((err / TU.blend_bound(ref, n, mag, dtype).clamp_min(1e-300))[~once].max()) if bool((~once).any()) else 0.0
    assert frac <= 1.0, f"{name} {dtype}: {frac:.3g} x the bound"
    into = torch.full_like(out, 7.0)
    assert T.blend(e, grid, wt, out=into) is into and torch.equal(into, out)
    with pytest.raises(ValueError, match="do not fit"):
        T.gather(canvas[:, :, :, :-1], grid)
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        T.blend(e, grid, torch.ones(3, 3))


# ------------------------------------------------------------------------------------------------ 3. the binding
def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_binding_header_and_validation(lib):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stabletriton_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, count in (("st_tile_gather", 15), ("st_tile_blend", 16)):
        decl = re.search(rf"int {name}\((.*?)\);", text, flags=re.S)
        assert decl is not None and len(decl.group(1).split(",")) == len(_C.SIGNATURES[name][1]) == count
        assert hasattr(lib, name)
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    # argument validation happens on the host, before any launch: exercise it without a GPU
    f32, bf = _C.ST_F32, _C.ST_BF16
    CAN, WIN, WTS = 1 << 20, 1 << 22, 1 << 24                   # never dereferenced: every call below is rejected first
    ys, xs = _ints([0, 2]), _ints([0, 3, 6])                   # canvas 6 x 10, windows 4 x 4

    def gather(canvas=CAN, windows=WIN, rows=2, H=6, W=10, h=4, w=4, C=4, ys=ys, ny=2, xs=xs, nx=3, wrap=0, dtype=f32):
        return lib.st_tile_gather(canvas, windows, rows, H, W, h, w, C, ys, ny, xs, nx, wrap, dtype, None)

    def blend(canvas=CAN, windows=WIN, weights=WTS, rows=2, H=6, W=10, h=4, w=4, C=4, ys=ys, ny=2, xs=xs, nx=3, wrap=0, dtype=f32):
        return lib.st_tile_blend(windows, canvas, weights, rows, H, W, h, w, C, ys, ny, xs, nx, wrap, dtype, None)

    for call in (gather, blend):
        bad = lambda msg, **kw: call(**kw) != 0 and msg in lib.st_last_error()
        assert bad(b"null", canvas=None) and bad(b"null", windows=None) and bad(b"null", ys=None) and bad(b"null", xs=None)
        assert bad(b"unsupported dtype", dtype=_C.ST_F32S) and bad(b"bad shape", rows=0) and bad(b"multiple of 4", C=6)
        assert bad(b"larger than the canvas", h=8, ys=_ints([0]), ny=1) and bad(b"larger than the canvas", w=12, xs=_ints([0]), nx=1)
        assert bad(b"window starts", ny=0) and bad(b"window starts", nx=17)
        assert bad(b"ys[1]=3 outside", ys=_ints([0, 3])) and bad(b"ys[0]=-1 outside", ys=_ints([-1, 2]))
        assert bad(b"xs[2]=7 outside", xs=_ints([0, 3, 7])) and bad(b"xs[0]=-2 outside", xs=_ints([-2, 3, 6]))
        assert bad(b"xs[2]=10 outside", xs=_ints([0, 3, 10]), wrap=1), "with wrap a start lies in [0, W)"
        assert bad(b"rows not covered", H=9, ys=_ints([0, 5])) and bad(b"rows not covered", ys=_ints([2, 2]))
        assert bad(b"columns not covered", xs=_ints([0, 6, 6])) and bad(b"columns not covered", xs=_ints([0, 1, 2]))
        assert bad(b"columns not covered", xs=_ints([0, 1, 2]), wrap=1), "wrap: columns 6..9 under no window"
        assert bad(b"misaligned", canvas=CAN + 8) and bad(b"misaligned", windows=WIN + 4)
        assert bad(b"misaligned", canvas=CAN + 4, dtype=bf) and not bad(b"misaligned", canvas=CAN + 8, windows=CAN, dtype=bf)
        # canvas 2 * 6 * 10 * 4 fp32 = 1920 bytes, windows 2 * 6 * 4 * 4 * 4 fp32 = 3072: the same address and either one beginning
        # inside the other are refused
        assert bad(b"alias or overlap", windows=CAN) and bad(b"overlap", windows=CAN + 1904) and bad(b"overlap", canvas=WIN + 3056)
        big = (1 << 31) - 1
        assert bad(b"too large", rows=1 << 30, H=big, W=big, h=big, w=big, ys=_ints([0]), ny=1, xs=_ints([0]), nx=1)
    assert blend(weights=None) != 0 and b"weight map" in lib.st_last_error()
    assert blend(weights=WTS + 2) != 0 and b"weight map" in lib.st_last_error()
    assert blend(weights=CAN + 64) != 0 and b"overlap the canvas" in lib.st_last_error()


def test_launchers_reject_cpu_tensors_and_bad_shapes():
    from stabletriton_amd import ops
    c = torch.zeros(1, 4, 6, 10).contiguous(memory_format=torch.channels_last)
    w = torch.zeros(6, 4, 4, 4).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.tile_gather(c, w, [0, 2], [0, 3, 6])
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.tile_blend(w, c, torch.ones(4, 4), [0, 2], [0, 3, 6])


# ------------------------------------------------------------------------------------------------ 4. the loop's refusals
def _loop(unet=None, hw=(16, 24), **kw):
    return DenoiseLoop(unet or (lambda *a, **k: None), 1, hw, torch.float32, "cpu", euler_discrete_tables(4), cross_dim=TINY.cross_dim,
                       pooled_dim=TINY.pooled_dim, mode="eager", **kw)


def test_loop_layout_and_refusals():
    loop = _loop(tile_hw=16, guidance_scale=5.0)
    assert loop.tile_grid.xs == [0, 8] and loop.tile_grid.T == 2
    assert tuple(loop.latent.shape) == (1, 4, 16, 24) and tuple(loop.x_step.shape) == tuple(loop.eps_canvas.shape) == (2, 4, 16, 24)
    assert tuple(loop.x_in.shape) == (4, 4, 16, 16) and loop.ehs.shape[0] == loop.text_embeds.shape[0] == loop.time_ids.shape[0] == 4
    assert loop.x_step is not loop.x_in and torch.equal(loop.tile_weights, torch.ones(16, 16))
    plain = _loop(guidance_scale=5.0)
    assert plain.x_step is plain.x_in and plain.tile_grid is None and plain.eps_canvas is None and plain.tile_weights is None
    with pytest.raises(ValueError, match="multiples of 4"):
        _loop(tile_hw=10)
    with pytest.raises(ValueError, match="larger than the canvas"):
        _loop(tile_hw=32)
    with pytest.raises(ValueError, match="at most 16"):
        _loop(hw=(16, 64), tile_hw=16, tile_stride=1)
    with pytest.raises(ValueError, match="gap"):
        _loop(hw=(16, 64), tile_hw=16, tile_stride=24)
    for kw in (dict(tile_stride=8), dict(tile_wrap_w=True), dict(tile_weights="gaussian")):
        with pytest.raises(ValueError, match="need tile_hw"):
            _loop(**kw)
    with pytest.raises(ValueError, match="positive"):
        _loop(tile_hw=16, tile_weights=torch.zeros(16, 16))
    with pytest.raises(ValueError, match="without tile_hw"):
        plain.set_tile_weights("gaussian")
    # the weight map: an in-place write, validated on the host
    at = loop.tile_weights.data_ptr()
    loop.set_tile_weights("gaussian")
    assert loop.tile_weights.data_ptr() == at and torch.equal(loop.tile_weights, T.gaussian_weights(16, 16))
    for bad in (torch.ones(8, 8), torch.full((16, 16), float("inf")), -torch.ones(16, 16), "cosine"):
        with pytest.raises(ValueError):
            loop.set_tile_weights(bad)
    assert torch.equal(loop.tile_weights, T.gaussian_weights(16, 16)), "a refused map leaves the old one"


def test_conditioning_rows_per_sample_and_per_window():
    loop = DenoiseLoop(lambda *a, **k: None, 2, (16, 24), torch.float32, "cpu", euler_discrete_tables(4), cross_dim=8, pooled_dim=4,
                       tokens=3, mode="eager", guidance_scale=5.0, tile_hw=16)
    T_ = loop.tile_grid.T
    assert T_ == 2 and loop.ehs.shape[0] == 2 * 2 * T_
    mk = lambda rows, base: (torch.arange(rows).float().view(rows, 1, 1).expand(rows, 3, 8) + base, torch.arange(rows).float().view(rows, 1).expand(rows, 4) + base,
                             torch.arange(rows).float().view(rows, 1).expand(rows, 6) + base)
    loop.set_conditioning(*mk(2, 10.0), *mk(2, 20.0))          # B rows: repeated over a sample's windows; negatives first
    assert loop.text_embeds[:, 0].tolist() == [20.0, 20.0, 21.0, 21.0, 10.0, 10.0, 11.0, 11.0]
    assert loop.ehs[:, 0, 0].tolist() == loop.time_ids[:, 0].tolist() == loop.text_embeds[:, 0].tolist()
    loop.set_conditioning(*mk(4, 10.0), *mk(2, 20.0))          # B * T rows: one prompt per window, sample-major
    assert loop.text_embeds[:, 0].tolist() == [20.0, 20.0, 21.0, 21.0, 10.0, 11.0, 12.0, 13.0]
    loop.set_conditioning(*mk(4, 10.0))                        # no negatives: zeros, time ids copy the positive ones
    assert loop.text_embeds[:4].abs().max() == 0 and loop.time_ids[:, 0].tolist() == [10.0, 11.0, 12.0, 13.0] * 2
    with pytest.raises(ValueError, match="B = 2 rows .* or B \\* T = 4 rows"):
        loop.set_conditioning(*mk(3, 10.0))


@pytest.mark.parametrize("flag", [dict(regions=2), dict(ip_adapter=1), dict(t2i_adapter=True)])
def test_refused_with_row_bound_features(flag):
    with torch.device("meta"):
        m = UNet2DConditionModel(TINY).eval()
    gm = replace_backend(fx.symbolic_trace(m), **flag)
    name = next(iter(flag))
    with pytest.raises(ValueError, match=f"tile_hw cannot be combined with a UNet compiled with {name}"):
        _loop(gm, tile_hw=16, tokens=154 if name == "regions" else 77)
