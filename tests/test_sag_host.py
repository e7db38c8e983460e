"""Self-attention guidance on the host: the site pass, the refused combinations, the torch slow path of the column sums and the
loop's `set_sag` validation (no GPU)."""
import pytest
import torch
from torch import fx, nn

from stabletriton_amd import sag
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel


def _meta(spec):
    with torch.device("meta"):
        return UNet2DConditionModel(spec).eval()


@pytest.mark.parametrize("spec", [TINY, SDXL_BASE])
def test_one_site_and_every_other_rewrite_as_without_the_flag(spec):
    off = replace_backend(fx.symbolic_trace(_meta(spec)))
    assert "sag_sites" not in off.rewrite_stats and not hasattr(off, "sag")
    assert off.rewrite_stats == replace_backend(fx.symbolic_trace(_meta(spec)), sag_layer=None).rewrite_stats
    on = replace_backend(fx.symbolic_trace(_meta(spec)), sag_layer=True)
    stats = dict(on.rewrite_stats)
    assert stats.pop("sag_sites") == 1 and stats == off.rewrite_stats
    assert on.sag.site.endswith("mid_block.attentions.0.transformer_blocks.0.attn1") and on.sag.rows == 0
    leaves = [n for n in on.graph.nodes if n.op == "call_function" and n.target is sag.attention_sag_wrapper]
    assert len(leaves) == 1
    named = replace_backend(fx.symbolic_trace(_meta(spec)), sag_layer=r"down_blocks\.1\.attentions\.0\.transformer_blocks\.0\.attn1$")
    assert named.sag.site.startswith("down_blocks.1") and named.rewrite_stats["sag_sites"] == 1
    both = replace_backend(fx.symbolic_trace(_meta(spec)), sag_layer=True, hypertile_layers=(".*",))      # HyperTile takes the other sites
    assert both.rewrite_stats["hypertile_sites"] == off.rewrite_stats["attention"] // 2 - 1


@pytest.mark.parametrize("pattern,count", [("no_such_block", "no self-attention"), ("mid", "selects 2"), (r"attn1$", "selects")])
def test_patterns_that_select_zero_or_several_sites_raise(pattern, count):
    with pytest.raises(ValueError, match=count):
        replace_backend(fx.symbolic_trace(_meta(TINY)), sag_layer=pattern)


@pytest.mark.parametrize("flag,value", [("pag_layers", ("mid",)), ("seg_layers", ("mid",)), ("reference_layers", (".*",)),
                                        ("style_aligned_layers", (".*",)), ("regions", 2), ("ip_adapter", 4), ("t2i_adapter", True),
                                        ("controlnet", True), ("fp8", True)])
def test_refused_combinations_name_the_flag(flag, value):
    with pytest.raises(ValueError, match=f"sag_layer cannot be combined with {flag}"):
        replace_backend(_meta(TINY), sag_layer=True, **{flag: value})


@pytest.mark.parametrize("shape", [(2, 5, 1, 8), (1, 33, 3, 16)])
def test_colsum_slow_path_equals_the_float64_reduction(shape):
    B, T, H, D = shape
    gen = torch.Generator().manual_seed(T)
    q, k = torch.randn((B, T, H * D), generator=gen), torch.randn((B, T, H * D), generator=gen) * 2.0
    heads = lambda t: t.double().reshape(B, T, H, D).transpose(1, 2)
    ref = torch.softmax(heads(q) @ heads(k).transpose(-2, -1) * 0.3, dim=-1).sum(dim=2).mean(dim=1)
    from stabletriton_amd import ops
    out = torch.full((B, T), -7.0)
    got = ops.attention_colsum(q, k, H, 0.3, rows=B - 1 if B > 1 else B, out=out)      # CPU tensors: the slow path
    n = B - 1 if B > 1 else B
    assert got is out and bool((out[n:] == -7.0).all())
    assert float((out[:n].double() - ref[:n]).abs().max()) <= 16 * T * 2.0 ** -24      # T fp32 terms of at most 1 per sum
    assert float((out[:n].double().sum(dim=1) - T).abs().max()) <= 16 * T * 2.0 ** -24


class _NoUNet(nn.Module):
    def __init__(self, with_sag=True):
        super().__init__()
        if with_sag:
            self.sag = sag.SAG("mid_block.attentions.0.transformer_blocks.0.attn1", sag.DEFAULT_SITE)


def _loop(unet=None, **kw):
    return DenoiseLoop(unet or _NoUNet(), 2, (24, 16), torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8, pooled_dim=6, tokens=3, **kw)


def test_loop_buffers_and_set_sag_validation():
    unet = _NoUNet()
    lp = _loop(unet, guidance_scale=5.0, sag_scale=0.5, sag_sigma=1.5)
    assert lp.x_in.shape[0] == 4 and lp.x_sag.shape == (2, 4, 24, 16) and torch.equal(lp.sag, torch.full((10,), 0.5))
    assert (unet.sag.sigma, unet.sag.threshold) == (1.5, 1.0) and lp.sigma.numel() == 10
    table = lp.sag
    lp.set_sag([0.1 * i for i in range(10)], threshold=0.75)
    assert lp.sag is table and abs(float(lp.sag[4]) - 0.4) < 1e-6 and (unet.sag.sigma, unet.sag.threshold) == (1.5, 0.75)
    lp.set_sag(sigma=3.0)
    assert abs(float(lp.sag[4]) - 0.4) < 1e-6 and unet.sag.sigma == 3.0
    for bad, match in ((dict(scale=[1.0] * 9), "set_sag"), (dict(sigma=0.0), "sigma"), (dict(scale=1.0, threshold=float("nan")), "threshold")):
        with pytest.raises(ValueError, match=match):
            lp.set_sag(**bad)
    assert abs(float(lp.sag[4]) - 0.4) < 1e-6, "a refused call writes nothing"
    with pytest.raises(ValueError, match="needs guidance_scale"):
        _loop(sag_scale=0.5)
    with pytest.raises(ValueError, match="sag_layer"):
        _loop(_NoUNet(with_sag=False), guidance_scale=5.0, sag_scale=0.5)
    for kw in (dict(pag_scale=1.0), dict(seg_scale=1.0), dict(tile_hw=(16, 16)), dict(reference=True), dict(style_aligned=True)):
        with pytest.raises(ValueError, match="sag_scale cannot be combined"):
            _loop(guidance_scale=5.0, sag_scale=0.5, **kw)
    with pytest.raises(ValueError, match="set_sag"):
        _loop(guidance_scale=5.0).set_sag(1.0)
