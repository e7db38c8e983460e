"""Token merging in the captured loop (TINY at latent 32: the first attention level, 128 channels, has a 16 x 16 token grid and runs its
self-attention half on 128 of 256 rows) and as one site chain at SDXL's first-level width on tests/tome_util.py's 16 x 24 site."""
import functools

import pytest
import torch

from stabletriton_amd import ops, synth, tome
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import tome_util as TU

pytestmark = pytest.mark.gpu
HW, STEPS, DTYPE = 32, 4, torch.bfloat16


@functools.lru_cache(maxsize=None)
def _inputs():
    return synth.denoise_inputs(2, HW, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)


@functools.lru_cache(maxsize=None)
def _compiled(layers):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to("cuda:0", DTYPE)
    synth.fill_module_(m, 0)
    return optimize_model(m, cuda_graph=False, tome_layers=layers)


def _loop(gm, dev, mode="loop"):
    x = _inputs()
    loop = DenoiseLoop(gm, 1, HW, DTYPE, dev, euler_discrete_tables(STEPS), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode)
    loop.set_conditioning(*(x[k][1:2].to(dev, DTYPE) for k in ("encoder_hidden_states", "text_embeds", "time_ids")))
    return loop


def test_rewritten_block_launches_and_captured_loop(gpu, monkeypatch):
    gm = _compiled(("down_blocks.1",))
    assert gm.rewrite_stats["tome_sites"] == len(gm.tome.sites) == 2 and "tome_sites" not in _compiled(None).rewrite_stats
    calls = []
    for name in ("tome_match", "tome_select", "tome_merge_norm", "tome_unmerge_add", "linear", "attention"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=fn, **k: (calls.append((_n, tuple(a[0].shape))), _f(*a, **k))[1])
    noise = _inputs()["latent"][:1]
    with torch.no_grad():
        eager = _loop(gm, gpu, "eager").denoise(noise).cpu()
        first = calls[[c[0] for c in calls].index("tome_match"):[c[0] for c in calls].index("tome_unmerge_add") + 1]      # the first site, in order
        assert [c[0] for c in first] == ["tome_match", "tome_select", "tome_merge_norm", "linear", "attention", "linear", "tome_unmerge_add"], first
        assert first[0][1][1:] == (256, 128) and first[3][1][1:] == (128, 128) and first[4][1][1:] == (128, 128), \
            "q|k|v is one GEMM on N - r = 128 rows, attention likewise"
        monkeypatch.undo()
        loop = _loop(gm, gpu)
        off = loop.denoise(noise).cpu()
        graph = loop.graph
        assert graph is not None and torch.isfinite(off).all() and torch.equal(off, eager), "the replay repeats the eager bits"
        assert torch.equal(loop.denoise(noise).cpu(), off), "set_tome(None) is deterministic"
        assert not torch.equal(off, _loop(_compiled(None), gpu).denoise(noise).cpu()), "merging moves the result"
        loop.set_tome(seed=3)
        on = loop.denoise(noise).cpu()
        assert loop.graph is graph and torch.isfinite(on).all() and not torch.equal(on, off), "new offsets, no new capture"
        assert torch.equal(_loop(gm, gpu).denoise(noise).cpu(), on), "a loop that captures with the tables written gives the same bits"
        loop.set_tome(None)
        assert torch.equal(loop.denoise(noise).cpu(), off) and loop.graph is graph
    with pytest.raises(ValueError, match="tome_layers"):
        _loop(_compiled(None), gpu).set_tome(0)


def _attention64(q, k, v, heads):
    h = lambda t: t.reshape(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)
    return torch.nn.functional.scaled_dot_product_attention(h(q), h(k), h(v)).transpose(1, 2).reshape(q.shape)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_site_chain_against_float64(gpu, dtype):
    """The merged chain against its float64 chain on unit-scale inputs (cos_lo 0.5: |x| < 9, the site adds |y| of about 1); allowed: 2 x
    what the existing unmerged chain of launches deviates from ITS float64 chain on the same inputs.  Figures: profiles/tome_time.json."""
    grid, C, heads, eps = (16, 24), 640, 10, 1e-5
    x_cpu, off_cpu = TU.site(grid, C, dtype, True, 0.5)
    g = torch.Generator().manual_seed(5)
    wqkv, wo = ((torch.randn((n, C), generator=g) * C ** -0.5).to(dtype) for n in (3 * C, C))
    bo, (gamma, beta) = (0.1 * torch.randn(C, generator=g)).to(dtype), TU.norm_affine(C, dtype)
    x, off, r = x_cpu.to(gpu), off_cpu.to(gpu), tome.merged_count(384, 0.5)
    Wqkv, Wo, Bo, G, Bt = (t.to(gpu) for t in (wqkv, wo, bo, gamma, beta))

    def chain_ops(merge):
        if merge:
            where, assign, kept = ops.tome_select(*ops.tome_match(x, grid, off), grid, r, off)
            n = ops.tome_merge_norm(x, G, Bt, eps, grid, r, assign, kept, off)
        else:
            n = ops.layer_norm(x, G, Bt, eps)
        q, k, v = ops.linear(n, Wqkv).split(C, dim=-1)
        att = ops.attention(q, k, v, heads, 64 ** -0.5)
        return ops.tome_unmerge_add(x, ops.linear(att, Wo, Bo), where) if merge else ops.linear(att, Wo, Bo, residual=x)

    def chain64(merge):
        x64, w1, w2, b2, g64, bt64 = (t.double() for t in (x_cpu, wqkv, wo, bo, gamma, beta))
        if merge:
            where, assign, kept = tome.select_reference(*TU.match64(grid, C, dtype, True, 0.5), grid, r, off_cpu[0])
            n = tome.merge_reference(x64, g64, bt64, eps, grid, r, assign, kept, off_cpu[0])
        else:
            n = torch.nn.functional.layer_norm(x64, (C,), g64, bt64, eps)
        q, k, v = (n @ w1.T).split(C, dim=-1)
        o = _attention64(q, k, v, heads) @ w2.T + b2
        return tome.unmerge_reference(x64, o, where) if merge else x64 + o

    plain = float((chain_ops(False).cpu().double() - chain64(False)).abs().max())
    merged = float((chain_ops(True).cpu().double() - chain64(True)).abs().max())
    print(f"tome site chain {dtype}: max abs err merged {merged:.3e}, unmerged chain of launches {plain:.3e} (allowed: 2 x)")
    assert merged <= 2.0 * plain
