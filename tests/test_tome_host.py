"""Token merging's host side (stabletriton_amd/tome.py, optimizers/insert_tome.py): the plan arithmetic, the table draw, the plain-torch
statement, the pass's rewrite, the refused flag combinations and the binding's argument errors.  No GPU."""
import pytest
import torch
from torch import fx

from stabletriton_amd import _C, tome
from stabletriton_amd.optimization import check_feature_combination, replace_backend
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import tome_util as TU


def _traced():
    with torch.device("meta"):
        return fx.symbolic_trace(UNet2DConditionModel(TINY).eval())


def test_merged_count_and_table_draws_are_reproducible_per_seed_and_grid():
    assert all(tome.merged_count(n, ratio) == want for n, ratio, want in [(64, 0.5, 32), (64, 0.3, 0), (384, 0.5, 192), (384, 0.3, 96), (384, 0.75, 288),
                                                                            (1024, 0.75, 768), (4096, 0.5, 2048), (36, 0.5, 4)])
    a = tome.draw_offsets((16, 24), 5, 3)
    assert a.shape == (5, 96) and a.dtype == torch.uint8 and int(a.max()) == 3 and torch.equal(a, tome.draw_offsets((16, 24), 5, 3))
    assert not torch.equal(a, tome.draw_offsets((16, 24), 5, 4)) and not torch.equal(a, tome.draw_offsets((24, 16), 5, 3))      # seed, grid
    assert int(tome.draw_offsets((16, 24), 5, None).max()) == 0 and tome.merged_count(1024, 0.3) == 288
    dst, src = tome.site_tokens((16, 24), a[2])
    assert sorted(torch.cat([dst, src]).tolist()) == list(range(384)), "every token is dst or src exactly once"
    with pytest.raises(ValueError, match="even"):
        tome.site_tokens((5, 8), torch.zeros(10, dtype=torch.uint8))


def test_reference_is_the_identity_at_r_0_and_follows_the_constructed_plan():
    grid, C = (8, 8), 64
    x, off = TU.site(grid, C, torch.bfloat16, True)
    x64, gamma, beta = x.double(), *(t.double() for t in TU.norm_affine(C, torch.bfloat16))
    node_max, node_idx = TU.match64(grid, C, torch.bfloat16, True)
    where, assign, kept = tome.select_reference(node_max, node_idx, grid, 0, off[0])
    y = tome.merge_reference(x64, gamma, beta, 1e-5, grid, 0, assign, kept, off[0])
    ln = torch.nn.functional.layer_norm(x64, (C,), gamma, beta, 1e-5)
    assert torch.equal(tome.unmerge_reference(torch.zeros_like(x64), y, where), ln), "unmerge(merge(x)) at r = 0"
    where, assign, kept = tome.select_reference(node_max, node_idx, grid, 32, off[0])
    order = node_max.argsort(dim=-1, descending=True)
    assert torch.equal(kept, order[:, 32:]) and bool((assign.gather(1, order[:, :32]) >= 0).all()) and int(where.max()) == 31


def test_pass_rewrites_sites_and_refuses_combinations():
    gm = replace_backend(_traced(), tome_layers=("down_blocks.1",), tome_ratio=0.3)
    assert gm.rewrite_stats["tome_sites"] == len(gm.tome.sites) == 2 and gm.tome.ratio == 0.3
    assert "tome_sites" not in replace_backend(_traced()).rewrite_stats
    for plan in (n for n in gm.graph.nodes if n.op == "call_function" and n.target is tome.tome_plan_wrapper):
        merge, unmerge = sorted(plan.users, key=lambda n: n.target is tome.tome_unmerge_wrapper)
        qkv = next(iter(merge.users))
        assert merge.target is tome.tome_merge_wrapper and qkv.target.__name__ == "linear_cat_wrapper" and len(qkv.args[1]) == 3
        assert unmerge.args[3] is True and {u.target.__name__ for u in unmerge.users} == {"getitem"}, "norm2's fold reads the unmerge launch's partials"
    with pytest.raises(ValueError, match="tome_layers"):
        replace_backend(_traced(), tome_layers=("nowhere",))
    with pytest.raises(ValueError, match="ratio"):
        replace_backend(_traced(), tome_layers=(".*",), tome_ratio=0.9)
    for other in ("pag_layers", "seg_layers", "reference_layers", "hypertile_layers", "style_aligned_layers", "sag_layer", "fp8", "freeu"):
        kw = dict(fp8=False, regions=None, ip_adapter=None, pag_layers=None, seg_layers=None, t2i_adapter=False, tome_layers=(".*",))
        kw[other] = True if other in ("fp8", "freeu", "sag_layer") else ("mid",)
        with pytest.raises(ValueError, match=f"tome_layers cannot be combined with {other}"):
            check_feature_combination(**kw)
    with pytest.raises(ValueError, match="n_steps"):
        gm.tome.bind(0)
    x, norm = torch.randn(1, 16, 128), torch.nn.LayerNorm(128)
    plan = tome.tome_plan_wrapper(x, gm.tome)      # a CPU site: the unmerged chain
    assert plan.r is None and torch.equal(tome.tome_unmerge_wrapper(x, x, plan), x + x) and tome.tome_merge_wrapper(x, norm, plan).shape == x.shape


def test_argument_errors_come_back_without_a_gpu(lib):
    P = 1 << 20
    for call, word in ((lambda: lib.st_tome_match(None, 64, P, None, 1, 1, 8, 8, 64, P, P, _C.ST_BF16, None), b"null"),
                     (lambda: lib.st_tome_match(P, 64, P, None, 1, 1, 7, 8, 64, P, P, _C.ST_BF16, None), b"even"),
                     (lambda: lib.st_tome_match(P, 96, P, None, 1, 1, 8, 8, 96, P, P, _C.ST_BF16, None), b"multiple of 64"),
                     (lambda: lib.st_tome_match(P, 64, P, None, 1, 1, 8, 8, 64, P, P, _C.ST_F32, None), b"16-bit"),
                     (lambda: lib.st_tome_match(P, 64, P, None, 1, 1, 256, 256, 64, P, P, _C.ST_BF16, None), b"LDS"),
                     (lambda: lib.st_tome_select(P, P, P, None, 1, 1, 8, 8, 49, P, P, P, None), b"out of range"),
                     (lambda: lib.st_tome_merge_norm(P, 64, P, P, 1e-5, P, None, 1, P, P, 1, 8, 8, 64, -1, P, _C.ST_F16, None), b"out of range"),
                     (lambda: lib.st_tome_unmerge_add(P, 64, P, P, 1, 64, 65, 64, P, None, _C.ST_BF16, None), b"out of range"),
                     (lambda: lib.st_tome_unmerge_add(P, 64, P, None, 1, 64, 32, 64, P, None, _C.ST_BF16, None), b"null")):
        assert call() != 0 and word in lib.st_last_error(), (word, lib.st_last_error())


def test_hooks_pass_the_keywords_and_drive_the_state(monkeypatch):
    from types import SimpleNamespace as NS
    from stabletriton_amd import hooks
    seen = []

    def compiled(model, **kw):
        seen.append(kw)
        stub = torch.nn.Module()
        stub.forward_with_context, stub.tome = None, (tome.ToMe(ratio=kw["tome_ratio"]) if kw.get("tome_layers") else None)
        return stub

    monkeypatch.setattr(hooks, "optimize_model", compiled)
    net, kw = UNet2DConditionModel(TINY).eval(), dict(tome_layers=("down_blocks.1",), tome_ratio=0.3)
    wrapped = hooks.attach_to_diffusers(NS(unet=net), TINY, **kw).unet
    hooks.patch_comfy_model(NS(model=NS(diffusion_model=None)), net, **kw)
    assert len(seen) == 2 and all(s["tome_layers"] == kw["tome_layers"] and s["tome_ratio"] == 0.3 for s in seen)
    wrapped.compiled.tome.bind(4)
    wrapped.enable_tome(seed=3)
    assert wrapped.compiled.tome.seed == 3 and wrapped._hypertile_calls == 0
    wrapped.disable_tome()
    assert wrapped.compiled.tome.seed is None
    with pytest.raises(ValueError, match="tome_layers"):
        hooks.compile_comfy_unet(net).enable_tome()
