"""Drop-in check against the reference's OWN eager module, through the stored record of it
(tests/golden/f0_reference_schema.npz, written by `oracle/make_golden.py f0_schema` from the reference module): its
state-dict schema, the leaf modules its fx trace calls in order, and the rewrite counts the backend passes left on it."""
import torch
from torch import fx

from tests.util import golden


def _leaf_calls(m):
    traced = fx.symbolic_trace(m)
    mods = dict(traced.named_modules())
    return [(n.target, type(mods[n.target]).__name__) for n in traced.graph.nodes if n.op == "call_module"]


def test_passes_rewrite_the_reference_unet_like_the_reference_does():
    from stabletriton_amd.optimization import replace_backend
    from stabletriton_amd.unet import SDXL_BASE, UNet2DConditionModel
    from tests.test_host_logic import EXPECTED
    g = golden("f0_reference_schema")
    ref_stats = dict(zip(g["stat_names"].tolist(), g["stat_values"].tolist()))
    for k, v in EXPECTED.items():
        assert ref_stats[k] == v, (k, ref_stats[k], v)
    with torch.device("meta"):
        m = UNet2DConditionModel(SDXL_BASE)
    # the passes match leaf modules: ours calls the reference's, by name and class, in the same order
    assert _leaf_calls(m) == list(zip(g["leaf_targets"].tolist(), g["leaf_classes"].tolist()))
    gm = replace_backend(fx.symbolic_trace(m))
    assert {k: gm.rewrite_stats[k] for k in ref_stats} == ref_stats


def test_state_dict_schema_is_identical():
    from stabletriton_amd.unet import SDXL_BASE, UNet2DConditionModel
    g = golden("f0_reference_schema")
    sa = {k: tuple(int(d) for d in s.split(",") if d) for k, s in zip(g["sd_keys"].tolist(), g["sd_shapes"].tolist())}
    with torch.device("meta"):
        b = UNet2DConditionModel(SDXL_BASE)
    sb = {k: tuple(v.shape) for k, v in b.state_dict().items()}
    assert sa == sb
