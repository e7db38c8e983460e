"""ControlNet on the host: where the fx pass puts the leaf and what it leaves the other passes, the unchanged default graph, a traced
float64 TINY module carrying only this pass against the restated eager `denoise` with the residuals of the eager float64 branch
(tests/controlnet_util.py), the branch network's shapes and state-dict spelling, the start / end table, flag combinations,
validation messages, the entry point's argument checks, and the hooks' argument routing.  No GPU."""
import operator

import pytest
import torch
from torch import fx

from stabletriton_amd import _C, controlnet as CN, synth
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.optimizers import insert_controlnet
from stabletriton_amd.optimizers.wrappers import group_norm_wrapper
from stabletriton_amd.unet import SDXL_BASE, TINY, TINY_REFINER, UNet2DConditionModel, UNetWithLabelVector
from tests import controlnet_util as CU
from tests.test_t2i_adapter_host import _ORDER, STATS_BEFORE


def _meta(spec, wrap=False):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec).eval()
        return UNetWithLabelVector(m) if wrap else m


def _leaves(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is CN.controlnet_sites]


def _cats_on_channels(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target in (torch.cat, torch.concat)
            and n.kwargs.get("dim", n.args[1] if len(n.args) > 1 else 0) == 1]


# ------------------------------------------------------------------------------------------------ 1. the pass
@pytest.mark.parametrize("spec,wrap,count", [(TINY, False, 10), (TINY, True, 10), (SDXL_BASE, False, 10), (TINY_REFINER, False, 13)])
def test_site_counts_and_what_the_other_passes_keep(spec, wrap, count):
    plain = replace_backend(fx.symbolic_trace(_meta(spec, wrap)))
    gm = replace_backend(fx.symbolic_trace(_meta(spec, wrap)), controlnet=True)
    st = gm.rewrite_stats
    assert st["controlnet_sites"] == count and len(_leaves(gm)) == 1
    # every other count is the plain module's: fuse_skip_cat still removes every concatenation and no GroupNorm is left to a
    # statistics pass that the plain module fuses
    assert {k: v for k, v in st.items() if k != "controlnet_sites"} == dict(plain.rewrite_stats)
    assert not _cats_on_channels(gm)
    left = lambda g: len([n for n in g.graph.nodes if n.op == "call_function" and n.target is group_norm_wrapper])
    assert left(gm) == left(plain)
    # the leaf took every producer's partials and hands its own on: values 0..n-1, statistics n..2n-1
    leaf = _leaves(gm)[0]
    assert len(leaf.args[1]) == count - 1 and len(leaf.kwargs["src_stats"]) == count
    assert all(isinstance(s, fx.Node) for s in leaf.kwargs["src_stats"])
    assert {u.args[1] for u in leaf.users if u.target is operator.getitem} == set(range(2 * count))
    state = gm.controlnet
    assert isinstance(state, CN.ControlNetState) and state.host_scale == 0.0 and len(state.sites) == count
    assert list(state.channels) == [c for c, _, _ in CU.site_shapes(spec, 1)]
    assert state.site_shapes((24, 16)) == CU.site_shapes(spec, (24, 16)) and state.site_shapes(6) == CU.site_shapes(spec, 6)
    assert state.sites[0] == "conv_in" and state.sites[-1] == "mid_block"


def test_only_the_decoder_reads_the_leaf():
    gm = fx.symbolic_trace(_meta(TINY))
    assert insert_controlnet(gm) == 10
    leaf = _leaves(gm)[0]
    order = {n: i for i, n in enumerate(gm.graph.nodes)}
    outs = {u.args[1]: u for u in leaf.users}
    assert sorted(outs) == list(range(10))
    cats = _cats_on_channels(gm)
    cats = [c for c in cats if any("up_blocks" in str(u.target) for u in c.users)]
    assert len(cats) == 9
    for j, cat in enumerate(cats):                             # the decoder pops: concatenation j reads skip 8 - j
        assert cat.args[0][1] is outs[8 - j]
        assert list(outs[8 - j].users) == [cat]
    assert cats[0].args[0][0] is outs[9] and leaf.args[0].users.keys() == {leaf}
    for skip in leaf.args[1]:                                  # the encoder's readers keep the original node, and run before the leaf
        others = [u for u in skip.users if u is not leaf]
        assert others and all(order[u] < order[leaf] for u in others), skip
    # every node of the middle block precedes the leaf, every node of the decoder follows
    for n in gm.graph.nodes:
        if n.op == "call_module" and ("mid_block" in str(n.target) or "down_blocks" in str(n.target)):
            assert order[n] < order[leaf]
        if n.op == "call_module" and "up_blocks" in str(n.target):
            assert order[n] > order[leaf]


@pytest.mark.parametrize("name,spec", [("sdxl", SDXL_BASE), ("tiny", TINY)])
def test_feature_off_graph_is_unchanged(name, spec):
    a = replace_backend(fx.symbolic_trace(_meta(spec)))
    b = replace_backend(fx.symbolic_trace(_meta(spec)), controlnet=False)
    assert a.code == b.code and "controlnet" not in a.code and not hasattr(a, "controlnet")
    assert list(a.rewrite_stats.items()) == list(b.rewrite_stats.items()) == [(k, STATS_BEFORE[name][k]) for k in _ORDER]


def test_with_freeu_both_passes_keep_their_sites():
    plain = replace_backend(fx.symbolic_trace(_meta(TINY)), freeu=True)
    gm = replace_backend(fx.symbolic_trace(_meta(TINY)), controlnet=True, freeu=True)
    assert gm.rewrite_stats["controlnet_sites"] == 10 and not _cats_on_channels(gm)
    assert {k: v for k, v in gm.rewrite_stats.items() if k != "controlnet_sites"} == dict(plain.rewrite_stats)


def test_flag_combinations():
    with pytest.raises(ValueError, match="controlnet=True cannot be combined with t2i_adapter=True"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), controlnet=True, t2i_adapter=True)
    with pytest.raises(ValueError, match="controlnet=True cannot be combined with fp8=True"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), controlnet=True, fp8=True)
    with pytest.raises(ValueError, match="the sites cannot be placed"):
        insert_controlnet(fx.symbolic_trace(torch.nn.Sequential(torch.nn.Conv2d(4, 4, 1))))


# ------------------------------------------------------------------------------------------------ 2. TINY, float64, CPU
def _tiny64(spec=TINY):
    m = UNet2DConditionModel(spec).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double()


def _args(x):
    return x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]}


def _inputs(spec, rows, hw):
    x = synth.denoise_inputs(rows, hw, 1234, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    x = {k: v.double() for k, v in x.items()}
    if spec.n_time_ids != x["time_ids"].shape[1]:
        x["time_ids"] = x["time_ids"][:, :spec.n_time_ids]
    return x


@pytest.mark.parametrize("spec,hw", [(TINY, 16), (TINY, (24, 16)), (TINY_REFINER, 16)])
def test_traced_module_with_sites_equals_the_float64_reference(spec, hw):
    m = _tiny64(spec)
    x = _inputs(spec, 2, hw)
    net = CU.branch(spec).double()
    cond = net.embed_condition(CU.control_image(2, hw).double())
    res = CU.branch_residuals(net, *_args(x), cond)
    n = len(res)
    assert [tuple(r.shape[1:]) for r in res] == CU.site_shapes(spec, hw) and all(r.shape[0] == 2 for r in res)
    with torch.no_grad():
        plain = m(*_args(x))[0]
        assert torch.equal(CU.controlled(m, *_args(x))[0], plain), "the restated denoise is the module's own"
        want = CU.controlled(m, *_args(x), res, 0.7)[0]
    moved = float((want - plain).abs().max())
    assert moved > 10 * 1e-3, f"the residuals must matter for this check to mean anything (moved {moved:.2e})"
    gm = fx.symbolic_trace(m)
    assert insert_controlnet(gm) == n
    state = gm.controlnet
    with torch.no_grad():
        with pytest.raises(ValueError, match="bind"):
            gm(*_args(x))                                      # nothing bound yet: the leaf says what to call
        state.bind(2, hw, "cpu", dtype=torch.float64)
        assert torch.equal(gm(*_args(x))[0], plain), "scale 0 (the state after bind) must reproduce the plain module exactly"
        state.set(res, 0.7)
        assert float((gm(*_args(x))[0] - want).abs().max()) < 1e-9
        state.clear()
        assert torch.equal(gm(*_args(x))[0], plain)
        # per-site weights, one of them 0
        w = [0.5 + 0.125 * k for k in range(n)]
        w[2] = 0.0
        state.set_site_weights(w)
        state.set_scale(0.7)
        want_w = CU.controlled(m, *_args(x), res, 0.7, w)[0]
        assert float((gm(*_args(x))[0] - want_w).abs().max()) < 1e-9
        state.set_site_weights(None)
        # a caller's own table, step counter and residuals: the buffers (now zeroed) are not read
        state.set([torch.zeros_like(r) for r in res], 0.7)
        table, step = torch.tensor([0.0, 0.25, 0.0]), torch.tensor([1], dtype=torch.int32)
        want2 = CU.controlled(m, *_args(x), res, 0.25)[0]
        with state.using(step, table, residuals=res):
            assert float((gm(*_args(x))[0] - want2).abs().max()) < 1e-9
            step.fill_(2)
            assert torch.equal(gm(*_args(x))[0], plain)
            step.fill_(7)                                      # past the table: its last entry, as the kernel clamps
            assert torch.equal(gm(*_args(x))[0], plain)
        with state.using(step, table):                         # without residuals=: the state's buffers
            step.fill_(1)
            assert torch.equal(gm(*_args(x))[0], plain)


def test_the_encoder_sees_the_unmodified_skip():
    """With a residual on one early skip alone, a module whose encoder also read the sum would differ from the reference, in which
    the next encoder layer reads the unmodified tensor."""
    m = _tiny64()
    x = _inputs(TINY, 1, 16)
    res = [r.double() for r in CU.residuals(TINY, 16)]
    only = [r if k == 1 else torch.zeros_like(r) for k, r in enumerate(res)]
    gm = fx.symbolic_trace(m)
    insert_controlnet(gm)
    gm.controlnet.bind(1, 16, "cpu", dtype=torch.float64)
    gm.controlnet.set(only, 1.0)
    with torch.no_grad():
        want = CU.controlled(m, *_args(x), only, 1.0)[0]
        assert float((gm(*_args(x))[0] - want).abs().max()) < 1e-9
        assert float((want - m(*_args(x))[0]).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------ 3. the branch network
def test_branch_state_dict_keys_and_shapes():
    net = CN.ControlNetXL()
    keys = set(net.state_dict())
    emb = {f"controlnet_cond_embedding.{n}.{p}" for n in ["conv_in", "conv_out"] + [f"blocks.{i}" for i in range(6)] for p in ("weight", "bias")}
    zero = {f"controlnet_down_blocks.{k}.{p}" for k in range(9) for p in ("weight", "bias")} | {"controlnet_mid_block.weight", "controlnet_mid_block.bias"}
    assert emb <= keys and zero <= keys and "controlnet_down_blocks.9.weight" not in keys
    sd = net.state_dict()
    chain = [tuple(sd[f"controlnet_cond_embedding.blocks.{i}.weight"].shape[:2]) for i in range(6)]
    assert tuple(sd["controlnet_cond_embedding.conv_in.weight"].shape) == (16, 3, 3, 3)
    assert chain == [(16, 16), (32, 16), (32, 32), (96, 32), (96, 96), (256, 96)]
    assert tuple(sd["controlnet_cond_embedding.conv_out.weight"].shape) == (320, 256, 3, 3)
    assert [net.controlnet_cond_embedding.blocks[i].stride for i in range(6)] == [(1, 1), (2, 2)] * 3
    assert [tuple(sd[f"controlnet_down_blocks.{k}.weight"].shape) for k in range(9)] == \
        [(c, c, 1, 1) for c in (320, 320, 320, 320, 640, 640, 640, 1280, 1280)]
    assert tuple(sd["controlnet_mid_block.weight"].shape) == (1280, 1280, 1, 1)
    assert "parity with a published checkpoint unpinned" in " ".join(CN.ControlNetXL.__doc__.split())
    # everything but the embedding and the zero convolutions is spelled as the UNet's encoder spells it
    tiny, unet = CN.ControlNetXL(TINY), UNet2DConditionModel(TINY)
    shared = {k for k in tiny.state_dict() if not k.startswith("controlnet_")}
    assert shared == {k for k in unet.state_dict() if k.split(".")[0] in ("conv_in", "time_embedding", "add_embedding", "down_blocks", "mid_block")}
    assert all(tiny.state_dict()[k].shape == unet.state_dict()[k].shape for k in shared)


@pytest.mark.parametrize("spec,hw,count", [(TINY, (16, 16), 10), (TINY, (24, 16), 10), (TINY_REFINER, (16, 16), 13)])
def test_branch_outputs_are_the_sites_shapes(spec, hw, count):
    net = CU.branch(spec)
    cond = net.embed_condition(CU.control_image(1, hw))
    assert tuple(cond.shape) == (1, spec.widths[0]) + tuple(hw), "image / 8 = latent"
    x = {k: v.float() for k, v in _inputs(spec, 2, hw).items()}
    res = CU.branch_residuals(net, *_args(x), cond)
    assert len(res) == count and [tuple(r.shape) for r in res] == [(2,) + s for s in CU.site_shapes(spec, hw)]
    assert all(float(r.abs().max()) > 0 for r in res), "filled zero convolutions: the residuals are not zero"
    with pytest.raises(ValueError, match="multiples of 8"):
        net.embed_condition(torch.zeros(1, 3, 60, 64))
    # the existing passes run over the encoder-only module with its nested output
    with torch.device("meta"):
        meta = CN.ControlNetXL(spec).eval()
    st = replace_backend(fx.symbolic_trace(meta)).rewrite_stats
    assert st["skip_cats_removed"] == 0 and st["attention"] > 0 and st["group_norm_stats"] > 0
    if spec is TINY:
        assert st["attention"] == 16 and st["group_norm_stats"] == 21


# ------------------------------------------------------------------------------------------------ 4. tables and validation
def test_scale_table_from_start_and_end():
    assert CN.scale_table(10, 0.8).tolist() == [pytest.approx(0.8)] * 10
    assert CN.scale_table(10, 0.8, 0.0, 0.5).tolist() == [pytest.approx(0.8)] * 5 + [0.0] * 5
    assert CN.scale_table(10, 1.5, 0.2, 0.75).tolist() == [0.0] * 2 + [1.5] * 5 + [0.0] * 3          # [int(2.0), int(7.5))
    assert CN.scale_table(7, 1.0, 0.5, 1.0).tolist() == [0.0] * int(7 * 0.5) + [1.0] * (7 - int(7 * 0.5))
    assert CN.scale_table(30, 1.0, 0.0, 0.99).tolist() == [1.0] * 29 + [0.0]
    assert CN.scale_table(10, 1.0, 0.3, 0.3).tolist() == [0.0] * 10
    for bad in (dict(scale=float("nan")), dict(scale=float("inf")), dict(start=-0.1), dict(end=1.5), dict(start=0.6, end=0.4)):
        with pytest.raises(ValueError):
            CN.scale_table(10, **bad)


def test_validation_messages():
    gm = fx.symbolic_trace(_meta(TINY))
    insert_controlnet(gm)
    st = gm.controlnet
    res = CU.residuals(TINY, 16, rows=2)
    with pytest.raises(ValueError, match=r"bind\(rows, latent_hw, device\) first"):
        st.set(res)
    st.bind(2, 16, "cpu", dtype=torch.float32)
    st.set(res, 0.5)
    assert st.host_scale == 0.5 and float(st._own()[0]) == 0.5 and st._own()[2].tolist() == [1.0] * 10
    st.set([r[:1] for r in res], None)                         # one row for every batch row
    assert st.host_scale == 0.5 and torch.equal(st.buffer_for(2, 0, 16, 16)[1], res[0][0])
    with pytest.raises(ValueError, match="takes 10 residuals"):
        st.set(res[:9])
    with pytest.raises(ValueError, match=r"residual 4 .*must be \(rows, 128, h, w\)"):
        st.set(res[:4] + [res[0]] + res[5:])
    with pytest.raises(ValueError, match=r"residual 9 .* is \(8, 8\)"):
        st.set(res[:9] + [torch.zeros(2, 256, 8, 8)])
    with pytest.raises(ValueError, match="has 3 rows; the buffers hold 2"):
        st.set([r[:1].repeat(3, 1, 1, 1) for r in res])
    with pytest.raises(ValueError, match="no buffers for 3 rows"):
        st.set(res, rows=3)
    with pytest.raises(ValueError, match="takes 10 finite values"):
        st.set_site_weights([1.0] * 9)
    with pytest.raises(ValueError, match="int32 tensor of one entry"):
        with st.using(torch.zeros(1), torch.zeros(3)):
            pass
    with pytest.raises(ValueError, match="residuals are 10 tensors"):
        with st.using(torch.zeros(1, dtype=torch.int32), torch.zeros(3), residuals=res[:3]):
            pass
    addr = st.buffer_for(2, 0, 16, 16).data_ptr()
    st.bind(2, 16, "cpu", dtype=torch.float32)
    assert st.buffer_for(2, 0, 16, 16).data_ptr() == addr, "binding twice keeps the buffers"
    plain = fx.symbolic_trace(_meta(TINY))
    with pytest.raises(ValueError, match="compiled without ControlNet sites; compile it with controlnet=True"):
        CN.state_of(plain, "set_controlnet")
    assert CN.state_of(gm, "x") is st


def _bound_states(which):
    """(state, values for `set`) of a traced TINY module carrying that pass, nothing bound yet."""
    from stabletriton_amd import t2i_adapter as T
    from stabletriton_amd.optimizers import insert_t2i_adapter
    from tests import t2i_util as TU
    gm = fx.symbolic_trace(_meta(TINY))
    if which == "t2i_adapter":
        insert_t2i_adapter(gm)
        return T.state_of(gm, "x"), TU.features(TINY, 16, rows=2)
    insert_controlnet(gm)
    return CN.state_of(gm, "x"), CU.residuals(TINY, 16, rows=2)


@pytest.mark.parametrize("which", ["t2i_adapter", "controlnet"])
def test_both_states_share_one_base(which):
    from stabletriton_amd.state import ResidualSites
    st, values = _bound_states(which)
    assert isinstance(st, ResidualSites) and st.label == which
    st.bind(2, 16, "cpu", dtype=torch.float32)
    keys = [(2, k, h, w) for k, (_, h, w) in enumerate(st.site_shapes(16))]
    addrs = [st.buffer_for(*key).data_ptr() for key in keys]
    assert len(set(addrs)) == len(st.sites) and st.bound_rows() == [2]
    st.bind(2, 16, "cpu", dtype=torch.float32)
    assert [st.buffer_for(*key).data_ptr() for key in keys] == addrs, "binding twice keeps every buffer at its address"
    with pytest.raises(ValueError, match="asked for 2 .* rows of torch.float64"):
        st.bind(2, 16, "cpu", dtype=torch.float64)
    with pytest.raises(ValueError, match=r"nothing is bound on meta; call bind\(rows, latent_hw, device\) first"):
        st._own("meta")
    # one order for both: (step, table, site weights or None), the state's own outside `using`, the caller's inside
    own = st._own()
    assert own[0] is own.scale and own[1] is own.step and own[2] is own.weights
    assert own.scale.dtype == torch.float32 and own.step.dtype == torch.int32 and int(own.step) == 0
    assert (own.weights is None) == (which == "t2i_adapter")
    cur = st.current("cpu")
    assert len(cur) == 3 and cur[0] is own.step and cur[1] is own.scale and cur[2] is own.weights
    step, table = torch.tensor([1], dtype=torch.int32), torch.tensor([0.0, 0.25])
    with st.using(step, table):
        cur = st.current("cpu")
        assert len(cur) == 3 and cur[0] is step and cur[1] is table and cur[2] is own.weights
    assert st._use is None and st.current("cpu")[1] is own.scale
    st.set(values, 0.5)
    assert st.host_scale == 0.5 and float(st._own().scale) == 0.5
    assert all(torch.equal(st.buffer_for(*key), v) for key, v in zip(keys, values))
    st.clear()
    assert st.host_scale == 0.0 and float(st._own().scale) == 0.0
    assert all(torch.equal(st.buffer_for(*key), v) for key, v in zip(keys, values)), "clear leaves the buffers alone"
    assert [st.buffer_for(*key).data_ptr() for key in keys] == addrs


def test_the_leaf_has_one_form_and_keeps_the_site_weights():
    st = CN.ControlNetState([("a", 4, 0), ("b", 8, 1), ("m", 8, 1)])
    assert not hasattr(st, "grouped")
    st.bind(2, (6, 4), "cpu", dtype=torch.float64)
    xs = [synth.normal(f"cn.leaf.x{k}", (2, c, h, w), 11 + k).double() for k, (c, h, w) in enumerate(st.site_shapes((6, 4)))]
    rs = [synth.normal(f"cn.leaf.r{k}", (2, c, h, w), 21 + k).double() for k, (c, h, w) in enumerate(st.site_shapes((6, 4)))]
    st.set(rs, 0.75)
    w = [0.5, 0.0, 1.5]
    st.set_site_weights(w)
    assert st._own().weights.tolist() == w
    out = CN.controlnet_sites(xs[2], xs[:2], st)
    assert len(out) == 6 and out[3:] == (None, None, None)
    for k in range(3):
        assert torch.equal(out[k], xs[k] + (0.75 * w[k]) * rs[k]) if w[k] else out[k] is xs[k]
    table, step = torch.tensor([0.0, 0.25]), torch.tensor([1], dtype=torch.int32)
    lent = [2.0 * r for r in rs]
    with st.using(step, table, residuals=lent):                # the caller's table and tensors, the state's weights
        out = CN.controlnet_sites(xs[2], xs[:2], st)
    assert torch.equal(out[0], xs[0] + (0.25 * 0.5) * lent[0]) and out[1] is xs[1] and torch.equal(out[2], xs[2] + (0.25 * 1.5) * lent[2])


def test_comfy_control_lists_land_on_the_sites():
    st = CN.ControlNetState([(f"s{k}", 4, 0) for k in range(10)])
    t = [torch.zeros(1) + i for i in range(10)]
    got = CN.comfy_residuals(st, {"input": [], "middle": [t[9]], "output": t[:9]})
    assert [g is w for g, w in zip(got, t)] == [True] * 10
    assert CN.comfy_residuals(st, {"output": [None] * 9, "middle": []}) is None
    only_mid = CN.comfy_residuals(st, {"output": [], "middle": [t[9]]})
    assert only_mid[:9] == [None] * 9 and only_mid[9] is t[9]
    some = CN.comfy_residuals(st, {"output": [None, t[1]] + [None] * 7})
    assert some[1] is t[1] and [e for k, e in enumerate(some) if k != 1] == [None] * 9
    with pytest.raises(NotImplementedError, match="carries 3 residuals; this UNet has 9 skip tensors"):
        CN.comfy_residuals(st, {"output": t[:3]})             # a short list would align with the LAST skips (ComfyUI pops): refused
    with pytest.raises(NotImplementedError, match="T2I-Adapter residuals"):
        CN.comfy_residuals(st, {"input": [t[0]], "output": t[:9]})
    with pytest.raises(NotImplementedError, match="carries 10 residuals; this UNet has 9 skip tensors"):
        CN.comfy_residuals(st, {"output": t})
    with pytest.raises(NotImplementedError, match="more than one"):
        CN.comfy_residuals(st, {"middle": [t[0], t[1]]})


# ------------------------------------------------------------------------------------------------ 5. the binding
def test_binding_header_and_argument_checks(lib):
    import ctypes
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stabletriton_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int st_residual_add_grouped\((.*?)\);", text, flags=re.S)
    assert decl is not None and len(decl.group(1).split(",")) == len(_C.SIGNATURES["st_residual_add_grouped"][1]) == 8
    fields = re.search(r"typedef struct \{([^}]*)\} st_residual_site;", text).group(1)
    assert [f.strip().split()[-1].lstrip("*") for f in fields.replace(",", ";").split(";") if f.strip()] == [n for n, _ in _C.ResidualSite._fields_]
    assert ctypes.sizeof(_C.ResidualSite) == 56
    assert hasattr(lib, "st_residual_add_grouped") and lib.st_abi_version() == _C.ABI_VERSION == 18
    # argument validation happens on the host, before any launch: exercise it without a GPU
    bf = _C.ST_BF16
    X, R, TAB, STEP, STATS, W = 1 << 20, 1 << 21, 1 << 22, (1 << 22) + 64, 1 << 23, (1 << 22) + 128      # never dereferenced
    S = _C.ResidualSite
    ok = S(X, R, None, 2, 1, 16, 32, 0, 0)                     # x 2048 bytes, r 1024

    def call(sites, n=None, dtype=bf, table=TAB, n_steps=1, step=STEP, weights=None):
        arr = (S * max(len(sites), 1))(*sites)
        return lib.st_residual_add_grouped(arr, len(sites) if n is None else n, weights, table, n_steps, step, dtype, None)

    assert call([ok], n=0) != 0 and b"0 sites" in lib.st_last_error()
    assert call([ok] * 17) != 0 and b"17 sites" in lib.st_last_error()
    assert call([ok], dtype=7) != 0 and b"unsupported dtype" in lib.st_last_error()
    assert call([ok], table=None) != 0 and b"null" in lib.st_last_error()
    assert call([ok], n_steps=0) != 0 and b"scale table" in lib.st_last_error()
    assert call([ok], weights=W + 2) != 0 and b"misaligned" in lib.st_last_error()
    far = lambda k: S(X + (k << 16), R + (k << 16), None, 2, 1, 16, 32, 0, 0)
    assert call([far(0), S(X + (1 << 16), R + (1 << 16), None, 3, 2, 16, 32, 0, 0)]) != 0 and b"site 1: f_rows" in lib.st_last_error()
    assert call([far(0), far(1), S(X + (2 << 16), R + (2 << 16), None, 2, 1, 16, 36, 0, 0)]) != 0 and b"site 2: channel count" in lib.st_last_error()
    assert call([S(X, R, STATS, 2, 1, 16, 32, 5, 2)]) != 0 and b"do not divide" in lib.st_last_error()
    assert call([S(X, R, STATS, 2, 1, 16, 32, 8, 3)]) != 0 and b"statistics tiles" in lib.st_last_error()
    assert call([S(X, X + 512, None, 2, 1, 16, 32, 0, 0)]) != 0 and b"site 0: x and f must not alias or overlap" in lib.st_last_error()
    # across sites: the same x, an x that begins inside another site's r, statistics inside another site's statistics
    assert call([far(0), S(X, R + (1 << 16), None, 2, 1, 16, 32, 0, 0)]) != 0 and b"x of site 0 and x of site 1 overlap" in lib.st_last_error()
    assert call([far(0), S(R + 1008, R + (1 << 16), None, 2, 1, 16, 32, 0, 0)]) != 0 and b"r of site 0 and x of site 1 overlap" in lib.st_last_error()
    a = S(X, R, STATS, 2, 1, 16, 32, 8, 4)                     # 4 tiles x 32 channels x 8 bytes = 1024 bytes of partials
    b = S(X + (1 << 16), R + (1 << 16), STATS + 1016, 2, 1, 16, 32, 8, 4)
    assert call([a, b]) != 0 and b"stats of site 0 and stats of site 1 overlap" in lib.st_last_error()
    assert call([a, S(X + (1 << 16), STATS + 512, None, 2, 1, 16, 32, 0, 0)]) != 0 and b"stats of site 0 and r of site 1 overlap" in lib.st_last_error()


def test_launcher_rejects_cpu_tensors():
    from stabletriton_amd import ops
    x = torch.zeros(1, 32, 4, 4)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.residual_add_grouped([x], [x.clone()], torch.zeros(1), torch.zeros(1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ 6. the hooks' argument routing
def _wrapped(monkeypatch, cls, controlnet=True, wrap=False):
    """A hooks wrapper around a traced float64 CPU module that carries only this pass: the wrapper's own routing, no kernels."""
    from types import SimpleNamespace
    from stabletriton_amd import hooks
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)      # (no device to ask on the host)
    m = _tiny64()
    gm = fx.symbolic_trace(UNetWithLabelVector(m) if wrap else m)
    if controlnet:
        insert_controlnet(gm)
    plain = gm.forward
    gm.precompute_context = lambda ehs: (ehs,)
    gm.forward_with_context = lambda sample, t, ctx, cond: plain(sample, t, ctx[0], cond)
    gm.exec_context = SimpleNamespace(refresh_derived=lambda full=False: 0)
    args = (gm, TINY, torch.float64) if cls is hooks.DiffusersUNet else (gm, torch.float64)
    return m, cls(*args, cuda_graph=False)


def test_diffusers_hook_routes_the_residual_arguments(monkeypatch):
    from stabletriton_amd import hooks
    m, unet = _wrapped(monkeypatch, hooks.DiffusersUNet)
    state = unet.compiled.controlnet
    x = _inputs(TINY, 2, 16)
    lat, t, ehs, cond = _args(x)
    res = [0.7 * r.double() for r in CU.residuals(TINY, 16, rows=2)]          # scaled by the pipeline
    with torch.no_grad():
        plain = m(*_args(x))[0]
        want = CU.controlled(m, *_args(x), res, 1.0)[0]
    copies = []
    inner = state.set
    state.set = lambda *a, **kw: (copies.append(1), inner(*a, **kw))[1]
    call = lambda **kw: unet(lat, t, encoder_hidden_states=ehs, added_cond_kwargs=cond, **kw)[0]
    on = call(down_block_additional_residuals=res[:9], mid_block_additional_residual=res[9])
    assert float((on - want).abs().max()) < 1e-9 and state.host_scale == 1.0 and len(copies) == 1
    assert torch.equal(call(down_block_additional_residuals=res[:9], mid_block_additional_residual=res[9]), on)
    assert len(copies) == 1, "the same tensor objects at the same versions are not copied twice"
    assert torch.equal(call(down_block_additional_residuals=None, mid_block_additional_residual=None), plain) and state.host_scale == 0.0
    assert torch.equal(call(), plain)
    res[3].mul_(1.0)                                           # a new version of one tensor: copied again
    assert torch.equal(call(down_block_additional_residuals=res[:9], mid_block_additional_residual=res[9]), on) and len(copies) == 2
    only_mid = call(mid_block_additional_residual=res[9])
    with torch.no_grad():
        want_mid = CU.controlled(m, *_args(x), [torch.zeros_like(r) for r in res[:9]] + [res[9]], 1.0)[0]
    assert float((only_mid - want_mid).abs().max()) < 1e-9
    with pytest.raises(NotImplementedError, match="down_intrablock_additional_residuals"):
        call(down_intrablock_additional_residuals=res[:4])
    with pytest.raises(ValueError, match="10 tensors expected"):
        call(down_block_additional_residuals=res[:5], mid_block_additional_residual=res[9])
    # a wrapper compiled without the flag ignores all three, exactly as before
    _, bare = _wrapped(monkeypatch, hooks.DiffusersUNet, controlnet=False)
    out = bare(lat, t, encoder_hidden_states=ehs, added_cond_kwargs=cond, down_block_additional_residuals=res[:9],
               mid_block_additional_residual=res[9], down_intrablock_additional_residuals=res[:4])[0]
    assert torch.equal(out, plain)


def test_comfy_hook_routes_control_output_and_middle(monkeypatch):
    from stabletriton_amd import hooks
    m, adapter = _wrapped(monkeypatch, hooks.ComfyUNet, wrap=True)
    x = _inputs(TINY, 2, 16)
    with torch.no_grad():
        tid = m.add_time_proj(x["time_ids"].flatten()).reshape(2, -1)
        y = torch.cat([x["text_embeds"], tid.double()], dim=-1)
    t = torch.full((2,), 500.0)
    res = [0.7 * r.double() for r in CU.residuals(TINY, 16, rows=2)]
    with torch.no_grad():
        want = CU.controlled(m, *_args(x), res, 1.0)[0]
        plain = m(*_args(x))[0]
    control = {"input": [], "middle": [res[9]], "output": list(res[:9])}
    on = adapter(x["latent"], t, x["encoder_hidden_states"], y, control=control)
    assert float((on - want).abs().max()) < 1e-9 and len(control["output"]) == 9, "entry i is skip i; the caller's lists are not consumed"
    assert float((adapter(x["latent"], t, x["encoder_hidden_states"], y, control=None) - plain).abs().max()) < 1e-12
    assert float((adapter(x["latent"], t, x["encoder_hidden_states"], y, control={"output": [], "middle": []}) - plain).abs().max()) < 1e-12
    with pytest.raises(NotImplementedError, match="T2I-Adapter residuals"):
        adapter(x["latent"], t, x["encoder_hidden_states"], y, control={"input": [res[0]], "output": list(res[:9])})
    _, bare = _wrapped(monkeypatch, hooks.ComfyUNet, controlnet=False, wrap=True)
    with pytest.raises(NotImplementedError, match="ControlNet residuals"):
        bare(x["latent"], t, x["encoder_hidden_states"], y, control=control)
