"""T2I-Adapter on the host: where the fx pass puts the sites and what it leaves the other passes, the unchanged default graph, a
traced float64 TINY module carrying only this pass against the hooked eager module (tests/t2i_util.py), the adapter network's
shapes and state-dict spelling, the scale table, validation messages, and the binding.  No GPU."""
import operator

import pytest
import torch
from torch import fx

from stabletriton_amd import _C, synth, t2i_adapter as T
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.optimizers import insert_t2i_adapter
from stabletriton_amd.optimizers.wrappers import group_norm_wrapper
from stabletriton_amd.unet import SDXL_BASE, TINY, TINY_REFINER, UNet2DConditionModel, UNetWithLabelVector
from tests import t2i_util as TU


def _meta(spec, wrap=False):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec).eval()
        return UNetWithLabelVector(m) if wrap else m


def _sites(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is T.t2i_site]


def _cats_on_channels(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target in (torch.cat, torch.concat)
            and n.kwargs.get("dim", n.args[1] if len(n.args) > 1 else 0) == 1]


# ------------------------------------------------------------------------------------------------ 1. the pass
@pytest.mark.parametrize("spec,wrap,count", [(TINY, False, 4), (TINY, True, 4), (SDXL_BASE, False, 4), (TINY_REFINER, False, 5)])
def test_site_counts_and_what_the_other_passes_keep(spec, wrap, count):
    plain = replace_backend(fx.symbolic_trace(_meta(spec, wrap)))
    gm = replace_backend(fx.symbolic_trace(_meta(spec, wrap)), t2i_adapter=True)
    st = gm.rewrite_stats
    assert st["t2i_adapter_sites"] == count == len(spec.widths) + 1 and len(_sites(gm)) == count
    assert [n.args[2] for n in _sites(gm)] == list(range(count))
    # every other count is the plain module's: fuse_skip_cat still removes every concatenation and no GroupNorm is left to a
    # statistics pass that the plain module fuses
    assert {k: v for k, v in st.items() if k != "t2i_adapter_sites"} == dict(plain.rewrite_stats)
    assert not _cats_on_channels(gm)
    left = lambda g: len([n for n in g.graph.nodes if n.op == "call_function" and n.target is group_norm_wrapper])
    assert left(gm) == left(plain)
    # every site took its producer's partials and hands its own on
    for n in _sites(gm):
        assert n.kwargs.get("emit_colstats") is True and isinstance(n.kwargs.get("src_stats"), fx.Node)
        assert {u.args[1] for u in n.users if u.target is operator.getitem} == {0, 1}
    state = gm.t2i_adapter
    assert isinstance(state, T.T2IAdapterState) and state.host_scale == 0.0
    w = spec.widths
    assert state.channels == (w[0],) + tuple(w[1:]) + (w[-1],)
    assert state.levels == (1,) + tuple(range(1, len(w))) + (len(w) - 1,)


def test_sdxl_sites_and_comfy_input_blocks():
    gm = replace_backend(fx.symbolic_trace(_meta(SDXL_BASE, True)), t2i_adapter=True)
    st = gm.t2i_adapter
    assert st.channels == (320, 640, 1280, 1280) and st.levels == (1, 1, 2, 2)
    assert st.input_blocks == (3, 5, 8, None)           # ComfyUI's input_blocks 3 (the first downsampler), 5, 8, and the middle block
    assert st.site_shapes(128) == [(320, 64, 64), (640, 64, 64), (1280, 32, 32), (1280, 32, 32)]
    assert st.site_shapes((152, 104)) == [(320, 76, 52), (640, 76, 52), (1280, 38, 26), (1280, 38, 26)]


# `rewrite_stats` of the default compile as the commit BEFORE this pass gives them (printed from an export of that commit), in order
_COMMON = dict(deduped_activations=16, linear_silu=2, group_norm_silu=35, group_norm=11, timesteps=2, conv=51, temb_rowbias=17,
               token_residuals=11, group_norm_stats=46, skip_cats_removed=9, channels_last_views=11)
_ORDER = ("dropout", "deduped_activations", "attention", "geglu", "linear_silu", "group_norm_silu", "group_norm", "layer_norm", "linear",
          "timesteps", "conv", "geglu_in_gemm", "temb_rowbias", "residual_adds", "token_residuals", "shared_input_gemms",
          "layer_norm_in_gemm", "query_projection_in_attention", "group_norm_stats", "skip_cats_removed", "channels_last_views")
STATS_BEFORE = {
    "sdxl": dict(_COMMON, dropout=227, attention=140, geglu=70, layer_norm=210, linear=741, geglu_in_gemm=70, residual_adds=228,
                 shared_input_gemms=72, layer_norm_in_gemm=210, query_projection_in_attention=70),
    "tiny": dict(_COMMON, dropout=68, attention=34, geglu=17, layer_norm=51, linear=211, geglu_in_gemm=17, residual_adds=69,
                 shared_input_gemms=19, layer_norm_in_gemm=51, query_projection_in_attention=17),
}


@pytest.mark.parametrize("name,spec", [("sdxl", SDXL_BASE), ("tiny", TINY)])
def test_feature_off_graph_is_unchanged(name, spec):
    a = replace_backend(fx.symbolic_trace(_meta(spec)))
    b = replace_backend(fx.symbolic_trace(_meta(spec)), t2i_adapter=False)
    assert a.code == b.code and "t2i" not in a.code and not hasattr(a, "t2i_adapter")
    assert list(a.rewrite_stats.items()) == list(b.rewrite_stats.items()) == [(k, STATS_BEFORE[name][k]) for k in _ORDER]


def test_with_freeu_both_passes_keep_their_sites():
    gm = replace_backend(fx.symbolic_trace(_meta(TINY)), t2i_adapter=True, freeu=True)
    assert gm.rewrite_stats["t2i_adapter_sites"] == 4 and gm.rewrite_stats["freeu_sites"] == 6 and not _cats_on_channels(gm)


def test_not_with_fp8():
    with pytest.raises(ValueError, match="t2i_adapter=True cannot be combined with fp8=True"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), t2i_adapter=True, fp8=True)


# ------------------------------------------------------------------------------------------------ 2. TINY, float64, CPU
def _tiny64():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double()


def _call(mod, x):
    with torch.no_grad():
        return mod(x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


@pytest.mark.parametrize("hw", [16, (24, 16)])
def test_traced_module_with_sites_equals_the_hooked_eager_module(hw):
    m = _tiny64()
    x = {k: v.double() for k, v in synth.denoise_inputs(2, hw, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim).items()}
    feats = [f.double() for f in TU.features(TINY, hw, rows=2)]
    plain = _call(m, x)
    gm = fx.symbolic_trace(m)
    assert insert_t2i_adapter(gm) == 4
    state = gm.t2i_adapter
    with pytest.raises(ValueError, match="bind"):
        _call(gm, x)                                           # nothing bound yet: the site says what to call
    state.bind(2, hw, "cpu", dtype=torch.float64)
    assert torch.equal(_call(gm, x), plain), "scale 0 (the state after bind) must reproduce the plain module exactly"
    with TU.hooked(m, feats, 0.7):
        want = _call(m, x)
    moved = float((want - plain).abs().max())
    assert moved > 0.1, f"the residuals must matter for this check to mean anything (moved {moved:.2e})"
    state.set(feats, 0.7)
    got = _call(gm, x)
    assert float((got - want).abs().max()) < 1e-9
    # one feature row for every batch row
    state.set([f[:1] for f in feats], 0.7)
    with TU.hooked(m, [f[:1] for f in feats], 0.7):
        want1 = _call(m, x)
    assert float((_call(gm, x) - want1).abs().max()) < 1e-9
    state.clear()
    assert torch.equal(_call(gm, x), plain)
    # a caller's own table and step counter
    table, step = torch.tensor([0.0, 0.25, 0.0]), torch.tensor([1], dtype=torch.int32)
    with TU.hooked(m, [f[:1] for f in feats], 0.25):
        want2 = _call(m, x)
    with state.using(step, table):
        assert float((_call(gm, x) - want2).abs().max()) < 1e-9
        step.fill_(2)
        assert torch.equal(_call(gm, x), plain)
        step.fill_(7)                                          # past the table: its last entry, as the kernel clamps
        assert torch.equal(_call(gm, x), plain)
        step.fill_(-3)                                         # below it: its first
        assert torch.equal(_call(gm, x), plain)
        table[2] = 0.25
        step.fill_(7)
        assert float((_call(gm, x) - want2).abs().max()) < 1e-9


def test_skip_tensors_carry_the_residual():
    """Every reader of the value behind a site reads the site: with a residual on site A alone, a module whose decoder skip still read
    the conv's own output would differ from the hooked eager module (whose hook replaces the module's output for all readers)."""
    m = _tiny64()
    gm = fx.symbolic_trace(m)
    insert_t2i_adapter(gm)
    for n in _sites(gm):
        assert [u for u in n.args[0].users] == [n], "the value behind a site has one reader left: the site"
        assert len(n.users) >= 2 or n.args[2] == 3, "skip connection and next block both read the site (the middle site: one reader)"
    x = {k: v.double() for k, v in synth.denoise_inputs(1, 16, 99, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim).items()}
    feats = [f.double() for f in TU.features(TINY, 16)]
    only_a = [feats[0]] + [torch.zeros_like(f) for f in feats[1:]]
    gm.t2i_adapter.bind(1, 16, "cpu", dtype=torch.float64)
    gm.t2i_adapter.set(only_a, 1.0)
    with TU.hooked(m, only_a, 1.0):
        want = _call(m, x)
    assert float((_call(gm, x) - want).abs().max()) < 1e-9


# ------------------------------------------------------------------------------------------------ 3. the adapter network
@pytest.mark.parametrize("latent,shapes", [((16, 16), [(64, 8, 8), (128, 8, 8), (256, 4, 4), (256, 4, 4)]),
                                           ((96, 64), [(64, 48, 32), (128, 48, 32), (256, 24, 16), (256, 24, 16)]),
                                           ((6, 10), [(64, 3, 5), (128, 3, 5), (256, 2, 3), (256, 2, 3)])])
def test_full_adapter_xl_shapes(latent, shapes):
    ad = T.FullAdapterXL((64, 128, 256, 256)).eval()
    with torch.no_grad():
        feats = ad(torch.zeros(2, 3, 8 * latent[0], 8 * latent[1]))
    assert [tuple(f.shape[1:]) for f in feats] == shapes and all(f.shape[0] == 2 for f in feats)
    # ... which are the sizes of the UNet's sites at that latent (ceil_mode on both sides)
    state = T.T2IAdapterState([("a", 64, 1, 3), ("b", 128, 1, 5), ("c", 256, 2, 8), ("m", 256, 2, None)])
    assert state.site_shapes(latent) == shapes
    with pytest.raises(ValueError, match="multiples of 16"):
        ad(torch.zeros(1, 3, 120, 128))


def test_full_adapter_xl_state_dict_keys_and_round_trip():
    ad = T.FullAdapterXL()
    keys = set(ad.state_dict())
    want = {"conv_in.weight", "conv_in.bias", "body.1.in_conv.weight", "body.2.in_conv.weight"}
    want |= {f"body.{i}.resnets.{j}.{b}.{p}" for i in range(4) for j in range(2) for b in ("block1", "block2") for p in ("weight", "bias")}
    assert want <= keys and "body.0.in_conv.weight" not in keys and "body.3.in_conv.weight" not in keys
    assert keys - want == {"body.1.in_conv.bias", "body.2.in_conv.bias"}
    assert tuple(ad.conv_in.weight.shape) == (320, 768, 3, 3) and tuple(ad.body[2].in_conv.weight.shape) == (1280, 640, 1, 1)
    small = T.FullAdapterXL((64, 128, 256, 256))
    synth.fill_module_(small, 5)
    img = synth.normal("t2i.image", (1, 3, 64, 64), 3)
    with torch.no_grad():
        ref = small(img)
    for prefix in ("", "adapter."):
        other = T.FullAdapterXL((64, 128, 256, 256))
        other.load_adapter_state_dict({prefix + k: v.clone() for k, v in small.state_dict().items()})
        with torch.no_grad():
            assert all(torch.equal(a, b) for a, b in zip(other(img), ref))
    assert "parity unpinned" in " ".join(T.FullAdapterXL.__doc__.split())


# ------------------------------------------------------------------------------------------------ 4. tables and validation
def test_scale_table_from_factor():
    assert T.scale_table(10, 0.8, 1.0).tolist() == [pytest.approx(0.8)] * 10
    assert T.scale_table(10, 0.8, 0.5).tolist() == [pytest.approx(0.8)] * 5 + [0.0] * 5
    assert T.scale_table(7, 1.5, 0.5).tolist() == [1.5] * int(7 * 0.5) + [0.0] * (7 - int(7 * 0.5))
    assert T.scale_table(10, 1.0, 0.0).tolist() == [0.0] * 10
    assert T.scale_table(30, 1.0, 0.99).tolist() == [1.0] * 29 + [0.0]
    for bad in (dict(scale=float("nan")), dict(scale=float("inf")), dict(factor=-0.1), dict(factor=1.5)):
        with pytest.raises(ValueError):
            T.scale_table(10, **bad)


def test_validation_messages():
    gm = fx.symbolic_trace(_meta(TINY))
    insert_t2i_adapter(gm)
    st = gm.t2i_adapter
    with pytest.raises(ValueError, match=r"bind\(rows, latent_hw, device\) first"):
        st.set(TU.features(TINY, 16))
    st.bind(2, 16, "cpu", dtype=torch.float32, feature_rows=1)
    feats = TU.features(TINY, 16)
    st.set(feats, 0.5)
    assert st.host_scale == 0.5 and float(st._own()[0]) == 0.5
    with pytest.raises(ValueError, match="takes 4 feature maps"):
        st.set(feats[:3])
    with pytest.raises(ValueError, match=r"feature 1 .*must be \(rows or 1, 128, h, w\)"):
        st.set([feats[0], feats[0], feats[2], feats[3]])
    with pytest.raises(ValueError, match="feature 2 .* is \\(8, 8\\)"):
        st.set([feats[0], feats[1], torch.zeros(1, 256, 8, 8), feats[3]])
    with pytest.raises(ValueError, match="has 2 rows; the buffers hold 1"):
        st.set([f.repeat(2, 1, 1, 1) for f in feats])
    with pytest.raises(ValueError, match="no buffers for 3 rows"):
        st.set(feats, rows=3)
    with pytest.raises(ValueError, match="feature_rows 2"):
        st.bind(3, 16, "cpu", feature_rows=2)
    with pytest.raises(ValueError, match="asked for 2 feature rows"):
        st.bind(2, 16, "cpu", dtype=torch.float32, feature_rows=2)
    with pytest.raises(ValueError, match="int32 tensor of one entry"):
        with st.using(torch.zeros(1), torch.zeros(3)):
            pass
    plain = fx.symbolic_trace(_meta(TINY))
    with pytest.raises(ValueError, match="compiled without T2I-Adapter sites; compile it with t2i_adapter=True"):
        T.state_of(plain, "set_t2i_adapter")
    assert T.state_of(gm, "x") is st


def test_comfy_control_lists_land_on_the_sites():
    st = T.T2IAdapterState([("a", 320, 1, 3), ("b", 640, 1, 5), ("c", 1280, 2, 8), ("m", 1280, 2, None)])
    a, b, c, m = (torch.zeros(1) + i for i in range(4))
    # ComfyUI pops from the end: the entry for input block j is the j-th from the end of a list of nine
    inputs = [None] * 9
    inputs[-1 - 3], inputs[-1 - 5], inputs[-1 - 8] = a, b, c
    got = T.comfy_features(st, {"input": inputs, "middle": [m], "output": []})
    assert [g is w for g, w in zip(got, (a, b, c, m))] == [True] * 4
    assert T.comfy_features(st, {"input": [None] * 9, "middle": []}) == [None] * 4
    assert len(inputs) == 9, "the caller's lists are not consumed"
    bad = [None] * 9
    bad[-1 - 4] = a
    with pytest.raises(NotImplementedError, match="input block 4"):
        T.comfy_features(st, {"input": bad})
    with pytest.raises(NotImplementedError, match="output"):
        T.comfy_features(st, {"input": inputs, "output": [a]})
    with pytest.raises(NotImplementedError, match="more than one"):
        T.comfy_features(st, {"middle": [a, m]})


# ------------------------------------------------------------------------------------------------ 5. the binding
def test_binding_header_and_exports_agree(lib):
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stabletriton_amd.h")).read()
    decl = re.search(r"int st_residual_add\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    assert decl is not None and len(decl.group(1).split(",")) == len(_C.SIGNATURES["st_residual_add"][1]) == 14
    assert hasattr(lib, "st_residual_add")
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    # argument validation happens on the host, before any launch: exercise it without a GPU
    bf = _C.ST_BF16
    X, F, TAB, STEP, STATS = 1 << 20, 1 << 21, 1 << 22, (1 << 22) + 64, 1 << 23      # never dereferenced: every call below is rejected first
    call = lambda *a: lib.st_residual_add(*a, None)
    assert call(None, F, 1, 1, 16, 32, TAB, 1, STEP, bf, None, 0, 0) != 0 and b"null" in lib.st_last_error()
    assert call(X, F, 3, 2, 16, 32, TAB, 1, STEP, bf, None, 0, 0) != 0 and b"f_rows" in lib.st_last_error()
    assert call(X, F, 2, 1, 16, 36, TAB, 1, STEP, bf, None, 0, 0) != 0 and b"multiple of 8" in lib.st_last_error()
    assert call(X, F + 8, 2, 1, 16, 32, TAB, 1, STEP, bf, None, 0, 0) != 0 and b"misaligned" in lib.st_last_error()
    assert call(X, F, 2, 1, 16, 32, TAB, 1, STEP, bf, STATS, 0, 2) != 0 and b"do not agree" in lib.st_last_error()
    assert call(X, F, 2, 1, 16, 32, TAB, 1, STEP, bf, STATS, 5, 2) != 0 and b"do not divide" in lib.st_last_error()
    assert call(X, F, 2, 1, 16, 32, TAB, 1, STEP, bf, STATS, 8, 3) != 0 and b"statistics tiles" in lib.st_last_error()
    assert call(X, F, 2, 1, 16, 32, TAB, 0, STEP, bf, None, 0, 0) != 0 and b"scale table" in lib.st_last_error()
    # x is 2 * 16 * 32 bf16 = 2048 bytes, f 1024: the same address, an f that begins inside x and an x that begins inside f are refused
    assert call(X, X, 2, 1, 16, 32, TAB, 1, STEP, bf, None, 0, 0) != 0 and b"alias or overlap" in lib.st_last_error()
    assert call(X, X + 512, 2, 1, 16, 32, TAB, 1, STEP, bf, None, 0, 0) != 0 and b"overlap" in lib.st_last_error()
    assert call(X + 1008, X, 2, 1, 16, 32, TAB, 1, STEP, bf, None, 0, 0) != 0 and b"overlap" in lib.st_last_error()

def test_launcher_rejects_cpu_tensors():
    from stabletriton_amd import ops
    x = torch.zeros(1, 32, 4, 4)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.residual_add(x, x.clone(), torch.zeros(1), torch.zeros(1, dtype=torch.int32))
