"""Regional prompts on the host: the fx pass's sites and what it leaves the other passes, the unchanged default graph, mask to
weights against hand-written values, the plain torch statement against the tests' float64 restatement (tests/regions_util.py), a
traced CPU TINY module carrying the pass, DenoiseLoop / state argument errors, and the C entry point's host-side checks.  No GPU."""
import pytest
import torch
from torch import fx

from stabletriton_amd import pag, regions, synth
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.optimizers.wrappers import attention_wrapper, ln_linear_attention_wrapper, ln_linear_wrapper
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel, UNetWithLabelVector
from tests import regions_util as RU


def _meta(spec, wrap=False):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec).eval()
        return UNetWithLabelVector(m) if wrap else m


def _targets(gm, target):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is target]


# ------------------------------------------------------------------------------------------------ 1. the pass
# attn2 sites from the specs: an encoder stage has resnets_per_level attention blocks of depths[level] layers, a decoder stage
# resnets_per_level + 1, the middle block depths[-1] layers: TINY (0, 1, 2) -> 2 + 4 + 2 + 6 + 3, SDXL-base (0, 2, 10) -> 4 + 20 + 10 + 30 + 6
@pytest.mark.parametrize("spec,want,levels", [(TINY, 17, (1, 2)), (SDXL_BASE, 70, (1, 2))])
def test_site_counts_and_lost_fusion(spec, want, levels):
    plain = replace_backend(fx.symbolic_trace(_meta(spec)))
    gm = replace_backend(fx.symbolic_trace(_meta(spec)), regions=2)
    assert gm.rewrite_stats["region_sites"] == want == len(_targets(gm, regions.attention_regions_wrapper))
    st = gm.regions
    assert isinstance(st, regions.Regions) and (st.R, st.seg_len) == (2, 77) and len(st.sites) == want
    assert all(s.endswith(".attn2") for s in st.sites) and st.levels == levels
    # the fused query projection + attention form is gone at these sites (they were all of its sites): ln_linear + the new leaf
    assert len(_targets(plain, ln_linear_attention_wrapper)) == want == plain.rewrite_stats["query_projection_in_attention"]
    assert not _targets(gm, ln_linear_attention_wrapper) and gm.rewrite_stats["query_projection_in_attention"] == 0
    for n in _targets(gm, regions.attention_regions_wrapper):
        q = n.args[0]
        assert q.target is ln_linear_wrapper and len(q.args[3]) == 1, "the query projection still folds its LayerNorm"
    # self-attention is untouched
    assert len(_targets(gm, attention_wrapper)) == len(_targets(plain, attention_wrapper)) > 0
    other = {k: v for k, v in gm.rewrite_stats.items() if k not in ("region_sites", "query_projection_in_attention")}
    assert other == {k: v for k, v in plain.rewrite_stats.items() if k != "query_projection_in_attention"}


def test_prefix_in_front_of_the_block_names_does_not_matter():
    gm = replace_backend(fx.symbolic_trace(_meta(TINY, wrap=True)), regions=3, region_tokens=64)
    assert gm.rewrite_stats["region_sites"] == 17 and (gm.regions.R, gm.regions.seg_len) == (3, 64) and gm.regions.levels == (1, 2)


@pytest.mark.parametrize("spec", [SDXL_BASE, TINY])
def test_default_graph_is_unchanged(spec):
    a = replace_backend(fx.symbolic_trace(_meta(spec)))
    b = replace_backend(fx.symbolic_trace(_meta(spec)), regions=None, region_tokens=64)
    assert a.code == b.code and "regions" not in a.code and not hasattr(a, "regions")
    assert [str(n.target) for n in a.graph.nodes] == [str(n.target) for n in b.graph.nodes]
    assert list(a.rewrite_stats.items()) == list(b.rewrite_stats.items()) and "region_sites" not in a.rewrite_stats
    assert not _targets(a, regions.attention_regions_wrapper)


def test_bad_compile_arguments_raise():
    with pytest.raises(ValueError, match="fp8"):
        replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True, regions=2)
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="R must be"):
            replace_backend(fx.symbolic_trace(_meta(TINY)), regions=bad)
    for bad in (0, 256):
        with pytest.raises(ValueError, match="region_tokens"):
            replace_backend(fx.symbolic_trace(_meta(TINY)), regions=2, region_tokens=bad)


# ------------------------------------------------------------------------------------------------ 2. mask to weights
def test_half_masks_at_levels_0_and_1():
    m = RU.left_right_masks(4, 4)
    w0 = regions.level_weights(m, 0)
    assert w0.shape == (1, 2, 16) and w0.dtype == torch.float32
    assert w0[0, 0].tolist() == [1.0, 1.0, 0.0, 0.0] * 4 and w0[0, 1].tolist() == [0.0, 0.0, 1.0, 1.0] * 4
    w1 = regions.level_weights(m, 1)
    assert w1.shape == (1, 2, 4)
    assert w1[0, 0].tolist() == [1.0, 0.0, 1.0, 0.0] and w1[0, 1].tolist() == [0.0, 1.0, 0.0, 1.0]
    # a boundary inside a cell: columns [0, 1) against [1, 4) - the level-1 cell (row, 0) is half and half, cell (row, 1) segment 1's
    m = torch.zeros(2, 4, 4)
    m[0, :, :1] = 1.0
    m[1, :, 1:] = 1.0
    w1 = regions.level_weights(m, 1)
    assert w1[0, 0].tolist() == [0.5, 0.0, 0.5, 0.0] and w1[0, 1].tolist() == [0.5, 1.0, 0.5, 1.0]


def test_uncovered_cells_take_segment_0():
    m = RU.left_right_masks(4, 4)
    m[:, :, 3] = 0.0                                   # the last column: no mask at all
    m[:, :, 0] = 0.0                                   # the first column too
    w0 = regions.level_weights(m, 0)
    assert w0[0, 0].tolist() == [1.0, 1.0, 0.0, 1.0] * 4 and w0[0, 1].tolist() == [0.0, 0.0, 1.0, 0.0] * 4
    # level 1: cell (row, 0) holds columns 0, 1 = (nothing, segment 0) -> segment 0; cell (row, 1) columns 2, 3 = (segment 1, nothing)
    w1 = regions.level_weights(m, 1)
    assert w1[0, 0].tolist() == [1.0, 0.0, 1.0, 0.0] and w1[0, 1].tolist() == [0.0, 1.0, 0.0, 1.0]
    allzero = regions.level_weights(torch.zeros(3, 2, 2), 1)
    assert allzero[0].tolist() == [[1.0], [0.0], [0.0]]


def test_overlapping_masks_are_normalised():
    m = torch.zeros(2, 2, 2)
    m[0] = 1.0                                         # a background prompt everywhere
    m[1, :, 1] = 3.0                                   # a stronger region on the right column
    w = regions.level_weights(m, 0)
    assert w[0, 0].tolist() == [1.0, 0.25, 1.0, 0.25] and w[0, 1].tolist() == [0.0, 0.75, 0.0, 0.75]
    # level 1: the one cell holds means (1, 1.5) -> (0.4, 0.6)
    w1 = regions.level_weights(m, 1)
    assert w1[0, :, 0].tolist() == pytest.approx([0.4, 0.6], abs=1e-7)
    assert float(w.sum(dim=1).sub(1).abs().max()) <= 1e-7


def test_per_batch_masks_and_negative_rows():
    a = RU.left_right_masks(2, 2)
    b = a.flip(0)
    masks = torch.stack([a, b])                        # (batch 2, R 2, 2, 2)
    # rows [neg0, neg1 | pos0, pos1 | pert0, pert1]: the positive and the perturbed block take the masks, the negative block segment 0
    w = regions.row_weights(masks, 0, 6, range(2, 6))
    assert w.shape == (6, 2, 4)
    off = [[1.0] * 4, [0.0] * 4]
    assert w[0].tolist() == off and w[1].tolist() == off
    la, lb = [[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]], [[0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 1.0, 0.0]]
    assert w[2].tolist() == la and w[3].tolist() == lb and w[4].tolist() == la and w[5].tolist() == lb
    one = regions.row_weights(a, 0, 3, [1, 2])
    assert one[0].tolist() == off and one[1].tolist() == la and one[2].tolist() == la
    with pytest.raises(ValueError, match="positive rows"):
        regions.row_weights(masks, 0, 6, [3, 4, 5])
    with pytest.raises(ValueError, match="positive_rows"):
        regions.row_weights(a, 0, 3, [3])


@pytest.mark.parametrize("bad", [torch.full((2, 4, 4), -1.0), torch.full((2, 4, 4), float("nan")), torch.zeros(3, 4, 4),
                                 torch.zeros(4, 4), torch.zeros(2, 6, 6)])
def test_state_rejects_bad_masks(bad):
    st = regions.Regions(2, 77, levels=(1, 2))
    st.bind(2, 4, "cpu")
    with pytest.raises(ValueError):
        st.set(bad, [0, 1])
    assert st.weights_for(2, 4)[0].tolist() == [[1.0] * 4, [0.0] * 4], "a rejected set writes nothing"


def test_state_bind_set_clear_in_place():
    st = regions.Regions(2, 77, levels=(1, 2))
    with pytest.raises(ValueError, match="bind"):
        st.weights_for(2, 4)
    with pytest.raises(ValueError, match="bind"):
        st.set(RU.left_right_masks(4, 4), [1])
    st.bind(2, (4, 4), "cpu")
    b1, b2 = st.weights_for(2, 4), st.weights_for(2, 1)
    assert b1.shape == (2, 2, 4) and b2.shape == (2, 2, 1) and b1.dtype == torch.float32
    with pytest.raises(ValueError, match="bind"):
        st.weights_for(2, 16)                          # level 0 has no cross-attention in this UNet: no buffer
    st.bind(2, (4, 4), "cpu")
    assert st.weights_for(2, 4) is b1, "binding again keeps the buffers: captured graphs read them by address"
    st.set(RU.left_right_masks(4, 4), [1])
    assert st.weights_for(2, 4) is b1 and b1[1].tolist() == [[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0]]
    assert b1[0].tolist() == [[1.0] * 4, [0.0] * 4] and b2[1].tolist() == [[0.5], [0.5]]
    st.clear()
    assert b1[1].tolist() == [[1.0] * 4, [0.0] * 4] and b2[1].tolist() == [[1.0], [0.0]]
    st.bind(4, (4, 4), "cpu")                           # a second owner with another row count: its own buffers
    assert st.weights_for(2, 4) is b1 and st.bound_rows() == [2, 4]
    with pytest.raises(ValueError, match="rows="):
        st.set(RU.left_right_masks(4, 4), [1])
    with pytest.raises(ValueError, match="regions=R"):
        regions.state_of(torch.nn.Linear(2, 2), "set_regions")
    assert regions.positive_rows(6, 3) == [2, 3, 4, 5] and regions.positive_rows(4, 2) == [2, 3] and regions.positive_rows(2, 1) == [0, 1]
    with pytest.raises(ValueError, match="chunks"):
        regions.positive_rows(4, 3)


def _row_bound_states():
    from stabletriton_amd import ip_adapter, t2i_adapter
    return {"regions": lambda: regions.Regions(2, 77, levels=(1, 2)),
            "ip_adapter": lambda: ip_adapter.IPAdapter((4,), ("mid_block.attn2",), [(8, 8)], levels=(1, 2), like=torch.zeros(1)),
            "t2i_adapter": lambda: t2i_adapter.T2IAdapterState([("mid_block", 8, 2, None)])}


@pytest.mark.parametrize("name", ["regions", "ip_adapter", "t2i_adapter"])
def test_row_lookup_messages_of_the_three_row_bound_states(name):
    """`_rows(rows, what)` is one function for the three states that bind buffers per row count: the texts are the ones each state
    had of its own."""
    st = _row_bound_states()[name]()
    want = "who.set: pass rows=: this state is bound for the row counts {} (bind(rows, latent_hw, device) first)"
    with pytest.raises(ValueError) as e:
        st._rows(None, "who.set")
    assert str(e.value) == want.format([])
    st.bind(2, (4, 4), "cpu")
    assert st._rows(None, "who.set") == 2 and st._rows(2, "who.set") == 2
    st.bind(4, (4, 4), "cpu")
    with pytest.raises(ValueError) as e:
        st._rows(None, "who.set")
    assert str(e.value) == want.format([2, 4])
    with pytest.raises(ValueError) as e:
        st._rows(3, "who.set")
    assert str(e.value) == "who.set: no buffers for 3 rows (bound: [2, 4]); call bind(rows, latent_hw, device) first"
    assert st._rows(4, "who.set") == 4
    with pytest.raises(ValueError) as e:
        st.bind(0, (4, 4), "cpu")
    tail = ", feature_rows 0 (a divisor of rows)" if name == "t2i_adapter" else ""
    assert str(e.value) == f"{name}.bind: rows 0, latent 4 x 4" + tail


def test_weights_are_not_module_state():
    """The weight buffers are not registered with torch: state_dict() / buffers() of a bound compiled module (and of anything
    that holds it) work and do not list them, and a dtype cast of the module leaves them fp32 at their addresses - captured
    graphs read them in place."""
    gm = replace_backend(fx.symbolic_trace(UNet2DConditionModel(TINY).eval()), regions=2)
    gm.regions.bind(2, 16, "cpu")
    gm.regions.set(RU.left_right_masks(16, 16), [1])
    holder = torch.nn.Sequential(gm)
    for mod in (gm.regions, gm, holder):
        names = [n for n, _ in mod.named_buffers()]
        assert not any("regions" in n for n in names), names
        assert not any("regions" in k for k in mod.state_dict())
        assert len(list(mod.buffers())) == len(names)
    assert list(gm.regions.state_dict()) == [] and list(gm.regions.parameters()) == []
    w = gm.regions.weights_for(2, 64)
    ptr, before = w.data_ptr(), w.clone()
    for cast in (lambda m: m.to(torch.bfloat16), lambda m: m.half(), lambda m: m.float(), lambda m: m.to("cpu")):
        cast(holder)
        again = gm.regions.weights_for(2, 64)
        assert again is w and again.dtype == torch.float32 and again.data_ptr() == ptr and torch.equal(again, before)
    assert next(gm.parameters()).dtype == torch.float32


# ------------------------------------------------------------------------------------------------ 3. the plain torch statement
def test_reference_against_the_float64_restatement():
    B, T, H, D, R, L = 2, 24, 2, 16, 3, 7
    C = H * D
    q = synth.normal("regions.host.q", (B, T, C), 5)
    k = synth.normal("regions.host.k", (B, R * L, C), 6) * 1.5
    v = synth.normal("regions.host.v", (B, R * L, C), 7)
    w = torch.rand((B, R, T), generator=torch.Generator().manual_seed(3)) * 1.7 - 0.3          # un-normalised, some negative
    scale = D ** -0.5
    want = RU.regions64(q, k, v, w, H, scale, L)
    got = regions.reference(q, k, v, w, H, scale, L)
    assert got.dtype == torch.float32
    mag = sum(w[:, r].abs().double().unsqueeze(-1) * RU.attention64(q, k[:, r * L:(r + 1) * L], v[:, r * L:(r + 1) * L], H, scale).abs()
              for r in range(R))
    # fp32 arithmetic throughout: dot products of D and L terms, a softmax, R multiply-adds - 64 ulp of the terms' size is generous
    assert float(((got.double() - want).abs() - 64 * 2.0 ** -24 * (mag + 1e-3)).max()) <= 0.0
    assert float((regions.reference(q.double(), k.double(), v.double(), w, H, scale, L) - want).abs().max()) < 1e-13
    for r in range(R):
        onehot = torch.zeros((B, R, T))
        onehot[:, r] = 1.0
        seg = slice(r * L, (r + 1) * L)
        plain = pag.identity_attention_reference(q, k[:, seg], v[:, seg], H, scale, 0)
        assert torch.equal(regions.reference(q, k, v, onehot, H, scale, L), plain), f"one-hot on segment {r} is plain attention on it"
    with pytest.raises(ValueError, match="seg_len"):
        regions.reference(q, k, v, w, H, scale, L + 1)


# ------------------------------------------------------------------------------------------------ 4. TINY on the CPU
def _tiny():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def _traced(m, R=None):
    return RU.traced_cpu(m, R)


def _call(mod, x, ehs):
    with torch.no_grad():
        return mod(x["latent"], torch.tensor(500.0), ehs, {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


def test_traced_cpu_module_off_is_the_plain_module_and_masks_mix_the_prompts():
    m = _tiny()
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    both = RU.two_prompts(2, 77, TINY.cross_dim)
    first, second = both[:, :77].contiguous(), both[:, 77:].contiguous()
    plain, _ = _traced(m)
    gm, sites = _traced(m, 2)
    assert sites == 17
    with pytest.raises(ValueError, match="bind"):
        _call(gm, x, both)
    gm.regions.bind(2, 16, "cpu")
    with pytest.raises(ValueError, match="154 tokens"):
        _call(gm, x, first)
    a, b = _call(plain, x, first), _call(plain, x, second)
    off = _call(gm, x, both)
    assert torch.equal(off, a), "off: segment 0's prompt alone, the bits of the module without the pass"
    gm.regions.set(RU.left_right_masks(16, 16), [0, 1])
    mixed = _call(gm, x, both)
    da, db = float((mixed - a).abs().max()), float((mixed - b).abs().max())
    print(f"traced TINY, left / right prompts: max abs distance to the first prompt's output {da:.3e}, to the second's {db:.3e}; "
          f"the two prompts' outputs are {float((a - b).abs().max()):.3e} apart")
    assert da > 1e-3 and db > 1e-3 and torch.isfinite(mixed).all()
    gm.regions.set(torch.stack([torch.zeros(16, 16), torch.ones(16, 16)]), [0, 1])
    only_b = _call(gm, x, both)
    assert torch.equal(only_b, b), "weight 1 on segment 1 everywhere: the second prompt alone"
    gm.regions.clear()
    assert torch.equal(_call(gm, x, both), a)


# ------------------------------------------------------------------------------------------------ 5. DenoiseLoop (CPU tensors)
class _NoUNet:
    """Stands in for a compiled UNet: the host-side paths below never evaluate it."""

    def __init__(self, R=2, seg_len=3):
        self.pag = pag.PAG()
        if R:
            self.regions = regions.Regions(R, seg_len, levels=(1, 2))


def _loop(unet, tokens, **kw):
    from stabletriton_amd.pipeline import DenoiseLoop
    from stabletriton_amd.scheduler import euler_discrete_tables
    return DenoiseLoop(unet, 2, 16, torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8, pooled_dim=6, tokens=tokens, **kw)


def test_loop_binds_tiles_the_negative_and_sets_in_place():
    with pytest.raises(ValueError, match="tokens=6"):
        _loop(_NoUNet(), 3)
    unet = _NoUNet()
    lp = _loop(unet, 6, guidance_scale=5.0, pag_scale=3.0)
    st = unet.regions
    assert st.bound_rows() == [6] and st.weights_for(6, 64).shape == (6, 2, 64) and st.weights_for(6, 16).shape == (6, 2, 16)
    pos = (torch.randn(2, 6, 8), torch.randn(2, 6), torch.randn(2, 6))
    neg = torch.randn(2, 3, 8)
    lp.set_conditioning(*pos, negative_encoder_hidden_states=neg)
    assert torch.equal(lp.ehs[:2, :3], neg) and torch.equal(lp.ehs[:2, 3:], neg), "one negative prompt: tiled into every segment"
    assert torch.equal(lp.ehs[2:4], pos[0]) and torch.equal(lp.ehs[4:], pos[0])
    full = torch.randn(2, 6, 8)
    lp.set_conditioning(*pos, negative_encoder_hidden_states=full)
    assert torch.equal(lp.ehs[:2], full)
    lp.set_conditioning(*pos)
    assert not lp.ehs[:2].any()
    buf = st.weights_for(6, 64)
    lp.set_regions(RU.left_right_masks(16, 16))
    assert st.weights_for(6, 64) is buf
    off = [[1.0] * 64, [0.0] * 64]
    left = [1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0] * 8
    assert buf[0].tolist() == off and buf[1].tolist() == off, "the negative block keeps segment 0"
    for r in range(2, 6):
        assert buf[r, 0].tolist() == left and buf[r, 1].tolist() == [1.0 - v for v in left]
    per_sample = torch.stack([RU.left_right_masks(16, 16), RU.left_right_masks(16, 16).flip(0)])
    lp.set_regions(per_sample)
    assert buf[2, 0].tolist() == left and buf[3, 1].tolist() == left and buf[4, 0].tolist() == left and buf[5, 1].tolist() == left
    lp.set_regions(None)
    assert all(buf[r].tolist() == off for r in range(6))
    for bad in (torch.zeros(2, 8, 8), torch.zeros(3, 16, 16), torch.zeros(3, 2, 16, 16)):
        with pytest.raises(ValueError, match="set_regions|masks"):
            lp.set_regions(bad)
    unguided = _loop(unet, 6)
    unguided.set_regions(RU.left_right_masks(16, 16))
    assert st.bound_rows() == [2, 6] and st.weights_for(2, 64)[0, 0].tolist() == left, "without guidance every row is positive"
    with pytest.raises(ValueError, match="regions=R"):
        _loop(_NoUNet(R=0), 3).set_regions(None)


# ------------------------------------------------------------------------------------------------ 6. the C entry point
P = 1 << 20            # fake, aligned, never dereferenced device addresses: validation happens before any launch


def test_entry_point_is_exported_bound_and_validates_on_the_host(lib):
    from stabletriton_amd import _C
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    assert "st_attention_regions" in _C.SIGNATURES and hasattr(lib, "st_attention_regions")

    def call(**kw):
        a = dict(q=P, k=P, v=P, w=P, out=P, B=2, T=96, R=2, L=77, H=2, D=64, ldq=128, ldk=256, ldv=256, ldo=128, dtype=_C.ST_BF16)
        a.update(kw)
        return lib.st_attention_regions(a["q"], a["k"], a["v"], a["w"], a["out"], a["B"], a["T"], a["R"], a["L"], a["H"], a["D"],
                                        a["ldq"], a["ldk"], a["ldv"], a["ldo"], 0.125, a["dtype"], None)

    for kw, word in ((dict(dtype=_C.ST_F32), b"dtype"), (dict(D=32, ldq=64, ldo=64), b"head_dim"), (dict(R=9), b"R 9"), (dict(R=0), b"R 0"),
                     (dict(L=256), b"seg_len 256"), (dict(L=0), b"seg_len 0"), (dict(w=None), b"weights"), (dict(q=None), b"q is null"),
                     (dict(k=P + 2), b"k must be 16-byte"), (dict(out=P + 8), b"out must be 16-byte"), (dict(ldv=260), b"ldv 260"),
                     (dict(ldq=132), b"ldq 132"), (dict(ldo=130), b"ldo 130"), (dict(ldk=64), b"ldk 64"), (dict(w=P + 2), b"weights")):
        assert call(**kw) != 0, kw
        assert word in lib.st_last_error(), (kw, lib.st_last_error())
