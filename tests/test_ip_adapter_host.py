"""IP-Adapter, everything that runs without a GPU: the pass on the graph, the checkpoint layouts and the numbered-key order, the
image projection, mask level weights, scale resolution, a traced CPU module with the pass against the tests' own float64
restatement of one site, and the C entry point's export and host-side validation."""
import ctypes

import pytest
import torch
from torch import fx

from stabletriton_amd import ip_adapter, pag, synth
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.optimizers.wrappers import attention_wrapper, ln_linear_attention_wrapper, ln_linear_wrapper
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel, UNetWithLabelVector
from tests import ip_adapter_util as IU


def _meta(spec, wrap=False):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec).eval()
        return UNetWithLabelVector(m) if wrap else m


def _targets(gm, target):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is target]


# ------------------------------------------------------------------------------------------------ 1. the pass
@pytest.mark.parametrize("spec,want", [(TINY, 17), (SDXL_BASE, 70)])
def test_site_counts_and_lost_fusion(spec, want):
    plain = replace_backend(fx.symbolic_trace(_meta(spec)))
    gm = replace_backend(fx.symbolic_trace(_meta(spec)), ip_adapter=4)
    leaves = _targets(gm, ip_adapter.attention_ip_wrapper)
    assert gm.rewrite_stats["ip_adapter_sites"] == want == len(leaves)
    st = gm.ip_adapter
    assert isinstance(st, ip_adapter.IPAdapter) and st.tokens == (4,) and len(st.sites) == want == len(st.dims)
    assert all(s.endswith(".attn2") for s in st.sites) and st.levels == (1, 2)
    assert all(x == spec.cross_dim and c % spec.head_dim == 0 for c, x in st.dims)
    assert [n.args[-1] for n in leaves] == list(range(want)), "every site carries its own index, in graph order"
    assert not _targets(gm, ln_linear_attention_wrapper) and gm.rewrite_stats["query_projection_in_attention"] == 0
    for n in leaves:
        assert n.args[0].target is ln_linear_wrapper, "the query projection still folds its LayerNorm"
    assert len(_targets(gm, attention_wrapper)) == len(_targets(plain, attention_wrapper)) > 0
    other = {k: v for k, v in gm.rewrite_stats.items() if k not in ("ip_adapter_sites", "query_projection_in_attention")}
    assert other == {k: v for k, v in plain.rewrite_stats.items() if k != "query_projection_in_attention"}


def test_prefix_and_token_tuples():
    gm = replace_backend(fx.symbolic_trace(_meta(TINY, wrap=True)), ip_adapter=(16, 4))
    assert gm.rewrite_stats["ip_adapter_sites"] == 17 and gm.ip_adapter.tokens == (16, 4) and gm.ip_adapter.slots == 2


@pytest.mark.parametrize("spec", [SDXL_BASE, TINY])
def test_default_graph_is_unchanged(spec):
    a = replace_backend(fx.symbolic_trace(_meta(spec)))
    b = replace_backend(fx.symbolic_trace(_meta(spec)), ip_adapter=None)
    assert a.code == b.code and "ip_adapter" not in a.code and not hasattr(a, "ip_adapter")
    assert list(a.rewrite_stats.items()) == list(b.rewrite_stats.items()) and "ip_adapter_sites" not in a.rewrite_stats


def test_bad_compile_arguments_raise():
    with pytest.raises(ValueError, match="ip_adapter=N cannot be combined with fp8"):
        replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True, ip_adapter=4)
    with pytest.raises(ValueError, match="ip_adapter=N cannot be combined with regions"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), regions=2, ip_adapter=4)
    for bad in (0, 256, 2.0, True, (), (4, 4, 4, 4, 4), (4, 0)):
        with pytest.raises(ValueError, match="token count"):
            replace_backend(fx.symbolic_trace(_meta(TINY)), ip_adapter=bad)


# ------------------------------------------------------------------------------------------------ 2. TINY on the CPU: loading
def _tiny():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


@pytest.fixture(scope="module")
def cpu_pair():
    m = _tiny()
    plain, _ = IU.traced_cpu(m)
    gm, sites = IU.traced_cpu(m, (4, 16))
    assert sites == 17
    return m, plain, gm


def _stacked(st, slot):
    return [st._ip_weights[(i, slot)].clone() for i in range(len(st.sites))]


@pytest.mark.parametrize("layout", ["published", "flat", "processor", "path"])
def test_checkpoint_layouts(cpu_pair, layout):
    st = cpu_pair[2].ip_adapter
    sd, by_path = IU.checkpoint(st, 4, layout=layout, slot=0)
    proj = st.load(sd, 0)
    assert (proj is not None and "proj.weight" in proj) == (layout in ("published", "flat"))
    for i, path in enumerate(st.sites):
        c = st.dims[i][0]
        w = st._ip_weights[(i, 0)]
        assert torch.equal(w[:c], by_path[path][0]) and torch.equal(w[c:], by_path[path][1]), path
    st.unload(0)
    assert all(float(w.abs().max()) == 0.0 for w in _stacked(st, 0))
    # a multi-adapter processor state dict: slot 1 takes the keys spelled .1.
    sd1, by1 = IU.checkpoint(st, 16, seed=9, layout="processor", slot=1)
    merged = dict(IU.checkpoint(st, 4, layout="processor", slot=0)[0])
    merged.update(sd1)
    st.load(merged, 1)
    assert torch.equal(st._ip_weights[(0, 1)][:st.dims[0][0]], by1[st.sites[0]][0])
    assert all(float(w.abs().max()) == 0.0 for w in _stacked(st, 0)), "slot 0 was not touched"
    st.unload(1)


def test_numbered_keys_follow_the_attn_processors_order(cpu_pair):
    """down_blocks, then up_blocks, then mid_block (restated from the published loaders; parity with real checkpoints unpinned):
    on TINY 6 down sites, 9 up sites, 2 mid sites, while the module (graph) order is down, mid, up."""
    st = cpu_pair[2].ip_adapter
    sites = st.sites
    assert [s.split(".")[0] for s in sites] == ["down_blocks"] * 6 + ["mid_block"] * 2 + ["up_blocks"] * 9
    order = ip_adapter.diffusers_order(sites)
    assert order == list(range(6)) + list(range(8, 17)) + [6, 7]
    numbered = {}
    for n in range(17):
        i = order[n]
        c, x = st.dims[i]
        numbered[f"{2 * n + 1}.to_k_ip.weight"] = torch.full((c, x), float(2 * n + 1))
        numbered[f"{2 * n + 1}.to_v_ip.weight"] = torch.full((c, x), -float(2 * n + 1))
    st.load({"ip_adapter": numbered, "image_proj": {}}, 0)
    first = lambda i: float(st._ip_weights[(i, 0)][0, 0])
    assert first(0) == 1.0 and sites[0].startswith("down_blocks.1.attentions.0"), "key 1 lands on the first down_blocks site"
    assert first(5) == 11.0 and first(8) == 13.0 and sites[8].startswith("up_blocks.0"), "the first up key follows the last down key"
    assert first(6) == 31.0 and first(7) == 33.0, "the mid keys come last"
    assert float(st._ip_weights[(7, 0)][-1, 0]) == -33.0, "to_v_ip is the lower half of the stacked weight"
    st.unload(0)


def test_shape_and_site_count_errors_write_nothing(cpu_pair):
    st = cpu_pair[2].ip_adapter
    good, _ = IU.checkpoint(st, 4, seed=3)
    st.load(good, 0)
    before = _stacked(st, 0)
    bad_shape = {"ip_adapter": dict(good["ip_adapter"]), "image_proj": {}}
    bad_shape["ip_adapter"]["33.to_v_ip.weight"] = torch.zeros(7, 7)          # the LAST key: everything before it validated
    with pytest.raises(ValueError, match=r"\(C_site, cross_dim\)"):
        st.load(bad_shape, 0)
    fewer = {"ip_adapter": {k: v for k, v in good["ip_adapter"].items() if not k.startswith("33.")}}
    with pytest.raises(ValueError, match="17 sites"):
        st.load(fewer, 0)
    more = {"ip_adapter": dict(good["ip_adapter"])}
    more["ip_adapter"]["35.to_k_ip.weight"] = more["ip_adapter"]["35.to_v_ip.weight"] = torch.zeros(256, 128)
    with pytest.raises(ValueError, match="17 sites"):
        st.load(more, 0)
    with pytest.raises(ValueError, match="names no cross-attention site"):
        st.load({"nowhere.attn2.to_k_ip.weight": torch.zeros(128, 128)}, 0)
    with pytest.raises(ValueError, match="needs 34"):
        st.load({f"{st.sites[0]}.to_k_ip.weight": torch.zeros(st.dims[0])}, 0)
    with pytest.raises(ValueError, match="slot"):
        st.load(good, 2)
    assert all(torch.equal(a, b) for a, b in zip(before, _stacked(st, 0))), "a rejected checkpoint writes nothing"
    st.unload(0)


def test_project_image_embeds_against_a_hand_formula(cpu_pair):
    st = cpu_pair[2].ip_adapter
    sd, _ = IU.checkpoint(st, 4, emb_dim=32)
    proj = sd["image_proj"]
    e = synth.normal("ip.embeds", (3, 32), 17)
    got = ip_adapter.project_image_embeds(proj, e)
    assert got.shape == (3, 4, TINY.cross_dim) and got.dtype == torch.float32
    y = (e.double() @ proj["proj.weight"].double().T + proj["proj.bias"].double()).reshape(3, 4, TINY.cross_dim)
    mean = y.mean(dim=-1, keepdim=True)
    var = ((y - mean) ** 2).mean(dim=-1, keepdim=True)
    want = (y - mean) / torch.sqrt(var + 1e-5) * proj["norm.weight"].double() + proj["norm.bias"].double()
    assert float((got.double() - want).abs().max()) < 1e-5
    with pytest.raises(ValueError, match="Resampler"):
        ip_adapter.project_image_embeds({"latents": torch.zeros(1, 16, 8)}, e)
    with pytest.raises(ValueError, match="image_embeds"):
        ip_adapter.project_image_embeds(proj, torch.zeros(3, 31))


# ------------------------------------------------------------------------------------------------ 3. masks and scales
def test_mask_level_weights():
    m = torch.zeros(8, 8)
    m[:, :3] = 2.0                                   # columns 0..2: not aligned to the 2 x 2 and 4 x 4 cells
    w0, w1, w2 = (ip_adapter.mask_level_weights(m, l) for l in range(3))
    assert w0.shape == (1, 64) and torch.equal(w0.view(8, 8), m)
    assert torch.equal(w1.view(4, 4)[0], torch.tensor([2.0, 1.0, 0.0, 0.0])), "area mean, NOT normalised"
    assert torch.equal(w2.view(2, 2), torch.tensor([[1.5, 0.0], [1.5, 0.0]]))
    batched = ip_adapter.mask_level_weights(torch.stack([m, m.flip(1)]), 1)
    assert batched.shape == (2, 16) and torch.equal(batched[1].view(4, 4)[0], torch.tensor([0.0, 0.0, 1.0, 2.0]))
    for bad in (torch.full((8, 8), -1.0), torch.full((8, 8), float("nan")), torch.zeros(2, 2, 8, 8)):
        with pytest.raises(ValueError, match="masks"):
            ip_adapter.mask_level_weights(bad, 0)
    with pytest.raises(ValueError, match="divide"):
        ip_adapter.mask_level_weights(torch.zeros(6, 6), 2)


def test_set_masks_writes_every_row_in_place(cpu_pair):
    st = cpu_pair[2].ip_adapter
    st.bind(4, 16, "cpu")
    w64, w16 = st.weights_for(4, 64), st.weights_for(4, 16)
    assert w64.shape == (4, 3, 64) and float(w64.min()) == 1.0 == float(w16.max()) and w64.dtype == torch.float32
    ptr = w64.data_ptr()
    left = torch.zeros(16, 16)
    left[:, :8] = 1.0
    st.set_masks(torch.stack([left, left.flip(1)]), 1, 4)
    assert st.weights_for(4, 64).data_ptr() == ptr
    assert float(w64[:, 0].min()) == 1.0 == float(w64[:, 1].min()), "the text column and the other slot stay 1"
    assert torch.equal(w64[0, 2].view(8, 8)[0], torch.tensor([1.0] * 4 + [0.0] * 4)) and torch.equal(w64[0, 2], w64[2, 2])
    assert torch.equal(w64[1, 2], w64[0, 2].view(8, 8).flip(1).reshape(-1)) and torch.equal(w64[1, 2], w64[3, 2]), "row r takes mask r % batch"
    with pytest.raises(ValueError, match="latent size"):
        st.set_masks(torch.ones(8, 8), 1, 4)
    with pytest.raises(ValueError, match="rows"):
        st.set_masks(left, 1, 6)
    st.set_masks(None, 1, 4)
    assert float(w64.min()) == 1.0 == float(w16.min())
    assert "ip_adapter" not in "".join(cpu_pair[2].state_dict().keys()), "the buffers are not module state"


def test_scale_resolution(cpu_pair):
    st = cpu_pair[2].ip_adapter
    sc = st.scales
    assert sc.shape == (17, 3) and sc.dtype == torch.float32 and float(sc[:, 0].min()) == 1.0 and float(sc[:, 1:].abs().max()) == 0.0
    ptr = sc.data_ptr()
    st.set_scale(0.6, 0)
    assert torch.equal(sc[:, 1], torch.full((17,), 0.6)) and float(sc[:, 2].abs().max()) == 0.0 and float(sc[:, 0].min()) == 1.0
    st.set_scale({"mid": 1.0}, 0)
    assert sc[:, 1].tolist() == [0.0] * 6 + [1.0] * 2 + [0.0] * 9, '"mid" selects the middle block; unmatched sites get 0'
    st.set_scale({r"up_blocks\.0": 0.25, "up_blocks": 0.5, r"down_blocks\.2\..*transformer_blocks\.1": -1.0}, 1)
    assert sc[:, 2].tolist() == [0.0, 0.0, 0.0, -1.0, 0.0, -1.0, 0.0, 0.0] + [0.25] * 6 + [0.5] * 3, "the first match wins"
    assert sc[:, 1].tolist() == [0.0] * 6 + [1.0] * 2 + [0.0] * 9, "the other slot's column stays"
    st.set_scale({".*": 0}, 0)
    st.set_scale(0, 1)
    assert float(sc[:, 1:].abs().max()) == 0.0 and st.scales.data_ptr() == ptr
    for bad in (float("nan"), {"mid": float("inf")}, True):
        with pytest.raises(ValueError, match="scale"):
            st.set_scale(bad, 0)
    with pytest.raises(ValueError, match="slot"):
        st.set_scale(1.0, 2)


# ------------------------------------------------------------------------------------------------ 4. the formula
def test_reference_against_the_float64_restatement():
    B, T, H, D = 2, 24, 2, 16
    C = H * D
    q = synth.normal("ip.host.q", (B, T, C), 5)
    segs = [(synth.normal(f"ip.host.k{r}", (B, n, C), 6 + r) * 1.5, synth.normal(f"ip.host.v{r}", (B, n, C), 16 + r)) for r, n in enumerate((9, 4, 1))]
    w = torch.rand((B, 3, T), generator=torch.Generator().manual_seed(3)) * 1.7 - 0.3
    sc = torch.tensor([1.0, 0.6, -1.5])
    sm = D ** -0.5
    want = IU.segments64(q, segs, w, sc, H, sm)
    got = ip_adapter.reference(q, segs, w, sc, H, sm)
    # fp32 arithmetic throughout: dot products of D and len terms, a softmax, S multiply-adds.  Every rounding is relative to the
    # TERMS of the sums, so the size the error scales with is sum_r |w_eff| sum_s p |v| (no cancellation inside a segment's P V),
    # not |result|; 64 ulp of that is generous for at most 16 + 9 + 3 operations per value
    mag = sum(IU.effective_weights(w, sc)[:, r].abs().double().unsqueeze(-1) * IU.attention64(q, k, v.abs(), H, sm) for r, (k, v) in enumerate(segs))
    assert got.dtype == torch.float32
    assert float(((got.double() - want).abs() - 64 * 2.0 ** -24 * (mag + 1e-3)).max()) <= 0.0
    one = torch.ones((B, 3, T))
    assert torch.equal(ip_adapter.reference(q, segs, one, torch.tensor([1.0, 0.0, 0.0]), H, sm),
                       pag.identity_attention_reference(q, segs[0][0], segs[0][1], H, sm, 0)), "image scales 0: the text attention's bits"


def _call(mod, x, ehs):
    with torch.no_grad():
        return mod(x["latent"], torch.tensor(500.0), ehs, {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


def test_traced_cpu_module_against_the_float64_restatement_of_one_site(cpu_pair):
    m, plain, gm = cpu_pair
    st = gm.ip_adapter
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    ehs = x["encoder_hidden_states"]
    fresh, _ = IU.traced_cpu(m, 4)
    with pytest.raises(ValueError, match="bind"):
        _call(fresh, x, ehs)
    st.bind(2, 16, "cpu")
    base = _call(plain, x, ehs)
    assert torch.equal(_call(gm, x, ehs), base), "nothing loaded: the bits of the module without the pass"
    sd, by_path = IU.checkpoint(st, 4)
    st.load(sd, 0)
    tok = IU.image_tokens(2, 4, TINY.cross_dim)
    st.set_image(tok, None, 0, 2)
    assert torch.equal(_call(gm, x, ehs), base), "loaded, image set, scale 0: still those bits"
    # one site, restated: capture its inputs and output through a hook on the leaf's module-level name
    seen = {}
    real = ip_adapter.attention_ip_wrapper

    def spy(q, k, v, output, sm, heads, head_dim, state, site):
        out = real(q, k, v, output, sm, heads, head_dim, state, site)
        if site == 7:
            seen.update(q=q, k=k, v=v, sm=sm, heads=heads, out=out)
        return out

    left = torch.zeros(16, 16)
    left[:, :8] = 1.0
    st.set_scale({"mid": 0.7, "down": 0.3}, 0)
    st.set_masks(left, 0, 2)
    spied = fx.GraphModule(gm, gm.graph)
    for n in spied.graph.nodes:
        if n.op == "call_function" and n.target is real:
            n.target = spy
    spied.recompile()
    on = _call(spied, x, ehs)
    assert float((on - base).abs().max()) > 1e-3 and torch.isfinite(on).all()
    site = 7                                           # mid_block, the second layer: 16 queries, C = 256
    assert st.sites[site].startswith("mid_block") and seen["q"].shape == (2, 16, 256)
    wk, wv = by_path[st.sites[site]]
    segs = [(seen["k"], seen["v"]), (tok @ wk.T, tok @ wv.T), (torch.zeros(2, 16, 256), torch.zeros(2, 16, 256))]
    w = torch.ones(2, 3, 16)
    w[:, 1] = ip_adapter.mask_level_weights(left, 2)
    want = IU.segments64(seen["q"], segs, w, [1.0, 0.7, 0.0], seen["heads"], seen["sm"])
    assert float((seen["out"].double() - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max()))
    assert torch.equal(st.kv_for(2, site, 0)[..., :256], torch.nn.functional.linear(tok, wk))
    st.unload(0)
    assert torch.equal(_call(gm, x, ehs), base), "unload restores the bits of off"
    with pytest.raises(ValueError, match=r"\(B or 1, N, cross_dim\)"):
        st.set_image(IU.image_tokens(2, 16, TINY.cross_dim), None, 0, 2)
    with pytest.raises(ValueError, match="negative row block"):
        st.set_image(tok, tok, 0, 2)


# ------------------------------------------------------------------------------------------------ 5. DenoiseLoop (host side)
class _NoUNet:
    def __init__(self):
        self.pag = pag.PAG()


def test_loop_without_the_pass_names_the_compile_argument():
    from stabletriton_amd.pipeline import DenoiseLoop
    from stabletriton_amd.scheduler import euler_discrete_tables
    loop = DenoiseLoop(_NoUNet(), 2, 16, torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8, pooled_dim=6, tokens=3)
    for call in (lambda: loop.load_ip_adapter({}), lambda: loop.set_ip_adapter_image(torch.zeros(1, 4, 8)), lambda: loop.set_ip_adapter_scale(1.0),
                 lambda: loop.set_ip_adapter_masks(None), lambda: loop.unload_ip_adapter()):
        with pytest.raises(ValueError, match="ip_adapter=N"):
            call()


# ------------------------------------------------------------------------------------------------ 6. the C entry point
P = 1 << 20            # fake, aligned, never dereferenced device addresses: validation happens before any launch


def test_entry_point_is_exported_bound_and_validates_on_the_host(lib):
    from stabletriton_amd import _C
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    assert "st_attention_segments" in _C.SIGNATURES and hasattr(lib, "st_attention_segments")
    assert ctypes.sizeof(_C.KVSegment) == 56

    def call(segs=None, **kw):
        a = dict(q=P, w=P, sc=P, out=P, B=2, T=96, H=2, D=64, ldq=128, ldo=128, dtype=_C.ST_BF16)
        a.update(kw)
        segs = [dict(), dict(len=4)] if segs is None else segs
        table = (_C.KVSegment * max(len(segs), 1))()
        for r, s in enumerate(segs):
            d = dict(k=P, v=P, ldk=256, ldv=256, bsk=77 * 256, bsv=77 * 256, len=77)
            d.update(s)
            table[r] = _C.KVSegment(d["k"], d["v"], d["ldk"], d["ldv"], d["bsk"], d["bsv"], d["len"])
        return lib.st_attention_segments(a["q"], table if a.get("table", True) else None, a.get("S", len(segs)), a["w"], a["sc"], a["out"],
                                         a["B"], a["T"], a["H"], a["D"], a["ldq"], a["ldo"], 0.125, a["dtype"], None)

    for kw, word in ((dict(dtype=_C.ST_F32), b"dtype"), (dict(D=32, ldq=64, ldo=64), b"head_dim"), (dict(S=9), b"S 9"), (dict(S=0), b"S 0"),
                     (dict(w=None), b"weights is null"), (dict(q=None), b"q is null"), (dict(table=False), b"segs is null"),
                     (dict(out=P + 8), b"out must be 16-byte"), (dict(ldq=132), b"ldq 132"), (dict(ldo=130), b"ldo 130"),
                     (dict(w=P + 2), b"weights must be 4-byte"), (dict(sc=P + 2), b"seg_scale must be 4-byte"),
                     (dict(segs=[dict(), dict(len=256)]), b"segment 1: len 256"), (dict(segs=[dict(len=0)]), b"segment 0: len 0"),
                     (dict(segs=[dict(), dict(k=None)]), b"segment 1: k is null"), (dict(segs=[dict(v=P + 2)]), b"segment 0: v must be 16-byte"),
                     (dict(segs=[dict(), dict(), dict(ldk=260)]), b"segment 2: ldk 260"), (dict(segs=[dict(ldv=64)]), b"segment 0: ldv 64"),
                     (dict(segs=[dict(), dict(bsk=12)]), b"segment 1: bsk 12"), (dict(segs=[dict(bsv=-8)]), b"segment 0: bsv -8")):
        assert call(**kw) != 0, kw
        assert word in lib.st_last_error(), (kw, lib.st_last_error())
