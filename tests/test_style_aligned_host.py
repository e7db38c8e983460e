"""StyleAligned on the host: the fx pass's site selection and flag conflicts, a traced CPU TINY module carrying the pass against a
hand-written float64 statement of "AdaIN then shared attention" hooked onto one site of the eager module, the loop's refusals and gate
table on CPU tensors, and the C entry points' presence.  No GPU."""
import pytest
import torch
from torch import fx

from stabletriton_amd import style_aligned, synth
from stabletriton_amd.optimization import check_feature_combination, replace_backend
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel


def _meta(spec):
    with torch.device("meta"):
        return UNet2DConditionModel(spec).eval()


@pytest.mark.parametrize("spec,layers,want", [(TINY, (".*",), 17), (TINY, ("mid",), 2), (TINY, ("down_blocks.2", "mid"), 6), (SDXL_BASE, ".*", 70)])
def test_site_counts_and_widths(spec, layers, want):
    gm = replace_backend(fx.symbolic_trace(_meta(spec)), style_aligned_layers=layers)
    nodes = [n for n in gm.graph.nodes if n.op == "call_function" and n.target is style_aligned.attention_style_wrapper]
    state = gm.style_aligned
    assert gm.rewrite_stats["style_aligned_sites"] == want == len(nodes) == len(state.sites) == len(state.channels)
    assert isinstance(state, style_aligned.StyleAligned) and state.per == 0 and state.adain == "qk"
    assert all(s.endswith(".attn1") for s in state.sites) and all(c % 64 == 0 for c in state.channels)


@pytest.mark.parametrize("layers", [("nowhere",), (".*", "nowhere"), ("attn2",), ()])
def test_patterns_that_select_no_self_attention_raise(layers):
    with pytest.raises(ValueError, match="style_aligned_layers"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), style_aligned_layers=layers)


@pytest.mark.parametrize("other", ["pag_layers", "seg_layers", "reference_layers", "hypertile_layers"])
def test_flag_conflicts_raise_before_the_trace(other):
    with pytest.raises(ValueError, match="style_aligned_layers cannot be combined"):
        replace_backend(torch.nn.Identity(), style_aligned_layers=(".*",), **{other: ("mid",)})
    check_feature_combination(False, None, None, None, None, False, False, None, None, (".*",))


SITE = "mid_block.attentions.0.transformer_blocks.0.attn1"


def _statement64(attn, x, per, adain):
    """attn1(x) for a (B, T, C) input in float64, written out: projections, AdaIN of q and k (and v) along the tokens, attention over
    [own keys | style row's keys] for every row that is not the first of its block."""
    B, T, C = x.shape
    H = attn.num_heads
    w = lambda lin: lin.weight.double()
    q, k, v = x.double() @ w(attn.to_q).T, x.double() @ w(attn.to_k).T, x.double() @ w(attn.to_v).T
    out = torch.empty_like(q)
    for b in range(B):
        s = b - b % per
        qb, kb, vb = q[b], k[b], v[b]
        if b != s:
            norm = lambda t, ts: (t - t.mean(0)) / (t.var(0, unbiased=True) + 1e-5).sqrt() * (ts.var(0, unbiased=True) + 1e-5).sqrt() + ts.mean(0)
            qb, kb = norm(q[b], q[s]), norm(k[b], k[s])
            vb = norm(v[b], v[s]) if adain == "qkv" else vb
            kb, vb = torch.cat([kb, k[s]]), torch.cat([vb, v[s]])
        heads = lambda t: t.reshape(t.shape[0], H, C // H).transpose(0, 1)
        p = torch.softmax(heads(qb) @ heads(kb).transpose(1, 2) * (C // H) ** -0.5, dim=-1)
        out[b] = (p @ heads(vb)).transpose(0, 1).reshape(T, C)
    return (out @ w(attn.to_out[0]).T + attn.to_out[0].bias.double()).to(x.dtype)


@pytest.mark.parametrize("per,adain", [(3, "qk"), (2, "qkv"), (6, "qk")])
def test_traced_cpu_module_with_the_pass_equals_the_float64_statement_on_one_site(per, adain):
    from stabletriton_amd.optimizers import fuse_attention, insert_style_aligned
    from stabletriton_amd.optimizers.wrappers import attention_wrapper
    from stabletriton_amd.pag import identity_attention_reference
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    x = synth.denoise_inputs(6, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    call = lambda mod: mod(x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]
    gm = fx.symbolic_trace(m)
    fuse_attention(gm)
    assert insert_style_aligned(gm, (SITE.replace(".", r"\.") + "$",)) == 1
    for n in list(gm.graph.nodes):                           # the unselected attention_wrapper leaves have no CPU route: eager ones
        if n.op == "call_function" and n.target is attention_wrapper:
            with gm.graph.inserting_before(n):
                new = gm.graph.call_function(identity_attention_reference, (n.args[0], n.args[1], n.args[2], n.args[5], n.args[4], 0))
            n.replace_all_uses_with(new)
            gm.graph.erase_node(n)
    gm.recompile()
    gm.style_aligned.set_adain(adain)
    attn = m.get_submodule(SITE)
    with torch.no_grad():
        plain = call(m)
        attn.forward = lambda x_, context=None: _statement64(attn, x_, per, adain)
        want = call(m)
        del attn.forward
        with gm.style_aligned.using(per):
            got = call(gm)
        off = call(gm)
        step, table = torch.zeros(1, dtype=torch.int32), torch.tensor([0.0, 1.0])
        with gm.style_aligned.using(per, step=step, table=table):
            gated_off = call(gm)
            step.fill_(1)
            gated_on = call(gm)
    assert gm.style_aligned.per == 0 and gm.style_aligned.gate is None, "the context manager restores the previous values"
    bound = 2e-5 * float(plain.abs().max())                  # fp32 rounding: a few 100 ulp of the output's size (tests/test_reference_host.py)
    moved = float((want - plain).abs().max())
    assert moved > 100 * bound, "the feature must matter for this check to mean anything"
    style = torch.arange(6) % per == 0
    assert float((want[style] - plain[style]).abs().max()) < bound, "style rows do not depend on the others"
    assert float((got - want).abs().max()) < bound
    assert float((off - plain).abs().max()) < bound and torch.equal(gated_off, off) and torch.equal(gated_on, got)


def test_loop_refusals():
    from types import SimpleNamespace
    from stabletriton_amd import controlnet, ip_adapter, pag, reference, regions, seg, t2i_adapter
    from stabletriton_amd.pipeline import DenoiseLoop
    from stabletriton_amd.scheduler import euler_discrete_tables

    def loop(states=None, batch=2, **kw):      # (the refusals precede any use of the UNet: a namespace that carries the states stands in)
        unet = SimpleNamespace(style_aligned=style_aligned.StyleAligned(), **(states or {}))
        return DenoiseLoop(unet, batch, 16, torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8, pooled_dim=6, tokens=3, style_aligned=True, **kw)

    assert torch.equal(loop(guidance_scale=5.0).style_aligned_table, torch.zeros(10)), "off until set_style_aligned"
    with pytest.raises(ValueError, match="batch >= 2"):
        loop(batch=1)
    for kw, states in ((dict(pag_scale=3.0), dict(pag=pag.PAG())), (dict(seg_scale=3.0), dict(seg=seg.SEG())), (dict(tile_hw=8), {}),
                       (dict(reference=True), dict(reference=reference.ReferenceRows()))):
        with pytest.raises(ValueError, match="style_aligned=True cannot be combined"):
            loop(states, **kw)
    for name, cls in (("regions", regions.Regions), ("ip_adapter", ip_adapter.IPAdapter), ("t2i_adapter", t2i_adapter.T2IAdapterState),
                      ("controlnet", controlnet.ControlNetState)):
        state = cls.__new__(cls)                             # (only its type is looked at, before anything is bound)
        torch.nn.Module.__init__(state)
        with pytest.raises(ValueError, match=f"compiled with {name}"):
            loop({name: state})


def test_entry_points_exist_and_validate_on_the_host(lib):
    from stabletriton_amd import _C
    assert hasattr(lib, "st_attention_shared") and hasattr(lib, "st_style_adain") and lib.st_abi_version() == _C.ABI_VERSION == 18
    P = 1 << 20                                              # a fake, aligned, never dereferenced device address: validation precedes any launch
    assert lib.st_attention_shared(P, P, P, P, 2, 256, 255, 2, 64, 2, 384, 384, 384, 128, 0.125, None, None, 0, _C.ST_BF16, None) != 0
    assert b"S1" in lib.st_last_error()
    assert lib.st_style_adain_workspace(4, 264, 640, 2) == 2 * 2 * 4 * 2 * 640
    assert lib.st_style_adain(P, P + 128, None, 2, 4, 1, 64, 192, 192, 0, 2, P, 1 << 20, None, None, 0, _C.ST_BF16, None) != 0
    assert b"two tokens" in lib.st_last_error(), "T == 1 is refused: the unbiased variance is undefined"
    assert lib.st_style_adain(P, P + 64, None, 2, 4, 264, 64, 192, 192, 0, 2, P, 1 << 20, None, None, 0, _C.ST_BF16, None) != 0
    assert b"overlap" in lib.st_last_error(), "columns [0, 64) and [32, 96) of one buffer share elements: the in-place affine would race"
