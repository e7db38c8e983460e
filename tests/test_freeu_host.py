"""FreeU on the host: the reference and the closed form against the published FFT filter (written here, float64), the fx
pass's site selection and what it leaves the other passes, the unchanged default graph, and a traced float64 TINY module
carrying only the FreeU pass against an independent eager route (tests/freeu_util.py).  No GPU."""
import pytest
import torch
from torch import fx

from stabletriton_amd import freeu, synth
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.optimizers import insert_freeu
from stabletriton_amd.unet import SDXL_BASE, SDXL_REFINER, TINY, UNet2DConditionModel, UNetWithLabelVector
from tests import freeu_util as FU

SIZES = [(4, 4), (8, 8), (32, 32), (64, 64), (38, 26), (76, 52), (3, 5), (2, 6), (19, 13)]
V = FU.SDXL_VALUES


def _planes(h, w, seed=0, n=2, c=6):
    return synth.normal(f"freeu.host.{h}x{w}", (n, c, h, w), seed).double()


# ------------------------------------------------------------------------------------------------ 1. the formulas
@pytest.mark.parametrize("hw", SIZES)
def test_reference_and_closed_form_equal_the_published_filter(hw):
    h, w = hw
    x, r = _planes(h, w, 1, c=8), _planes(h, w, 2)
    for s in (0.2, 0.9, 1.7):
        want = FU.fourier_filter(r, s)
        assert float((freeu.lowpass_closed_form(r, s) - want).abs().max()) < 1e-12
        for version in (1, 2):
            h2, r2 = freeu.reference(x, r, 1.3, s, version)
            assert float((r2 - want).abs().max()) < 1e-12
            assert float((h2 - FU.backbone(x, 1.3, version)).abs().max()) < 1e-12
            assert h2.dtype == torch.float64 and h2.shape == x.shape and r2.shape == r.shape


def test_degenerate_inputs():
    with pytest.raises(ValueError):
        freeu.reference(_planes(1, 8), _planes(1, 8), 1.3, 0.9, 1)
    with pytest.raises(ValueError):
        freeu.reference(_planes(8, 1), _planes(8, 1), 1.3, 0.9, 2)
    with pytest.raises(ValueError):
        freeu.reference(_planes(4, 4), _planes(4, 4), 1.3, 0.9, 3)
    # version 2 on a constant channel-mean map: the documented guard, mu_hat = 0, the identity on h
    const = torch.full((2, 4, 8, 8), 0.5, dtype=torch.float64)
    h2, r2 = freeu.reference(const, const, 1.4, 1.0, 2)
    assert torch.equal(h2, const) and torch.equal(r2, const)
    # neutral parameters are the identity on both, any dtype
    for dt in (torch.float64, torch.float32, torch.bfloat16, torch.float16):
        a, b = _planes(4, 6, 4).to(dt), _planes(4, 6, 5).to(dt)
        for version in (1, 2):
            h2, r2 = freeu.reference(a, b, 1.0, 1.0, version)
            assert torch.equal(h2, a) and torch.equal(r2, b) and h2.dtype == dt


# ------------------------------------------------------------------------------------------------ 2. / 3. the pass
def _meta(spec, wrap=False):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec).eval()
        return UNetWithLabelVector(m) if wrap else m


def _cats_on_channels(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target in (torch.cat, torch.concat)
            and n.kwargs.get("dim", n.args[1] if len(n.args) > 1 else 0) == 1]


def test_pass_counts_on_sdxl_base():
    gm = replace_backend(fx.symbolic_trace(_meta(SDXL_BASE)), freeu=True)
    st = gm.rewrite_stats
    assert st["freeu_sites"] == 6 and st["group_norm_stats"] == 46 and st["skip_cats_removed"] == 9
    assert not _cats_on_channels(gm)
    assert isinstance(gm.freeu, freeu.FreeU) and gm.freeu.host == freeu.NEUTRAL and not gm.freeu.enabled
    sites = [n for n in gm.graph.nodes if n.op == "call_function" and n.target is freeu.freeu_wrapper]
    assert [n.args[3] for n in sites] == [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("spec,wrap", [(SDXL_REFINER, False), (TINY, False), (TINY, True)])
def test_six_sites_on_other_topologies(spec, wrap):
    gm = replace_backend(fx.symbolic_trace(_meta(spec, wrap)), freeu=True)
    assert gm.rewrite_stats["freeu_sites"] == 6 and not _cats_on_channels(gm)


@pytest.mark.parametrize("spec", [SDXL_BASE, TINY])
def test_default_graph_is_unchanged(spec):
    a = replace_backend(fx.symbolic_trace(_meta(spec)))
    b = replace_backend(fx.symbolic_trace(_meta(spec)), freeu=False)
    assert a.code == b.code and "freeu" not in a.code and not hasattr(a, "freeu")
    assert list(a.rewrite_stats.items()) == list(b.rewrite_stats.items())
    assert "freeu_sites" not in a.rewrite_stats
    assert a.rewrite_stats["group_norm_stats"] == 46 and a.rewrite_stats["skip_cats_removed"] == 9
    on = replace_backend(fx.symbolic_trace(_meta(spec)), freeu=True)
    assert {k: v for k, v in on.rewrite_stats.items() if k != "freeu_sites"} == dict(a.rewrite_stats)


# ------------------------------------------------------------------------------------------------ 4. TINY, float64, CPU
def _tiny64():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.double()


def _call(mod, x):
    with torch.no_grad():
        return mod(x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


@pytest.mark.parametrize("hw", [16, (12, 20)])
def test_traced_module_with_the_pass_equals_the_hook_route(hw):
    m = _tiny64()
    x = {k: v.double() for k, v in synth.denoise_inputs(2, hw, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim).items()}
    plain = _call(m, x)
    gm = fx.symbolic_trace(m)
    assert insert_freeu(gm) == 6
    assert torch.equal(_call(gm, x), plain), "neutral parameters must reproduce the plain module exactly"
    for version in (1, 2):
        with FU.hooked(m, **V, version=version):
            want = _call(m, x)
        gm.freeu.set(**V, version=version)
        got = _call(gm, x)
        assert float((want - plain).abs().max()) > 1e-2, "FreeU must matter for this check to mean anything"
        assert float((got - want).abs().max()) < 1e-10, f"version {version}"
    gm.freeu.disable()
    assert torch.equal(_call(gm, x), plain)


# ------------------------------------------------------------------------------------------------ 5. validation
@pytest.mark.parametrize("bad", [dict(s1=0.0), dict(s2=-0.2), dict(b1=float("nan")), dict(b2=float("inf")), dict(s1="x"), dict(b1=None),
                                 dict(version=0), dict(version=3), dict(version=1.5), dict(version=True)])
def test_validation(bad):
    st = freeu.FreeU()
    with pytest.raises(ValueError):
        st.set(**{**V, **bad})
    assert st.host == freeu.NEUTRAL and torch.equal(st.params, torch.tensor(freeu.NEUTRAL))


def test_state_row_and_argument_order():
    st = freeu.FreeU()
    st.set(0.9, 0.2, 1.3, 1.4)                     # diffusers' order: s1, s2, b1, b2
    assert st.host == (1.3, 0.9, 1.4, 0.2, 1.0) and st.enabled
    assert torch.equal(st.params, torch.tensor([1.3, 0.9, 1.4, 0.2, 1.0]))
    p = st.params
    st.set(**V, version=2)
    assert st.params is p and float(p[4]) == 2.0, "an in-place write: captured graphs read this row by address"
    st.disable()
    assert st.params is p and torch.equal(p, torch.tensor(freeu.NEUTRAL))
    with pytest.raises(ValueError, match="freeu=True"):
        freeu.state_of(torch.nn.Linear(2, 2), "enable_freeu")
