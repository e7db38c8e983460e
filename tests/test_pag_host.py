"""Perturbed-attention guidance on the host: the fx pass's site selection and what it leaves the other passes, the unchanged
default graph, a traced CPU TINY module carrying the pass against the independent hooked eager route (tests/pag_util.py), the
adaptive scale table and the tests' float64 guidance against the published formulas on fixed numbers.  No GPU."""
import pytest
import torch
from torch import fx

from stabletriton_amd import pag, synth
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.unet import SDXL_BASE, SDXL_REFINER, TINY, TINY_REFINER, UNet2DConditionModel, UNetWithLabelVector
from tests import pag_util as PU


def _meta(spec, wrap=False):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec).eval()
        return UNetWithLabelVector(m) if wrap else m


def _pag_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is pag.attention_pag_wrapper]


# ------------------------------------------------------------------------------------------------ 1. the pass
# counts from the specs: mid_block has mid_depth (else depths[-1]) layers; an encoder stage resnets_per_level attention blocks of
# depths[level] layers, a decoder stage resnets_per_level + 1
@pytest.mark.parametrize("spec,layers,want", [
    (TINY, ("mid",), 2), (TINY_REFINER, ("mid",), 1), (TINY, ("down_blocks.2",), 4), (TINY, ("up_blocks.0",), 6),
    (SDXL_BASE, ("mid",), 10), (SDXL_REFINER, ("mid",), 4), (TINY, ("mid", "down_blocks.2"), 6), (TINY, "mid", 2)])
def test_site_counts(spec, layers, want):
    gm = replace_backend(fx.symbolic_trace(_meta(spec)), pag_layers=layers)
    assert gm.rewrite_stats["pag_sites"] == want and len(_pag_nodes(gm)) == want
    assert isinstance(gm.pag, pag.PAG) and gm.pag.chunks == 0 and len(gm.pag.sites) == want
    assert all(s.endswith(".attn1") for s in gm.pag.sites)


def test_prefix_in_front_of_the_block_names_does_not_matter():
    gm = replace_backend(fx.symbolic_trace(_meta(TINY, wrap=True)), pag_layers=("mid",))
    assert gm.rewrite_stats["pag_sites"] == 2
    assert all(".mid_block." in "." + s for s in gm.pag.sites)


@pytest.mark.parametrize("layers", [("nowhere",), ("mid", "nowhere"), ("attn2",), (r"attn2\.to_q",), (), ("",)])
def test_patterns_that_select_no_self_attention_raise(layers):
    with pytest.raises(ValueError, match="pag_layers"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), pag_layers=layers)


@pytest.mark.parametrize("spec", [SDXL_BASE, TINY])
def test_default_graph_is_unchanged_and_other_passes_still_fire(spec):
    a = replace_backend(fx.symbolic_trace(_meta(spec)))
    b = replace_backend(fx.symbolic_trace(_meta(spec)), pag_layers=None)
    assert a.code == b.code and "pag" not in a.code and not hasattr(a, "pag")
    assert list(a.rewrite_stats.items()) == list(b.rewrite_stats.items())
    assert "pag_sites" not in a.rewrite_stats and not _pag_nodes(a)
    on = replace_backend(fx.symbolic_trace(_meta(spec)), pag_layers=("mid",))
    assert {k: v for k, v in on.rewrite_stats.items() if k != "pag_sites"} == dict(a.rewrite_stats)
    # the sites take q, k and v as slices of ONE fused, LayerNorm-folded q|k|v projection, as every other self-attention
    from stabletriton_amd.optimizers.wrappers import ln_linear_wrapper
    for n in _pag_nodes(on):
        srcs = {arg.args[0] for arg in n.args[:3]}
        assert len(srcs) == 1
        prod = srcs.pop()
        assert prod.target is ln_linear_wrapper and len(prod.args[3]) == 3


def test_fp8_plan_is_what_it_is_without_pag():
    a = replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True)          # (the plan takes bf16 projections)
    on = replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True, pag_layers=("mid",))
    assert {k: v for k, v in on.rewrite_stats.items() if k != "pag_sites"} == dict(a.rewrite_stats)
    assert a.rewrite_stats["fp8_plan"] and sum(a.rewrite_stats["fp8_plan"].values()) > 0


# ------------------------------------------------------------------------------------------------ 2. TINY on the CPU
def _tiny():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def _call(mod, x):
    with torch.no_grad():
        return mod(x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


def _traced_with_only_the_pass(m):
    """fuse_attention + insert_pag on a traced module: every other node stays eager torch, so it runs on the CPU."""
    from stabletriton_amd.optimizers import fuse_attention, insert_pag
    gm = fx.symbolic_trace(m)
    n_att = fuse_attention(gm)
    sites = insert_pag(gm, ("mid",))
    return gm, n_att, sites


def test_traced_cpu_module_with_the_pass_equals_the_hook_route():
    m = _tiny()
    x = synth.denoise_inputs(6, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    plain = _call(m, x)
    gm, n_att, sites = _traced_with_only_the_pass(m)
    assert sites == 2 and n_att > sites
    # the unselected attention_wrapper leaves have no CPU route: give the traced module eager ones for this test
    from stabletriton_amd.optimizers.wrappers import attention_wrapper
    for n in list(gm.graph.nodes):
        if n.op == "call_function" and n.target is attention_wrapper:
            with gm.graph.inserting_before(n):
                new = gm.graph.call_function(pag.identity_attention_reference, (n.args[0], n.args[1], n.args[2], n.args[5], n.args[4], 0))
            n.replace_all_uses_with(new)
            gm.graph.erase_node(n)
    gm.recompile()
    for chunks in (3, 2, 1):
        with PU.hooked(m, ("mid",), chunks):
            want = _call(m, x)
        with gm.pag.using(chunks):
            got = _call(gm, x)
        assert gm.pag.chunks == 0, "the context manager restores the previous value"
        n = 6 // chunks
        moved = float((want[6 - n:] - plain[6 - n:]).abs().max())
        assert moved > 1e-2, "the perturbation must matter for this check to mean anything"
        assert torch.equal(want[:6 - n], plain[:6 - n]), "unperturbed rows are untouched"
        err = float((got - want).abs().max())
        print(f"chunks {chunks}: traced vs hooked max abs diff {err:.2e}; the perturbation moves its rows by {moved:.2e}")
        assert err < 2e-5 * float(plain.abs().max()), f"chunks {chunks}"        # fp32 rounding: a few 100 ulp of the output's size
    got0 = _call(gm, x)
    assert float((got0 - plain).abs().max()) < 2e-5 * float(plain.abs().max())
    with gm.pag.using(4), pytest.raises(ValueError, match="chunks"):
        _call(gm, x)                                     # 6 % 4 != 0


def test_state_validation_and_state_of():
    st = pag.PAG()
    for bad in (-1, 1.5, True, None, "3"):
        with pytest.raises(ValueError):
            st.set_chunks(bad)
    assert st.chunks == 0 and st.ident_count(6) == 0
    st.set_chunks(3)
    assert st.ident_count(6) == 2 and st.ident_count(3) == 1
    with pytest.raises(ValueError, match="chunks"):
        st.ident_count(4)
    with st.using(2):
        assert st.chunks == 2
        with pytest.raises(RuntimeError), st.using(1):
            assert st.chunks == 1
            raise RuntimeError("inside")
        assert st.chunks == 2
    assert st.chunks == 3
    with pytest.raises(ValueError, match="pag_layers"):
        pag.state_of(torch.nn.Linear(2, 2), "enable_pag")


def test_using_takes_a_latent_size_and_ignores_it():
    """PAG and SEG share `using(chunks, latent_hw)` (pag.PerturbedRows): PAG carries the latent size, restores it, and computes
    the same with it as without."""
    st = pag.PAG()
    assert isinstance(st, pag.PerturbedRows) and st.latent_hw is None
    with st.using(2, (16, 16)) as inside:
        assert inside is st and st.chunks == 2 and st.latent_hw == (16, 16) and st.ident_count(6) == st.tail_count(6) == 3
        with st.using(3):
            assert st.chunks == 3 and st.latent_hw == (16, 16) and st.ident_count(6) == 2
        assert st.chunks == 2 and st.latent_hw == (16, 16)
    assert st.chunks == 0 and st.latent_hw is None
    q, k, v = (torch.randn(4, 5, 8, generator=torch.Generator().manual_seed(i)) for i in range(3))
    with st.using(2):
        want = pag.attention_pag_wrapper(q, k, v, None, 0.5, 2, 4, st)
    with st.using(2, (16, 16)):
        got = pag.attention_pag_wrapper(q, k, v, None, 0.5, 2, 4, st)
    assert torch.equal(got, want) and torch.equal(got[2:], v[2:]) and not torch.equal(got[:2], v[:2])
    with pytest.raises(ValueError, match="PAG: chunks must be a non-negative integer"):
        st.set_chunks(-1)
    with st.using(4), pytest.raises(ValueError, match="PAG: a UNet batch of 6 rows does not divide into 4 chunks"):
        st.ident_count(6)


# ------------------------------------------------------------------------------------------------ 3. scales and formulas
def test_adaptive_scales_against_hand_computed_values():
    ts = [999.0, 800.0, 500.0, 1.0]
    assert pag.adaptive_scales(ts, 3.0) == [3.0, 3.0, 3.0, 3.0]
    assert pag.adaptive_scales(ts, 3.0, 0.0) == [3.0, 3.0, 3.0, 3.0]
    got = pag.adaptive_scales(ts, 3.0, 0.005)
    # 3 - 0.005 * (1000 - t): 2.995, 2.0, 0.5, and 3 - 4.995 < 0 clamps to 0
    assert got == pytest.approx([2.995, 2.0, 0.5, 0.0], abs=1e-12) and got[3] == 0.0
    assert pag.adaptive_scales(torch.tensor(ts), 3.0, 0.005) == pytest.approx(got, abs=1e-4)


def test_float64_guidance_restatement_on_fixed_numbers():
    one = lambda v: torch.full((1, 1, 1, 2), v, dtype=torch.float64)
    en, ep, ex = one(1.0), one(2.0), one(0.5)
    # 1 + 5 (2 - 1) + 3 (2 - 0.5) = 10.5;  without CFG 2 + 3 (2 - 0.5) = 6.5
    assert torch.equal(PU.guide64(en, ep, ex, 5.0, 3.0), one(10.5))
    assert torch.equal(PU.guide64(None, ep, ex, None, 3.0), one(6.5))
    assert torch.equal(PU.guide64(en, ep, ex, 5.0, 0.0), one(6.0))           # s = 0: the CFG value
    # rescale on the total: e_pos = (1, 3) (std sqrt 2), e_neg = 0, e_pert = e_pos, g = 2 -> e = (2, 6) (std 2 sqrt 2), ratio 1/2:
    # phi = 0.7 gives 0.7 * e / 2 + 0.3 e = 0.65 e
    ep = torch.tensor([1.0, 3.0], dtype=torch.float64).view(1, 1, 1, 2)
    got = PU.guide64(torch.zeros_like(ep), ep, ep, 2.0, 3.0, phi=0.7)
    assert float((got - 0.65 * 2.0 * ep).abs().max()) < 1e-15
    mag = PU.guide_magnitude(en, one(2.0), ex, 5.0, 3.0)
    assert torch.equal(mag, one(1.0 + 5.0 * 3.0 + 3.0 * 2.5))


# ------------------------------------------------------------------------------------------------ 4. DenoiseLoop (CPU tensors)
class _NoUNet:
    """Stands in for a compiled UNet: the host-side paths below never evaluate it."""

    def __init__(self, with_pag=True):
        if with_pag:
            self.pag = pag.PAG()


def _loop(unet=None, **kw):
    from stabletriton_amd.pipeline import DenoiseLoop
    from stabletriton_amd.scheduler import euler_discrete_tables
    return DenoiseLoop(unet or _NoUNet(), 2, 16, torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8, pooled_dim=6, tokens=3, **kw)


@pytest.mark.parametrize("guided", [False, True])
def test_loop_rows_conditioning_and_input_blocks(guided):
    kw = dict(guidance_scale=5.0) if guided else {}
    lp = _loop(pag_scale=3.0, mode="step", **kw)
    blocks = 3 if guided else 2
    assert lp.x_in.shape[0] == lp.ehs.shape[0] == lp.text_embeds.shape[0] == lp.time_ids.shape[0] == 2 * blocks
    assert lp.latent.shape[0] == 2 and torch.equal(lp.pag, torch.full((10,), 3.0)) and lp._perturbed_chunks == blocks and isinstance(lp._perturbed, pag.PAG)
    pos = (torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6))
    neg = (torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6))
    lp.set_conditioning(*pos, *(neg if guided else ()))
    for buf, p, q in zip((lp.ehs, lp.text_embeds, lp.time_ids), pos, neg):
        assert torch.equal(buf[-2:], p) and torch.equal(buf[-4:-2], p), "the perturbed block carries the positive conditioning"
        if guided:
            assert torch.equal(buf[:2], q)
    z = torch.randn(2, 4, 16, 16)
    lp.set_noise(z)
    for r in range(blocks):
        assert torch.equal(lp.x_in[2 * r:2 * r + 2], lp.x_in[:2])
    assert torch.equal(lp.x_in[:2], (z * lp.tables.init_noise_sigma) * float(lp.tables.in_scale()[0]))
    table = lp.pag
    lp.set_pag([0.5 * i for i in range(10)])
    assert lp.pag is table and float(lp.pag[4]) == 2.0, "an in-place write: captured graphs read this table by address"
    with pytest.raises(ValueError, match="set_pag"):
        lp.set_pag([1.0] * 9)


def test_loop_error_cases_on_the_host():
    with pytest.raises(ValueError, match="pag_layers"):
        _loop(_NoUNet(with_pag=False), pag_scale=3.0)
    with pytest.raises(ValueError, match="pag_scale"):
        _loop(guidance_scale=5.0).set_pag(1.0)
    with pytest.raises(ValueError, match="guidance_rescale needs guidance_scale"):
        _loop(pag_scale=3.0, guidance_rescale=0.7)
    plain = _loop(_NoUNet(with_pag=False), guidance_scale=5.0)          # without pag_scale nothing about the loop changes
    assert plain.pag is None and plain.x_in.shape[0] == 4 and plain._perturbed_chunks == 0 and plain._perturbed is None


# ------------------------------------------------------------------------------------------------ 5. the C entry points
P = 1 << 20            # fake, aligned, never dereferenced device addresses: validation happens before any launch


def test_entry_points_validate_on_the_host(lib):
    from stabletriton_amd import _C
    assert lib.st_abi_version() == _C.ABI_VERSION == 18

    def euler(**kw):
        a = dict(latent=P, eps=P, next_in=P, dsigma=P, in_scale=P, guidance=P, rescale=None, pag=P, step=P, batch=1, per_sample=1024,
                 n_steps=10, dtype=_C.ST_BF16, ws=None, ws_bytes=0)
        a.update(kw)
        return lib.st_pag_euler_step(a["latent"], a["eps"], a["next_in"], a["dsigma"], a["in_scale"], a["guidance"], a["rescale"], a["pag"],
                                     a["step"], a["batch"], a["per_sample"], a["n_steps"], a["dtype"], a["ws"], a["ws_bytes"], None)

    for name in ("latent", "eps", "next_in", "dsigma", "in_scale", "pag", "step"):
        assert euler(**{name: None}) != 0 and b"pag_euler_step: null" in lib.st_last_error(), name
    assert euler(guidance=None, rescale=P) != 0 and b"guidance" in lib.st_last_error()
    assert euler(per_sample=1020) != 0 and b"multiple of 8" in lib.st_last_error()
    assert euler(eps=P + 4) != 0 and b"aligned" in lib.st_last_error()
    assert euler(dtype=7) != 0 and b"dtype" in lib.st_last_error()
    assert euler(rescale=P) != 0 and b"workspace" in lib.st_last_error()
    rc = lib.st_pag_dpmpp2m_step(P, P, P, P, P, P, None, None, None, P, P, 1, 1024, 10, _C.ST_BF16, None, 0, None)
    assert rc != 0 and b"pag_dpmpp2m_step: null" in lib.st_last_error()
    rc = lib.st_pag_sde_step(P, P, P, P, P, P, None, None, None, P, P, P, 1, 1024, 10, _C.ST_BF16, None, 0, None)
    assert rc != 0 and b"pag_sde_step: null" in lib.st_last_error()
    # the two-way entry points keep their own names in their messages
    rc = lib.st_cfg_euler_step(P, P, P, P, P, None, None, P, 1, 1024, 10, _C.ST_BF16, None, 0, None)
    assert rc != 0 and b"cfg_euler_step: null" in lib.st_last_error()

    def att(**kw):
        a = dict(q=P, k=P, v=P, out=P, B=3, T=64, S=64, H=2, D=64, ldq=384, ldk=384, ldv=384, ldo=128, dtype=_C.ST_BF16, ident=1)
        a.update(kw)
        return lib.st_attention_pag(a["q"], a["k"], a["v"], a["out"], a["B"], a["T"], a["S"], a["H"], a["D"], a["ldq"], a["ldk"], a["ldv"],
                                    a["ldo"], 0.125, a["dtype"], a["ident"], None)

    assert att(v=None) != 0 and b"null" in lib.st_last_error()
    assert att(S=77) != 0 and b"T == S" in lib.st_last_error()
    assert att(ident=4) != 0 and b"ident_count" in lib.st_last_error()
    assert att(ident=-1) != 0 and b"ident_count" in lib.st_last_error()
    assert att(D=40) != 0 and b"head_dim" in lib.st_last_error()
    assert att(ldv=388) != 0 and b"16-byte" in lib.st_last_error()
    assert att(ldo=132) != 0 and b"16-byte" in lib.st_last_error()
    assert att(v=P + 8) != 0 and b"16-byte" in lib.st_last_error()
    assert att(ldo=64) != 0 and b"shorter" in lib.st_last_error()
    assert att(dtype=_C.ST_F32S) != 0 and b"dtype" in lib.st_last_error()
