"""Smoothed energy guidance on the host: the tap rule, reflect indexing and the token grid rule against the tests' own statement
(tests/seg_util.py) and torch's reflect padding, the fx pass's site selection and what it leaves the other passes, a traced CPU TINY
module carrying the pass against the independent hooked eager route, the state's validation, DenoiseLoop's host side and the C
entry points' argument checks.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import fx

from stabletriton_amd import seg, synth
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel
from tests import pag_util as PU
from tests import seg_util as SU

INF = float("inf")


def _meta(spec):
    with torch.device("meta"):
        return UNet2DConditionModel(spec).eval()


def _seg_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is seg.attention_seg_wrapper]


# ------------------------------------------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("grid,want", [(4, (3, 5, 5, 5)), (6, (3, 7, 7, 7)), (8, (3, 7, 9, 9)), (32, (3, 7, 19, 33)), (64, (3, 7, 19, 61))])
def test_tap_counts(grid, want):
    for sigma, k in zip((0.5, 1.0, 3.0, 10.0), want):
        assert seg.tap_count(sigma, grid, grid) == k == SU.tap_count(sigma, grid, grid), (grid, sigma)
        assert k % 2 == 1 and k // 2 < grid
        row = seg.param_row(sigma, grid, grid)
        assert len(row) == seg.PARAM_WORDS and row[0] == 0.0 and row[1] == k
        g = SU.taps64(sigma, k)
        assert torch.allclose(torch.tensor(row[2:2 + k], dtype=torch.float64), g, rtol=0, atol=1e-15)
        assert abs(sum(row[2:2 + k]) - 1.0) < 1e-14 and all(v == 0.0 for v in row[2 + k:])
    # a rectangle clamps on its short side
    assert seg.tap_count(10.0, 6, 4) == 5 and seg.tap_count(10.0, 5, 7) == 5 and seg.tap_count(10.0, 128, 128) == 61
    assert seg.tap_count(100.0, 128, 128) == 129 and 2 + 129 <= seg.PARAM_WORDS
    mean = seg.param_row(INF, 32, 32)
    assert mean[0] == 1.0 and seg.param_row(9999.0, 8, 8)[0] == 1.0 and seg.param_row(9998.0, 8, 8)[0] == 0.0


@pytest.mark.parametrize("n,k", [(4, 5), (5, 5), (7, 3), (32, 33)])
def test_reflect_indexing_against_torch_padding(n, k):
    r = k // 2
    line = torch.arange(n, dtype=torch.float64)
    padded = F.pad(line.view(1, 1, n), (r, r), mode="reflect").view(-1)
    for p in range(n):
        for i in range(k):
            assert SU.reflect_index(p + i - r, n) == int(padded[p + i])
    # the product's plain-torch statement and the tests' agree on an impulse response at the edge
    q = torch.zeros(1, n * n, 1, dtype=torch.float64)
    q[0, 0, 0] = 1.0
    q[0, n * n - 1, 0] = 2.0
    sigma = 1.0 if k <= 7 else 10.0
    assert float((seg.blur_reference(q, (n, n), sigma) - SU.blur64(q, (n, n), sigma)).abs().max()) < 1e-15


def test_blur_reference_against_the_tests_statement_on_rectangles():
    for (h, w), sigma in (((6, 4), 3.0), ((5, 7), 0.5), ((12, 20), 10.0), ((4, 4), INF), ((6, 4), 1.0)):
        q = torch.randn(2, h * w, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(h * w))
        assert float((seg.blur_reference(q, (h, w), sigma) - SU.blur64(q, (h, w), sigma)).abs().max()) < 1e-14


def test_token_grid_rule():
    for latent, cases in (((16, 16), {256: (16, 16), 64: (8, 8), 16: (4, 4)}), ((24, 16), {384: (24, 16), 96: (12, 8), 24: (6, 4)}),
                          ((152, 104), {15808: (152, 104), 3952: (76, 52), 988: (38, 26), 247: (19, 13)})):
        for tokens, want in cases.items():
            assert seg.site_grid(latent, tokens) == want == SU.grid_of(latent, tokens)
    for latent, tokens in (((16, 16), 100), ((24, 16), 48), ((18, 8), 9), ((152, 104), 3953)):
        with pytest.raises(ValueError, match="SEG"):
            seg.site_grid(latent, tokens)
    assert seg.SEG.grids((152, 104)) == [(76, 52), (38, 26), (19, 13)], "grids beyond 128 a side get no row"
    assert seg.SEG.grids((16, 16)) == [(16, 16), (8, 8), (4, 4), (2, 2)]


# ------------------------------------------------------------------------------------------------ 2. the pass
@pytest.mark.parametrize("spec,layers,want", [(TINY, ("mid",), 2), (TINY, ("down_blocks.1", "mid"), 4), (SDXL_BASE, ("mid",), 10), (TINY, "mid", 2)])
def test_site_counts(spec, layers, want):
    gm = replace_backend(fx.symbolic_trace(_meta(spec)), seg_layers=layers)
    assert gm.rewrite_stats["seg_sites"] == want and len(_seg_nodes(gm)) == want
    assert isinstance(gm.seg, seg.SEG) and gm.seg.chunks == 0 and len(gm.seg.sites) == want and gm.seg.sigma == INF
    assert all(s.endswith(".attn1") for s in gm.seg.sites)


@pytest.mark.parametrize("layers", [("nowhere",), ("mid", "nowhere"), ("attn2",), (), ("",)])
def test_patterns_that_select_no_self_attention_raise(layers):
    with pytest.raises(ValueError, match="seg_layers"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), seg_layers=layers)


def test_seg_and_pag_together_raise():
    with pytest.raises(ValueError, match="seg_layers cannot be combined with pag_layers"):
        replace_backend(fx.symbolic_trace(_meta(TINY)), seg_layers=("mid",), pag_layers=("down_blocks.1",))


@pytest.mark.parametrize("layers", [("mid",), ("down_blocks.1", "mid"), (r"up_blocks\.0.*transformer_blocks\.1",)])
def test_pag_and_seg_choose_the_same_sites(layers):
    """One site rule and one selection by regular expressions serve both passes."""
    from stabletriton_amd import pag
    from stabletriton_amd.optimizers import fuse_attention, insert_pag, insert_seg
    a, b = fx.symbolic_trace(_meta(TINY)), fx.symbolic_trace(_meta(TINY))
    fuse_attention(a), fuse_attention(b)
    assert insert_pag(a, layers) == insert_seg(b, layers) == len(a.pag.sites) > 0
    assert a.pag.sites == b.seg.sites and a.pag.layers == b.seg.layers == layers
    at = [i for i, n in enumerate(a.graph.nodes) if n.target is pag.attention_pag_wrapper]
    assert at == [i for i, n in enumerate(b.graph.nodes) if n.target is seg.attention_seg_wrapper] and len(at) == len(a.pag.sites)
    for layers_, flag in ((("nowhere",), "pag_layers"), ((), "seg_layers")):
        insert = insert_pag if flag == "pag_layers" else insert_seg
        with pytest.raises(ValueError, match=f"^{flag}: "):
            insert(fx.symbolic_trace(_meta(TINY)), layers_)


@pytest.mark.parametrize("spec", [SDXL_BASE, TINY])
def test_default_graph_is_unchanged_and_other_passes_still_fire(spec):
    a = replace_backend(fx.symbolic_trace(_meta(spec)))
    b = replace_backend(fx.symbolic_trace(_meta(spec)), seg_layers=None)
    assert a.code == b.code and "seg" not in a.code and not hasattr(a, "seg")
    assert list(a.rewrite_stats.items()) == list(b.rewrite_stats.items())
    assert "seg_sites" not in a.rewrite_stats and not _seg_nodes(a)
    on = replace_backend(fx.symbolic_trace(_meta(spec)), seg_layers=("mid",))
    assert {k: v for k, v in on.rewrite_stats.items() if k != "seg_sites"} == dict(a.rewrite_stats)
    from stabletriton_amd.optimizers.wrappers import ln_linear_wrapper
    for n in _seg_nodes(on):                                  # q, k, v: slices of ONE fused, LayerNorm-folded q|k|v projection
        srcs = {arg.args[0] for arg in n.args[:3]}
        assert len(srcs) == 1
        prod = srcs.pop()
        assert prod.target is ln_linear_wrapper and len(prod.args[3]) == 3


def test_fp8_plan_is_what_it_is_without_seg():
    a = replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True)
    on = replace_backend(fx.symbolic_trace(_meta(TINY).to(torch.bfloat16)), fp8=True, seg_layers=("mid",))
    assert {k: v for k, v in on.rewrite_stats.items() if k != "seg_sites"} == dict(a.rewrite_stats)


# ------------------------------------------------------------------------------------------------ 3. TINY on the CPU
def _tiny():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def _call(mod, x):
    with torch.no_grad():
        return mod(x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], {"text_embeds": x["text_embeds"], "time_ids": x["time_ids"]})[0]


@pytest.mark.parametrize("hw", [(16, 16), (24, 16)])
def test_traced_cpu_module_with_the_pass_equals_the_hook_route(hw):
    from stabletriton_amd.optimizers import fuse_attention, insert_seg
    from stabletriton_amd.optimizers.wrappers import attention_wrapper
    from stabletriton_amd.pag import identity_attention_reference
    m = _tiny()
    layers = ("down_blocks.1", "mid")
    x = synth.denoise_inputs(6, hw, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    plain = _call(m, x)
    gm = fx.symbolic_trace(m)
    n_att = fuse_attention(gm)
    sites = insert_seg(gm, layers)
    assert sites == 4 and n_att > sites
    for n in list(gm.graph.nodes):      # the unselected attention_wrapper leaves have no CPU route: eager ones for this test
        if n.op == "call_function" and n.target is attention_wrapper:
            with gm.graph.inserting_before(n):
                new = gm.graph.call_function(identity_attention_reference, (n.args[0], n.args[1], n.args[2], n.args[5], n.args[4], 0))
            n.replace_all_uses_with(new)
            gm.graph.erase_node(n)
    gm.recompile()
    for chunks, sigma in ((3, INF), (3, 1.0), (2, 3.0), (1, 0.5)):
        gm.seg.set_sigma(sigma)
        with SU.hooked(m, layers, chunks, hw, sigma):
            want = _call(m, x)
        with gm.seg.using(chunks, hw):
            got = _call(gm, x)
        assert gm.seg.chunks == 0 and gm.seg.latent_hw is None, "the context manager restores the previous values"
        n = 6 // chunks
        moved = float((want[6 - n:] - plain[6 - n:]).abs().max())
        assert moved > 1e-2, "the perturbation must matter for this check to mean anything"
        assert torch.equal(want[:6 - n], plain[:6 - n]), "unperturbed rows are untouched"
        err = float((got - want).abs().max())
        print(f"{hw} chunks {chunks} sigma {sigma}: traced vs hooked max abs diff {err:.2e}; the perturbation moves its rows by {moved:.2e}")
        assert err < 2e-5 * float(plain.abs().max())             # fp32 rounding: a few 100 ulp of the output's size
    assert float((_call(gm, x) - plain).abs().max()) < 2e-5 * float(plain.abs().max())
    with gm.seg.using(4, hw), pytest.raises(ValueError, match="chunks"):
        _call(gm, x)                                             # 6 % 4 != 0


# ------------------------------------------------------------------------------------------------ 4. the state
def test_state_validation_and_state_of():
    st = seg.SEG()
    for bad in (0, 0.0, -1.0, float("nan"), "3", None, True, torch.tensor(1.0)):
        with pytest.raises(ValueError, match="sigma"):
            st.set_sigma(bad)
    assert st.sigma == INF
    st.set_sigma(2)
    assert st.sigma == 2.0
    for bad in (-1, 1.5, True, None, "3"):
        with pytest.raises(ValueError):
            st.set_chunks(bad)
    with pytest.raises(ValueError, match="latent"):
        with st.using(3):
            pass
    assert st.chunks == 0 and st.tail_count(6) == 0
    with st.using(3, (16, 16)):
        assert st.chunks == 3 and st.latent_hw == (16, 16) and st.tail_count(6) == 2
        with pytest.raises(ValueError, match="chunks"):
            st.tail_count(4)
        with pytest.raises(RuntimeError), st.using(1, (24, 16)):
            assert st.latent_hw == (24, 16)
            raise RuntimeError("inside")
        assert st.chunks == 3 and st.latent_hw == (16, 16)
    assert st.chunks == 0 and st.latent_hw is None
    with pytest.raises(ValueError, match="seg_layers"):
        seg.state_of(torch.nn.Linear(2, 2), "enable_seg")


def test_using_without_a_latent_size_raises_and_changes_nothing():
    from stabletriton_amd import pag
    st = seg.SEG()
    assert isinstance(st, pag.PerturbedRows) and not hasattr(st, "ident_count")
    with pytest.raises(ValueError, match="SEG: using\\(chunks, latent_hw\\) needs the call's latent size"), st.using(2):
        pass
    assert st.chunks == 0 and st.latent_hw is None
    with st.using(0):                                          # chunks 0 needs none: ordinary attention
        assert st.chunks == 0 and st.latent_hw is None and st.tail_count(6) == 0
    with pytest.raises(ValueError, match="SEG: chunks must be a non-negative integer"), st.using(-1, (16, 16)):
        pass
    assert st.chunks == 0 and st.latent_hw is None
    with st.using(4, (16, 16)), pytest.raises(ValueError, match="SEG: a UNet batch of 6 rows does not divide into 4 chunks"):
        st.tail_count(6)


def test_parameter_rows_are_written_in_place():
    st = seg.SEG()
    st.bind((16, 16), "cpu")
    rows = dict(st._rows)
    assert sorted(g for _, _, g in rows) == [(2, 2), (4, 4), (8, 8), (16, 16)]
    assert all(float(r[0]) == 1.0 for r in rows.values()), "sigma = infinity until set"
    st.set_sigma(1.0)
    st.bind((16, 16), "cpu")
    for key, row in st._rows.items():
        assert row is rows[key] and float(row[0]) == 0.0 and int(row[1]) == seg.tap_count(1.0, *key[2])
        assert torch.equal(row, torch.tensor(seg.param_row(1.0, *key[2]), dtype=torch.float32))
    st.set_sigma(INF)
    assert all(r is rows[k] and float(r[0]) == 1.0 for k, r in st._rows.items())
    with st.using(3, (16, 16)):
        grid, row = st.row_for(64, "cpu")
    assert grid == (8, 8) and row is rows[("cpu", None, (8, 8))]


# ------------------------------------------------------------------------------------------------ 5. DenoiseLoop (CPU tensors)
class _NoUNet:
    """Stands in for a compiled UNet: the host-side paths below never evaluate it."""

    def __init__(self, with_seg=True, with_pag=False):
        if with_seg:
            self.seg = seg.SEG()
        if with_pag:
            from stabletriton_amd import pag
            self.pag = pag.PAG()


def _loop(unet=None, **kw):
    from stabletriton_amd.pipeline import DenoiseLoop
    from stabletriton_amd.scheduler import euler_discrete_tables
    return DenoiseLoop(unet or _NoUNet(), 2, (24, 16), torch.float32, "cpu", euler_discrete_tables(10), cross_dim=8, pooled_dim=6, tokens=3, **kw)


@pytest.mark.parametrize("guided", [False, True])
def test_loop_rows_tables_and_bound_state(guided):
    kw = dict(guidance_scale=5.0) if guided else {}
    unet = _NoUNet()
    lp = _loop(unet, seg_scale=3.0, seg_sigma=1.0, mode="step", **kw)
    blocks = 3 if guided else 2
    assert lp.x_in.shape[0] == lp.ehs.shape[0] == 2 * blocks and lp.latent.shape[0] == 2
    assert torch.equal(lp.pag, torch.full((10,), 3.0)) and lp._perturbed_chunks == blocks and lp._perturbed is unet.seg
    assert unet.seg.sigma == 1.0 and sorted(g for _, _, g in unet.seg._rows) == [(3, 2), (6, 4), (12, 8), (24, 16)]
    pos = (torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6))
    neg = (torch.randn(2, 3, 8), torch.randn(2, 6), torch.randn(2, 6))
    lp.set_conditioning(*pos, *(neg if guided else ()))
    for buf, p in zip((lp.ehs, lp.text_embeds, lp.time_ids), pos):
        assert torch.equal(buf[-2:], p) and torch.equal(buf[-4:-2], p), "the perturbed block carries the positive conditioning"
    table, row = lp.pag, unet.seg._rows[("cpu", None, (6, 4))]
    lp.set_seg([0.5 * i for i in range(10)], INF)
    assert lp.pag is table and float(lp.pag[4]) == 2.0 and float(row[0]) == 1.0 and unet.seg.sigma == INF
    lp.set_seg(sigma=3.0)
    assert float(lp.pag[4]) == 2.0 and float(row[0]) == 0.0 and int(row[1]) == 5
    lp.set_seg(scale=1.5)
    assert float(lp.pag[4]) == 1.5 and unet.seg.sigma == 3.0
    with pytest.raises(ValueError, match="set_seg"):
        lp.set_seg([1.0] * 9)
    with pytest.raises(ValueError, match="sigma"):
        lp.set_seg(sigma=-1.0)
    with pytest.raises(ValueError, match="set_pag"):
        lp.set_pag(1.0)


def test_loop_error_cases_on_the_host():
    with pytest.raises(ValueError, match="seg_layers"):
        _loop(_NoUNet(with_seg=False), seg_scale=3.0)
    with pytest.raises(ValueError, match="seg_scale cannot be combined with pag_scale"):
        _loop(_NoUNet(with_pag=True), seg_scale=3.0, pag_scale=3.0)
    with pytest.raises(ValueError, match="seg_scale"):
        _loop(guidance_scale=5.0).set_seg(1.0)
    with pytest.raises(ValueError, match="sigma"):
        _loop(seg_scale=3.0, seg_sigma=0.0)
    with pytest.raises(ValueError, match="set_seg"):
        _loop(seg_scale=[1.0, 2.0])
    plain = _loop(_NoUNet(with_seg=False), guidance_scale=5.0)      # without seg_scale nothing about the loop changes
    assert plain.pag is None and plain.x_in.shape[0] == 4 and plain._perturbed_chunks == 0 and plain._perturbed is None


# ------------------------------------------------------------------------------------------------ 6. the C entry points
P = 1 << 20            # fake, aligned, never dereferenced device addresses: validation happens before any launch


def test_entry_points_validate_on_the_host(lib):
    from stabletriton_amd import _C
    assert lib.st_abi_version() == _C.ABI_VERSION == 18
    assert _C.SEG_PARAM_WORDS == seg.PARAM_WORDS and _C.SEG_MAX_SIDE == seg.MAX_SIDE

    def blur(**kw):
        a = dict(q=P, out=P + 4096, params=P, n=1, h=8, w=8, C=128, ldq=384, ldo=128, dtype=_C.ST_BF16, ws=None, ws_bytes=0)
        a.update(kw)
        return lib.st_seg_blur(a["q"], a["out"], a["params"], a["n"], a["h"], a["w"], a["C"], a["ldq"], a["ldo"], a["dtype"], a["ws"], a["ws_bytes"], None)

    for name in ("q", "out", "params"):
        assert blur(**{name: None}) != 0 and b"seg_blur: null" in lib.st_last_error(), name
    assert blur(h=129) != 0 and b"larger than 128 x 128" in lib.st_last_error()
    assert blur(w=200) != 0 and b"larger than 128 x 128" in lib.st_last_error()
    assert blur(h=0) != 0 and b"bad shape" in lib.st_last_error()
    assert blur(C=132) != 0 and b"16-byte" in lib.st_last_error()
    assert blur(ldq=388) != 0 and b"16-byte" in lib.st_last_error()
    assert blur(q=P + 8) != 0 and b"16-byte" in lib.st_last_error()
    assert blur(ldo=64) != 0 and b"shorter" in lib.st_last_error()
    assert blur(dtype=_C.ST_F32S) != 0 and b"dtype" in lib.st_last_error()
    # the plane pair of a 64 x 64 grid of 16-bit elements does not fit the LDS: the general form needs its workspace
    need = lib.st_seg_blur_workspace_bytes(2, 64, 64, 640, _C.ST_BF16)
    assert need == 2 * 4096 * 640 * 4 and lib.st_seg_blur_workspace_bytes(1, 32, 32, 1280, _C.ST_BF16) == 0
    assert lib.st_seg_blur_workspace_bytes(1, 128, 128, 64, _C.ST_F32) == 128 * 128 * 64 * 4
    assert blur(n=2, h=64, w=64, C=640, ldq=640, ldo=640) != 0 and b"workspace" in lib.st_last_error()
    assert blur(n=2, h=64, w=64, C=640, ldq=640, ldo=640, ws=P, ws_bytes=need - 4) != 0 and b"workspace" in lib.st_last_error()

    def att(**kw):
        a = dict(q=P, k=P, v=P, out=P, scratch=P, B=3, T=64, S=64, H=2, D=64, ldq=384, ldk=384, ldv=384, ldo=128, dtype=_C.ST_BF16, tail=1,
                 h=8, w=8, params=P)
        a.update(kw)
        return lib.st_attention_seg(a["q"], a["k"], a["v"], a["out"], a["scratch"], a["B"], a["T"], a["S"], a["H"], a["D"], a["ldq"], a["ldk"],
                                    a["ldv"], a["ldo"], 0.125, a["dtype"], a["tail"], a["h"], a["w"], a["params"], None, 0, None)

    assert att(v=None) != 0 and b"null" in lib.st_last_error()
    assert att(S=77) != 0 and b"T == S" in lib.st_last_error()
    assert att(h=4) != 0 and b"token grid" in lib.st_last_error()
    assert att(tail=4) != 0 and b"tail_count" in lib.st_last_error()
    assert att(tail=-1) != 0 and b"tail_count" in lib.st_last_error()
    assert att(D=40) != 0 and b"head_dim" in lib.st_last_error()
    assert att(ldv=388) != 0 and b"16-byte" in lib.st_last_error()
    assert att(scratch=P + 8) != 0 and b"16-byte" in lib.st_last_error()
    assert att(scratch=None) != 0 and b"scratch" in lib.st_last_error()
    assert att(ldo=64) != 0 and b"shorter" in lib.st_last_error()
    assert att(T=129 * 2, S=129 * 2, h=129, w=2) != 0 and b"larger than 128 x 128" in lib.st_last_error()
