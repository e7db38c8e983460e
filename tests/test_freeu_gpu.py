"""FreeU on the GPU: the op against freeu.reference in float64, the GroupNorm partials it emits, a TINY UNet step against the
float64 hook route (tests/freeu_util.py), and one SDXL-base strict step against a CPU fixture."""
import pytest
import torch

from oracle import unet_oracle as orc
from stabletriton_amd import freeu, ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import freeu_util as FU
from tests.util import TOL, assert_close, golden, rounded

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
V = FU.SDXL_VALUES
# (C_h, C_skip, H, W, slot): SDXL-base's six sites at latent 128; a rectangular aspect bucket (152 x 104) at the same two stages;
# TINY's two stages at latent 16; an odd map
SHAPES = [(1280, 1280, 32, 32, 0), (1280, 1280, 32, 32, 0), (1280, 640, 32, 32, 0), (1280, 640, 64, 64, 1), (640, 640, 64, 64, 1),
          (640, 320, 64, 64, 1), (1280, 640, 38, 26, 0), (640, 320, 76, 52, 1), (256, 128, 4, 4, 0), (128, 64, 8, 8, 1), (64, 40, 3, 5, 0)]


def _params(dev, version, neutral=False):
    st = freeu.FreeU(dev)
    if not neutral:
        st.set(**V, version=version)
    return st


def _pair(ch, cs, h, w, n, dtype, dev, tag=""):
    cl = torch.channels_last
    a = rounded(synth.normal(f"freeu.h{tag}", (n, ch, h, w), 7), dtype)
    b = rounded(synth.normal(f"freeu.r{tag}", (n, cs, h, w), 8), dtype)
    return a, b, a.to(dev, dtype).contiguous(memory_format=cl), b.to(dev, dtype).contiguous(memory_format=cl)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_op_against_float64_reference(gpu, dtype, version):
    st = _params(gpu, version)
    neutral = _params(gpu, version, neutral=True)
    worst = 0.0
    for ch, cs, h, w, slot in dict.fromkeys(SHAPES):
        for n in (1, 2):
            a, b, ag, bg = _pair(ch, cs, h, w, n, dtype, gpu)
            bq, sq = (V["b1"], V["s1"]) if slot == 0 else (V["b2"], V["s2"])
            want_h, want_r = freeu.reference(a.double(), b.double(), bq, sq, version)
            h2, r2, sh, sr = ops.freeu(ag, bg, st.params, slot)
            what = f"{dtype} v{version} N={n} C=({ch},{cs}) {h}x{w}"
            assert h2.is_contiguous(memory_format=torch.channels_last) and r2.is_contiguous(memory_format=torch.channels_last)
            assert_close(h2, want_h, dtype, what + " h'")
            assert_close(r2, want_r, dtype, what + " skip'")
            worst = max(worst, float((r2.double().cpu() - want_r).abs().max() / want_r.abs().max()),
                        float((h2.double().cpu() - want_h).abs().max() / want_h.abs().max()))
            assert float((want_r - b.double()).abs().max()) > 1e-3 and float((want_h - a.double()).abs().max()) > 1e-2, what
            assert (sh is None) == (sr is None) == ((h * w) % 64 != 0), what + ": statistics exactly for the shapes the op tiles"
            again = ops.freeu(ag, bg, st.params, slot)
            assert torch.equal(_bits(again[0]), _bits(h2)) and torch.equal(_bits(again[1]), _bits(r2)), what + ": two calls differ"
            if sh is not None:
                assert torch.equal(again[2].buf, sh.buf) and torch.equal(again[3].buf, sr.buf)
            i0, i1, _, _ = ops.freeu(ag, bg, neutral.params, slot)
            assert torch.equal(_bits(i0), _bits(ag)) and torch.equal(_bits(i1), _bits(bg)), what + ": neutral parameters must copy the bits"
            assert i0.data_ptr() != ag.data_ptr() and i1.data_ptr() != bg.data_ptr()
    print(f"freeu op {dtype} v{version}: worst max err / max|ref| = {worst:.2e} (gate {TOL[dtype]:.0e})")


def test_op_reads_its_parameters_when_it_runs(gpu):
    """The row is read by address: the same call after an in-place `set` gives the new result (what a captured graph relies on)."""
    a, b, ag, bg = _pair(128, 64, 8, 8, 1, torch.float32, gpu)
    st = freeu.FreeU(gpu)
    p = st.params.data_ptr()
    for version in (1, 2):
        st.set(**V, version=version)
        assert st.params.data_ptr() == p
        h2, r2, _, _ = ops.freeu(ag, bg, st.params, 1)
        want_h, want_r = freeu.reference(a.double(), b.double(), V["b2"], V["s2"], version)
        assert_close(h2, want_h, torch.float32, f"v{version}")
        assert_close(r2, want_r, torch.float32, f"v{version}")
    flat = torch.full_like(ag, 0.5)                 # version 2 on a constant map: the documented guard, the identity
    h2, _, _, _ = ops.freeu(flat, bg, st.params, 1)
    assert torch.equal(h2, flat)


def test_op_rejects_what_it_does_not_take(gpu):
    st = freeu.FreeU(gpu)
    cl = torch.channels_last
    z = lambda *s: torch.zeros(s, device=gpu).contiguous(memory_format=cl)
    with pytest.raises(ops.BackendError):
        ops.freeu(z(1, 8, 1, 8), z(1, 8, 1, 8), st.params, 0)          # H = 1: the published box is empty
    with pytest.raises(ops.BackendError):
        ops.freeu(z(1, 6, 4, 4), z(1, 8, 4, 4), st.params, 0)          # channels that are no whole 16-byte vectors
    with pytest.raises(ops.BackendError):
        ops.freeu(z(1, 8, 4, 4), z(1, 8, 4, 4), st.params, 2)
    with pytest.raises(ops.BackendError):
        ops.freeu(z(1, 8, 4, 4), z(2, 8, 4, 4), st.params, 0)
    with pytest.raises(ops.BackendError):
        ops.freeu(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), st.params, 0)      # no CPU fallback in ops


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_emitted_statistics_feed_the_two_source_group_norm(gpu, dtype, version):
    st = _params(gpu, version)
    for ch, cs, h, w, slot in [(1280, 640, 32, 32, 0), (640, 320, 64, 64, 1), (128, 64, 8, 8, 1), (640, 320, 38, 26, 0)]:
        for n in (1, 2):
            _, _, ag, bg = _pair(ch, cs, h, w, n, dtype, gpu, tag=".gn")
            c = ch + cs
            weight = (1.0 + 0.1 * synth.normal("freeu.gn.w", (c,), 3)).to(gpu, dtype)
            bias = (0.05 * synth.normal("freeu.gn.b", (c,), 4)).to(gpu, dtype)
            h2, r2, sh, sr = ops.freeu(ag, bg, st.params, slot)
            assert (sh is None) == ((h * w) % 64 != 0)
            if sh is not None:
                assert sh.channels == ch and sr.channels == cs and (h * w) % sh.rows == 0 and sh.rows == sr.rows
                assert sh.buf.shape == (n * h * w // sh.rows, ch, 2) and sr.buf.shape == (n * h * w // sr.rows, cs, 2)
                per_tile = h2.float().permute(0, 2, 3, 1).reshape(-1, sh.rows, ch)
                assert_close(sh.buf[..., 0], per_tile.sum(1), torch.float32, "sum partials", factor=5)
                assert_close(sh.buf[..., 1], per_tile.pow(2).sum(1), torch.float32, "square partials", factor=5)
            got = ops.group_norm_from_stats_cat(h2, r2, (sh, sr), 32, weight, bias, 1e-5, True)
            want = ops.group_norm(torch.cat([h2, r2], dim=1), 32, weight, bias, 1e-5, True)
            assert_close(got, want, dtype, f"{dtype} v{version} N={n} C=({ch},{cs}) {h}x{w}")
            exact = torch.nn.functional.silu(torch.nn.functional.group_norm(torch.cat([h2, r2], dim=1).double().cpu(), 32, weight.double().cpu(),
                                                                            bias.double().cpu(), 1e-5))
            assert_close(got, exact, dtype, f"{dtype} v{version} N={n} C=({ch},{cs}) {h}x{w} vs float64")


# ------------------------------------------------------------------------------------------------ TINY UNet step
def _tiny(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


def _ref64(model, x, dtype, t, **fu):
    """The float64 CPU module on the weights and inputs the kernels see, plain and through the hook route."""
    m64 = UNet2DConditionModel(TINY).eval().requires_grad_(False).double()
    m64.load_state_dict({k: v.detach().double().cpu() for k, v in model.state_dict().items()})
    xi = {k: rounded(v, dtype).double() for k, v in x.items()}
    call = lambda: m64(xi["latent"], torch.tensor(t), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]
    with torch.no_grad():
        plain = call()
        out = {}
        for version in (1, 2):
            with FU.hooked(m64, **fu, version=version):
                out[version] = call()
    return plain, out


@pytest.mark.parametrize("hw", [16, (12, 20)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tiny_step_with_freeu_vs_float64_hook_route(gpu, dtype, hw):
    """Gates: fp32 the project's strict 1e-3; bf16 / fp16 the TINY step gates of tests/test_unet_gpu.py (0.1 / 0.025), times
    max|ref_freeu| / max|ref_plain| when FreeU enlarges the output (both float64 references, computed here)."""
    model = _tiny(dtype, gpu)
    gm = optimize_model(model, cuda_graph=False, freeu=True)
    assert gm.rewrite_stats["freeu_sites"] == 6 and gm.rewrite_stats["skip_cats_removed"] == 9
    x = synth.denoise_inputs(2, hw, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    step = lambda: gm(xg["latent"], torch.tensor(500.0, device=gpu), xg["encoder_hidden_states"],
                      {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0].double().cpu()
    plain, refs = _ref64(model, x, dtype, 500.0, **V)
    base = {torch.float32: ABS_TOL_STRICT, torch.bfloat16: 0.1, torch.float16: 0.025}[dtype]
    with torch.no_grad():
        err0 = float((step() - plain).abs().max())
        print(f"tiny {dtype} latent {hw} freeu=True, neutral: max abs err vs float64 plain {err0:.2e} (gate {base:.1e})")
        assert err0 <= base
        for version in (1, 2):
            gm.freeu.set(**V, version=version)
            ref = refs[version]
            ratio = float(ref.abs().max() / plain.abs().max())
            gate = base if dtype == torch.float32 else base * max(1.0, ratio)
            err = float((step() - ref).abs().max())
            print(f"tiny {dtype} latent {hw} FreeU v{version}: max abs err {err:.2e} (gate {gate:.2e}; |ref| max {float(ref.abs().max()):.2f}, "
                  f"plain {float(plain.abs().max()):.2f}; FreeU moves the output by {float((ref - plain).abs().max()):.2e})")
            assert float((ref - plain).abs().max()) > 100 * ABS_TOL_STRICT, "FreeU must matter for this check to mean anything"
            assert err <= gate


def test_neutral_fp32_module_vs_oracle(gpu):
    """A freeu=True module with neutral parameters is the plain network (not bit for bit: the statistics of the six sites
    come from the FreeU launch, in another summation order)."""
    dtype = torch.float32
    model = _tiny(dtype, gpu)
    gm = optimize_model(model, cuda_graph=False, freeu=True)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    ref = orc.unet_forward(sd, x["latent"], torch.tensor(500.0), x["encoder_hidden_states"], x["text_embeds"], x["time_ids"])
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    with torch.no_grad():
        out = gm(xg["latent"], torch.tensor(500.0, device=gpu), xg["encoder_hidden_states"],
                 {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0].float().cpu()
    err = float((out - ref).abs().max())
    print(f"tiny fp32 freeu=True neutral vs oracle: {err:.2e}")
    assert err <= ABS_TOL_STRICT


def test_fp8_plan_with_freeu_runs(gpu):
    dtype = torch.bfloat16
    gm = optimize_model(_tiny(dtype, gpu), cuda_graph=False, fp8=True, freeu=True)
    gm.freeu.set(**V)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    xg = {k: v.to(gpu, dtype) for k, v in x.items()}
    with torch.no_grad():
        out = gm(xg["latent"], torch.tensor(500.0, device=gpu), xg["encoder_hidden_states"],
                 {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0]
    assert out.shape == xg["latent"].shape and torch.isfinite(out.float()).all()


# ------------------------------------------------------------------------------------------------ SDXL-base, strict
def test_sdxl_strict_step_with_freeu_vs_cpu_fixture(gpu, sdxl_fp32_pair):
    """SDXL-base fp32 at latent 64, version 1 at the SDXL values, against tests/golden/f1_unet_step_latent64_freeu.npz (the eager
    fp32 module with the hook route on the CPU, tools/make_freeu_golden.py; its own deviation from a float64 run is in the file)."""
    g = golden("f1_unet_step_latent64_freeu")
    ref = torch.from_numpy(g["out"])
    gm = optimize_model(sdxl_fp32_pair[0], cuda_graph=False, freeu=True)
    assert gm.rewrite_stats["freeu_sites"] == 6
    gm.freeu.set(float(g["s1"]), float(g["s2"]), float(g["b1"]), float(g["b2"]), int(g["version"]))
    x = synth.denoise_inputs(1, int(g["latent_hw"]), 1234)
    xg = {k: v.to(gpu) for k, v in x.items()}
    with torch.no_grad():
        out = gm(xg["latent"], torch.tensor(float(g["timestep"]), device=gpu), xg["encoder_hidden_states"],
                 {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0].float().cpu()
    err = float((out - ref).abs().max())
    print(f"SDXL strict step with FreeU: max abs err {err:.2e} (|ref| max {float(ref.abs().max()):.2f}; FreeU moves the plain step by "
          f"{float(g['plain_max_abs_diff']):.2e}; fixture vs float64 {float(g['f64_max_abs_dev']) if 'f64_max_abs_dev' in g.files else float('nan'):.2e})")
    assert float(g["plain_max_abs_diff"]) > 100 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT
