"""T2I-Adapter residual sites on the GPU: the kernel alone in guarded buffers against float64, then the compiled TINY network and one
SDXL-base step against the EAGER module with forward hooks at the four places (tests/t2i_util.py) - never the compiled module.

Bounds.  Kernel: one rounding to the type (the ROUND table of tests/test_dpmpp_loop_gpu.py) plus 2 * 2^-24 (|x| + |s f|) for the fp32
fma; every partial within rows_per_tile * 2^-24 * sum|y| (sum y^2) of the float64 sums of the STORED values - the worst case of
any fp32 summation order over that many terms.  Networks: fp32 the project's strict 1e-3; bf16 / fp16 the TINY step gates of
tests/test_unet_gpu.py (0.1 / 0.025) times max|ref with residuals| / max|ref plain| where the residuals enlarge the output."""
import math

import pytest
import torch

from stabletriton_amd import ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import freeu_util as FU
from tests import t2i_util as TU
from tests.util import rounded

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
ULP = 2.0 ** -24
ROUND = {torch.float32: (2.0 ** -23, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24)}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
# (rows, C, H, W), the batch B of the row blocks, rows per statistics tile (a divisor of H * W, as a producer's tiles are)
SHAPES = [((1, 32, 4, 4), 1, 16), ((3, 320, 32, 32), 1, 256), ((2, 1280, 8, 8), 1, 64), ((2, 64, 38, 26), 1, 76), ((6, 64, 6, 6), 2, 12)]
TABLE = [0.0, 1.25, -0.7]          # the scale is read at a non-zero step index; entry 0 is "off"


# ------------------------------------------------------------------------------------------------ the kernel alone
def _guarded(shape, dtype, dev, fill):
    """A channels_last tensor inside a larger buffer whose margins hold `fill`: a write out of bounds shows in the margins."""
    n = math.prod(shape)
    pad = 64
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    b, c, h, w = shape
    t = buf[pad:pad + n].view(b, h, w, c).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=torch.channels_last)
    return t, buf, pad


def _margins_intact(buf, pad):
    return bool(torch.all(buf[:pad] == buf[0]) and torch.all(buf[-pad:] == buf[0]))


def _guarded_stats(tiles, C, dev, rows):
    pad = 64
    buf = torch.full((tiles * C * 2 + 2 * pad,), -5.5, dtype=torch.float32, device=dev)
    view = buf[pad:pad + tiles * C * 2].view(tiles, C, 2)
    view.copy_(synth.normal("t2i.stats", (tiles, C, 2), 3).to(dev))       # "the producer's" values: what scale 0 must keep
    return ops.ColStats(view, rows, C), buf, pad


def _launch(gpu, dtype, shape, f_rows, srows, step, with_stats=True):
    rows, C, H, W = shape
    x0 = synth.normal("t2i.x", shape, 11).to(dtype)
    f0 = (synth.normal("t2i.f", (f_rows,) + shape[1:], 12) * 0.8).to(dtype)
    x, xbuf, xpad = _guarded(shape, dtype, gpu, 77.0)
    x.copy_(x0.to(gpu))
    f = f0.to(gpu).contiguous(memory_format=torch.channels_last)
    table = torch.tensor(TABLE, dtype=torch.float32, device=gpu)
    st = torch.tensor([step], dtype=torch.int32, device=gpu)
    stats = sbuf = spad = before = None
    if with_stats:
        stats, sbuf, spad = _guarded_stats(rows * H * W // srows, C, gpu, srows)
        before = stats.buf.clone()
    xv = x._version
    ret = ops.residual_add(x, f, table, st, stats)
    torch.cuda.synchronize()
    assert x._version == xv, "the launch writes through the raw pointer"
    assert _margins_intact(xbuf, xpad) and (sbuf is None or _margins_intact(sbuf, spad))
    assert (ret is stats) if with_stats else ret is None
    return x0, f0, x.cpu(), None if stats is None else stats.buf.cpu(), None if before is None else before.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,batch,srows", SHAPES)
def test_kernel_vs_float64(gpu, dtype, shape, batch, srows):
    rows, C, H, W = shape
    rel, absr = ROUND[dtype]
    for f_rows in sorted({1, batch, rows}):
        for step in (1, 2):
            s = float(torch.tensor(TABLE, dtype=torch.float32)[step])
            x0, f0, y, stats, _ = _launch(gpu, dtype, shape, f_rows, srows, step)
            fx = f0.double().repeat(rows // f_rows, 1, 1, 1)              # row n reads f[n % f_rows]
            want = x0.double() + s * fx
            mag = x0.double().abs() + abs(s) * fx.abs()
            err = (y.double() - want).abs()
            bound = rel * want.abs() + absr + 2 * ULP * mag
            worst = float((err / bound.clamp_min(1e-300)).max())
            print(f"{dtype} {shape} f_rows={f_rows} s={s}: max abs err {float(err.max()):.2e}, {worst:.2f} of the bound")
            assert bool((err <= bound).all())
            # the partials: float64 sums of the values as stored, per tile of `srows` consecutive pixel rows and per channel
            yt = y.double().permute(0, 2, 3, 1).reshape(rows * H * W // srows, srows, C)
            for k, v in ((0, yt), (1, yt * yt)):
                e = (stats[:, :, k].double() - v.sum(1)).abs()
                b = srows * ULP * v.abs().sum(1)
                print(f"    partial {('sum', 'sum of squares')[k]}: {float((e / b.clamp_min(1e-300)).max()):.3f} of the bound")
                assert bool((e <= b).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,batch,srows", SHAPES)
def test_kernel_scale_zero_writes_nothing_and_two_launches_agree(gpu, dtype, shape, batch, srows):
    x0, _, y, stats, before = _launch(gpu, dtype, shape, batch, srows, 0)
    assert torch.equal(y, x0) and torch.equal(stats, before), "s == 0 leaves x and the statistics bit-identical"
    a = _launch(gpu, dtype, shape, batch, srows, 2)
    b = _launch(gpu, dtype, shape, batch, srows, 2)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), "two launches give the same bits"
    assert not torch.equal(a[2], x0) and not torch.equal(a[3], a[4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_kernel_without_statistics_and_step_clamp(gpu, dtype):
    for shape, batch, srows in SHAPES:
        x0, f0, y, _, _ = _launch(gpu, dtype, shape, batch, srows, 1, with_stats=False)
        with_stats = _launch(gpu, dtype, shape, batch, srows, 1)
        assert torch.equal(y, with_stats[2]), "the statistics pointer does not change what is stored"
        assert torch.equal(_launch(gpu, dtype, shape, batch, srows, 7, with_stats=False)[2],
                           _launch(gpu, dtype, shape, batch, srows, 2, with_stats=False)[2]), "a step past the table reads its last entry"


def test_launcher_fallback_and_rejections(gpu):
    table = torch.tensor(TABLE, device=gpu)
    step = torch.tensor([1], dtype=torch.int32, device=gpu)
    cl = torch.channels_last
    # not a whole number of 16-byte vectors, and NCHW-contiguous: torch's add, no statistics
    for shape, fmt in (((2, 36, 4, 4), cl), ((2, 64, 4, 4), torch.contiguous_format)):
        x0 = synth.normal("t2i.fb.x", shape, 1).to(gpu, torch.bfloat16).contiguous(memory_format=fmt)
        f = synth.normal("t2i.fb.f", (1,) + shape[1:], 2).to(gpu, torch.bfloat16).contiguous(memory_format=cl)
        x = x0.clone(memory_format=torch.preserve_format)
        st = ops.ColStats(torch.zeros(2, shape[1], 2, device=gpu), 16, shape[1])
        assert ops.residual_add(x, f, table, step, st) is None
        want = (x0.float() + (f.float() * 1.25).to(torch.bfloat16).float()).to(torch.bfloat16)
        assert torch.equal(x, want)
    x = torch.zeros(2, 64, 4, 4, device=gpu).contiguous(memory_format=cl)
    with pytest.raises(ops.BackendError, match="f_rows a divisor of rows"):
        ops.residual_add(x, torch.zeros(3, 64, 4, 4, device=gpu), table, step)
    with pytest.raises(ops.BackendError, match="one dtype"):
        ops.residual_add(x, torch.zeros(1, 64, 4, 4, device=gpu, dtype=torch.bfloat16), table, step)
    with pytest.raises(ops.BackendError, match="int32"):
        ops.residual_add(x, torch.zeros(1, 64, 4, 4, device=gpu), table, step.long())
    with pytest.raises(ops.BackendError, match="fp32"):
        ops.residual_add(x, torch.zeros(1, 64, 4, 4, device=gpu), table.double(), step)
    # statistics that do not fit the shape are not handed on (the GroupNorm behind makes its own pass)
    bad = ops.ColStats(torch.zeros(2, 64, 2, device=gpu), 5, 64)
    assert ops.residual_add(x, torch.ones(1, 64, 4, 4, device=gpu), table, step, bad) is None and float(x.mean()) == 1.25


def test_strict_split_image_of_the_old_values_is_dropped(gpu):
    """A producer's split image of x is honoured by address and version; the in-place add changes neither, so the launcher drops
    the note: the conv behind the site must read the new values."""
    x = synth.normal("t2i.split.x", (1, 64, 8, 8), 1).to(gpu).contiguous(memory_format=torch.channels_last)
    w, b = torch.ones(64, device=gpu), torch.zeros(64, device=gpu)
    y = ops.group_norm(x, 32, w, b, 1e-5, True)                       # fp32 NHWC: leaves its split image and notes it
    assert any(ent[1] == y.data_ptr() for ent in ops._split_notes(gpu)), "this check needs a producer's note to mean anything"
    f = synth.normal("t2i.split.f", (1, 64, 8, 8), 2).to(gpu).contiguous(memory_format=torch.channels_last)
    ops.residual_add(y, f, torch.tensor([1.0], device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
    assert not any(ent[1] == y.data_ptr() for ent in ops._split_notes(gpu))
    cw = synth.normal("t2i.split.w", (32, 64, 3, 3), 3).to(gpu).contiguous(memory_format=torch.channels_last)
    got = ops.conv2d(y, cw, None, 1, 1)
    want = ops.conv2d(y.clone(memory_format=torch.preserve_format), cw, None, 1, 1)
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ TINY UNet step
def _tiny(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m


def _step(gm, x, dev, dtype):
    xg = {k: v.to(dev, dtype) for k, v in x.items()}
    with torch.no_grad():
        return gm(xg["latent"], torch.tensor(500.0, device=dev), xg["encoder_hidden_states"],
                  {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0]


def _ref64(model, x, dtype, feats, scale, freeu=None):
    """The float64 CPU eager module on the weights, inputs and features the kernels see: (plain, hooked at `scale`)."""
    m64 = UNet2DConditionModel(TINY).eval().requires_grad_(False).double()
    m64.load_state_dict({k: v.detach().double().cpu() for k, v in model.state_dict().items()})
    xi = {k: rounded(v, dtype).double() for k, v in x.items()}
    f64 = [rounded(f, dtype).double() for f in feats]
    call = lambda: m64(xi["latent"], torch.tensor(500.0), xi["encoder_hidden_states"], {"text_embeds": xi["text_embeds"], "time_ids": xi["time_ids"]})[0]
    with torch.no_grad():
        plain = call()
        with TU.hooked(m64, f64, scale):
            if freeu is None:
                return plain, call()
            with FU.hooked(m64, **freeu):
                return plain, call()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tiny_sites_at_scale_zero_are_the_module_without_sites(gpu, dtype):
    model = _tiny(dtype, gpu)
    plain = optimize_model(model, cuda_graph=False)
    gm = optimize_model(model, cuda_graph=False, t2i_adapter=True)
    assert gm.rewrite_stats["t2i_adapter_sites"] == 4
    assert {k: v for k, v in gm.rewrite_stats.items() if k != "t2i_adapter_sites"} == dict(plain.rewrite_stats)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    gm.t2i_adapter.bind(2, 16, gpu)
    want = _step(plain, x, gpu, dtype)
    assert torch.equal(_step(gm, x, gpu, dtype), want), "after bind"
    gm.t2i_adapter.set([f.to(gpu) for f in TU.features(TINY, 16)], 0.0)
    assert torch.equal(_step(gm, x, gpu, dtype), want), "features set, scale 0"
    gm.t2i_adapter.set_scale(0.7)
    assert not torch.equal(_step(gm, x, gpu, dtype), want)
    gm.t2i_adapter.clear()
    assert torch.equal(_step(gm, x, gpu, dtype), want), "after clear"


@pytest.mark.parametrize("hw", [16, (24, 16)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_tiny_step_vs_float64_hooked_eager_module(gpu, dtype, hw):
    model = _tiny(dtype, gpu)
    gm = optimize_model(model, cuda_graph=False, t2i_adapter=True)
    x = synth.denoise_inputs(2, hw, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    feats = TU.features(TINY, hw, rows=2)
    plain, ref = _ref64(model, x, dtype, feats, 0.7)
    moved = float((ref - plain).abs().max())
    assert moved > 100 * ABS_TOL_STRICT, "the residuals must matter for this check to mean anything"
    gm.t2i_adapter.bind(2, hw, gpu)
    gm.t2i_adapter.set([f.to(gpu) for f in feats], 0.7)
    base = {torch.float32: ABS_TOL_STRICT, torch.bfloat16: 0.1, torch.float16: 0.025}[dtype]
    gate = base if dtype == torch.float32 else base * max(1.0, float(ref.abs().max() / plain.abs().max()))
    err = float((_step(gm, x, gpu, dtype).double().cpu() - ref).abs().max())
    print(f"tiny {dtype} latent {hw} T2I sites at 0.7: max abs err vs float64 hooked eager {err:.2e} (gate {gate:.2e}; |ref| max "
          f"{float(ref.abs().max()):.2f}; the residuals move the output by {moved:.2f})")
    assert err <= gate


def test_tiny_step_with_freeu_compiled_in(gpu):
    """FreeU's sites read skip tensors that carry the residual."""
    dtype = torch.float32
    model = _tiny(dtype, gpu)
    gm = optimize_model(model, cuda_graph=False, t2i_adapter=True, freeu=True)
    assert gm.rewrite_stats["t2i_adapter_sites"] == 4 and gm.rewrite_stats["freeu_sites"] == 6 and gm.rewrite_stats["skip_cats_removed"] == 9
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    feats = TU.features(TINY, 16)
    _, ref = _ref64(model, x, dtype, feats, 0.7, freeu=dict(FU.SDXL_VALUES, version=1))
    gm.t2i_adapter.bind(2, 16, gpu, feature_rows=1)
    gm.t2i_adapter.set([f.to(gpu) for f in feats], 0.7)
    gm.freeu.set(**FU.SDXL_VALUES, version=1)
    err = float((_step(gm, x, gpu, dtype).double().cpu() - ref).abs().max())
    print(f"tiny fp32 T2I sites at 0.7 + FreeU: max abs err vs the float64 eager module with both hook sets {err:.2e}")
    assert err <= ABS_TOL_STRICT


def test_unbound_and_mismatched_buffers_say_what_to_do(gpu):
    gm = optimize_model(_tiny(torch.bfloat16, gpu), cuda_graph=False, t2i_adapter=True)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    with pytest.raises(ValueError, match=r"t2i_adapter.bind\(rows, latent_hw, device\)"):
        _step(gm, x, gpu, torch.bfloat16)
    gm.t2i_adapter.bind(2, 16, gpu, dtype=torch.float32)
    with pytest.raises(ValueError, match="the activation is torch.bfloat16"):
        _step(gm, x, gpu, torch.bfloat16)
    with pytest.raises(ValueError, match="fp8"):
        optimize_model(_tiny(torch.bfloat16, gpu), cuda_graph=False, t2i_adapter=True, fp8=True)


# ------------------------------------------------------------------------------------------------ SDXL widths
def test_sdxl_strict_step_vs_the_hooked_eager_module(gpu, sdxl_fp32_pair):
    """SDXL-base fp32, one step at latent 32 (sites of 320 / 640 / 1280 / 1280 channels at 16 x 16 and 8 x 8), against the session's
    eager fp32 module with the four forward hooks, on the GPU."""
    from stabletriton_amd.unet import SDXL_BASE
    eager = sdxl_fp32_pair[0]
    gm = optimize_model(eager, cuda_graph=False, t2i_adapter=True)
    assert gm.rewrite_stats["t2i_adapter_sites"] == 4 and gm.t2i_adapter.channels == (320, 640, 1280, 1280)
    x = synth.denoise_inputs(1, 32, 1234)
    xg = {k: v.to(gpu) for k, v in x.items()}
    feats = [f.to(gpu) for f in TU.features(SDXL_BASE, 32)]
    call = lambda m: m(xg["latent"], torch.tensor(500.0, device=gpu), xg["encoder_hidden_states"],
                       {"text_embeds": xg["text_embeds"], "time_ids": xg["time_ids"]})[0].float().cpu()
    with torch.no_grad():
        plain = call(eager)
        with TU.hooked(eager, feats, 0.7):
            ref = call(eager)
        assert not eager.mid_block._forward_hooks, "the shared eager module keeps no hook"
        gm.t2i_adapter.bind(1, 32, gpu)
        assert float((call(gm) - plain).abs().max()) <= ABS_TOL_STRICT
        gm.t2i_adapter.set(feats, 0.7)
        out = call(gm)
    moved = float((ref - plain).abs().max())
    err = float((out - ref).abs().max())
    print(f"SDXL strict step with T2I sites at 0.7: max abs err vs the hooked eager module {err:.2e} (|ref| max {float(ref.abs().max()):.2f}; "
          f"the residuals move the step by {moved:.2e})")
    assert moved > 100 * ABS_TOL_STRICT
    assert err <= ABS_TOL_STRICT
