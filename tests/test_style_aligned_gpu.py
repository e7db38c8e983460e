"""StyleAligned on the GPU: st_style_adain (csrc/style_adain.hip) per element against float64, st_attention_shared
(csrc/attention_joint.hip) bit for bit against ops.attention on the concatenated keys, and the feature in the captured denoise loop
on the TINY network at latent 32 (its 256-token level takes the attention kernel, the 64-token level ops.attention_shared's slow path;
the AdaIN launches run at both)."""
import functools

import pytest
import torch

from stabletriton_amd import ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel

pytestmark = pytest.mark.gpu
HALF = [torch.bfloat16, torch.float16]
_name = lambda v: str(v).split(".")[-1] if isinstance(v, torch.dtype) else None


def _gate(gpu, value):
    return torch.zeros(1, dtype=torch.int32, device=gpu), torch.full((1,), float(value), dtype=torch.float32, device=gpu)


# fewer tokens than a 256-token slab; a token tail (264 = 256 + 8) with five 128-channel strips and two blocks; a channel tail (136 = 128 + 8)
# with one block of three and a token tail (1000 = 3 * 256 + 232)
@pytest.mark.parametrize("slices", ["qk", "qkv"])
@pytest.mark.parametrize("B,per,T,C", [(2, 2, 8, 64), (4, 2, 264, 640), (3, 3, 1000, 136)])
@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_adain_matches_float64(gpu, dtype, B, per, T, C, slices):
    """Per element: the kernel rounds an fp32 affine x * a + c once, so it may miss the float64 value by 1 ulp of the output type at
    |y_ref|, plus 2^-20 * (|x * a| + |c|) for the fp32 arithmetic where the two terms cancel."""
    g = torch.Generator().manual_seed(1000 * T + C)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    buf = rnd(B, T, 3 * C) * (0.25 + 2.0 * torch.rand(B, 1, 3 * C, generator=g)) + 2.0 * rnd(B, 1, 3 * C)      # per-channel scales and offsets
    buf[:, :, 5] = torch.tensor([1.5, -0.75, 0.5, 2.0][:B]).reshape(B, 1)      # constant along the tokens in every row: var = 0 on both sides
    buf[1:, :, C + 3] = 1.25                                                   # ... and in the other rows only: a = sd_style / sqrt(1e-5)
    buf = buf.to(dtype).to(gpu)
    n = len(slices)
    views = [buf[:, :, i * C:(i + 1) * C] for i in range(n)]
    before = buf.clone()
    ws = ops.style_adain_workspace(B, T, C, n, gpu).fill_(-7.0)
    assert ops.style_adain(views, per, gate=_gate(gpu, 0), workspace=ws)[0] is views[0]
    assert torch.equal(buf, before) and bool((ws == -7.0).all()), "gated off: neither the buffer nor the workspace is touched"
    ops.style_adain(views, per, gate=_gate(gpu, 1), workspace=ws)
    buf, before = buf.cpu(), before.cpu()
    style = torch.arange(B) % per == 0
    assert torch.equal(buf[style], before[style]), "style rows are never written"
    assert torch.equal(buf[:, :, n * C:], before[:, :, n * C:]), "columns outside the slices are never written"
    x = before[:, :, :n * C].double()
    s = torch.arange(B) - torch.arange(B) % per
    mu, sd = x.mean(1, keepdim=True), (x.var(1, unbiased=True, keepdim=True) + 1e-5).sqrt()
    a = sd[s] / sd
    c = mu[s] - mu * a
    want = (x - mu) / sd * sd[s] + mu[s]
    mant = 7 if dtype == torch.bfloat16 else 10
    ulp = torch.exp2((torch.frexp(want.abs())[1] - 1).clamp(min=-14 if mant == 10 else -126).double() - mant)
    bound = ulp + 2.0 ** -20 * ((x * a).abs() + c.abs())
    ratio = ((buf[:, :, :n * C].double() - want).abs() / bound)[~style]
    print(f"style_adain {_name(dtype)} {(B, per, T, C)} {slices}: worst error {float(ratio.max()):.3f} of the per-element bound")
    assert float(ratio.max()) <= 1.0
    assert not torch.equal(buf[~style], before[~style])


SHARED = [(2, 2, 256, 1), (4, 2, 264, 10), (3, 3, 320, 2), (2, 1, 256, 2)]


@functools.lru_cache(maxsize=None)
def _qkv(B, T, H):
    """q, k, v as the UNet has them: column slices of one (B, T, 3 * H * 64) buffer (float32 on the host)."""
    buf = torch.randn(B, T, 3 * H * 64, generator=torch.Generator().manual_seed(100 * T + H))
    return buf


def _slices(buf, H):
    C = H * 64
    return buf[:, :, :C], buf[:, :, C:2 * C], buf[:, :, 2 * C:]


def _expected(q, k, v, H, per):
    """ops.attention, batched at the same B: on the plain keys, and on every row's keys followed by its style row's."""
    B = q.shape[0]
    s = torch.arange(B, device=q.device) - torch.arange(B, device=q.device) % per
    plain = ops.attention(q, k, v, H, 0.125)
    joint = ops.attention(q, torch.cat([k, k[s]], dim=1), torch.cat([v, v[s]], dim=1), H, 0.125)
    return plain, joint, s == torch.arange(B, device=q.device)


@pytest.mark.parametrize("B,per,T,H", SHARED)
@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_shared_attention_equals_attention_on_the_concatenation(gpu, dtype, B, per, T, H):
    q, k, v = _slices(_qkv(B, T, H).to(gpu, dtype), H)
    plain, joint, style = _expected(q, k, v, H, per)
    assert bool(torch.isfinite(joint).all())
    out = ops.attention_shared(q, k, v, H, 0.125, per, fused=True)
    assert torch.equal(out[style], plain[style]), "a style row: the bits of ops.attention on that row"
    assert torch.equal(out[~style], joint[~style]), "another row: the bits of ops.attention on [own keys | style row's keys]"
    assert torch.equal(ops.attention_shared(q, k, v, H, 0.125, per, fused=False), out), "the slow path gives other bits"
    # gated off: ordinary attention, and the style rows' keys and values (NaN in this copy) are never read by the other rows
    poisoned = _qkv(B, T, H).to(gpu, dtype).clone()
    poisoned[style, :, H * 64:] = float("nan")
    qp, kp, vp = _slices(poisoned, H)
    off = ops.attention_shared(qp, kp, vp, H, 0.125, per, gate=_gate(gpu, 0), fused=True)
    assert torch.equal(off[~style], plain[~style])
    assert torch.equal(ops.attention_shared(q, k, v, H, 0.125, per, gate=_gate(gpu, 0), fused=True), plain)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_shared_attention_gate_is_read_at_every_replay(gpu, dtype):
    B, per, T, H = 4, 2, 264, 10
    q, k, v = _slices(_qkv(B, T, H).to(gpu, dtype), H)
    plain, joint, style = _expected(q, k, v, H, per)
    on = torch.where(style.reshape(B, 1, 1), plain, joint)
    step, table = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(2, dtype=torch.float32, device=gpu)
    ops.attention_shared(q, k, v, H, 0.125, per, gate=(step, table))      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attention_shared(q, k, v, H, 0.125, per, gate=(step, table))
    for value, entry, want in ((0.0, 0, plain), (1.0, 0, on), (0.0, 0, plain), (1.0, 0, on), (1.0, 1, plain)):
        table[0] = value
        step.fill_(entry)
        graph.replay()
        assert torch.equal(out, want), f"table[0] = {value}, step {entry}: the captured launch did not follow the gate"


HW, G, LAYERS = 32, 5.0, (".*",)


@functools.lru_cache(maxsize=None)
def _compiled():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to("cuda:0", torch.bfloat16)
    synth.fill_module_(m, 0)
    return optimize_model(m, cuda_graph=False, style_aligned_layers=LAYERS)


def _final(gpu, mode="loop", on=True, then=None, **kw):
    """The final latent (2 images) of a guided 10-step bf16 Euler loop; rows [negative(2) | positive(2)]."""
    dtype = torch.bfloat16
    x = synth.denoise_inputs(2, HW, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    loop = DenoiseLoop(_compiled(), 2, HW, dtype, gpu, euler_discrete_tables(10), cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, mode=mode,
                       guidance_scale=G, **kw)
    loop.set_conditioning(*(x[k].to(gpu, dtype) for k in keys), *(x[k].flip(0).to(gpu, dtype) for k in keys))
    if kw.get("style_aligned"):
        loop.set_style_aligned(0.0, 1.0) if on else loop.set_style_aligned(None)
    with torch.no_grad():
        out = loop.denoise(x["latent"]).cpu() if then is None else then(loop, x["latent"])
    assert _compiled().style_aligned.per == 0 and _compiled().style_aligned.gate is None, "the loop names its blocks around its own calls only"
    return out


@functools.lru_cache(maxsize=None)
def _aligned(gpu):
    return _final(gpu, style_aligned=True)


def test_loop_off_is_the_plain_loop_and_on_moves_image_1_alone(gpu):
    assert _compiled().rewrite_stats["style_aligned_sites"] == 17
    on, plain = _aligned(gpu), _final(gpu)
    assert torch.equal(_final(gpu, style_aligned=True, on=False), plain)
    assert torch.equal(on[0], plain[0]), "image 0, the style image, must not depend on the others"
    assert bool(torch.isfinite(on).all()) and not torch.equal(on[1], plain[1])


def test_window_moves_in_place_and_all_off_captures_the_plain_graph(gpu):
    def then(loop, noise):
        outs, graphs = [], []
        for window in ((0.0, 1.0), (0.0, 0.5), (None,)):      # on; on for the first half: the other steps' sites are gated off; off
            loop.set_style_aligned(*window)
            outs.append(loop.denoise(noise).cpu())
            graphs.append(loop.graph)
        assert graphs[1] is graphs[0] and graphs[2] is not graphs[0]
        return outs
    on, half, off = _final(gpu, style_aligned=True, then=then)
    assert torch.equal(on, _aligned(gpu)) and torch.equal(off, _final(gpu)) and torch.equal(half[0], off[0])
    assert not torch.equal(half[1], on[1]) and not torch.equal(half[1], off[1])


def test_loop_with_the_kernel_equals_the_slow_path_loop(gpu, monkeypatch):
    """torch.equal, as tests/test_reference_loop_gpu.py compares its kernel with its slow path: one launch per site gives the bits of
    the concatenate-and-attend route.  The AdaIN launches run in both loops: at every site ops.style_adain hands back the very q and
    k slices of the fused buffer it was given, which only the in-place HIP path does."""
    shared, adain, in_place = ops.attention_shared, ops.style_adain, []

    def checked(slices, per, **kw):
        out = adain(slices, per, **kw)
        in_place.append(all(o is s for o, s in zip(out, slices)))
        return out

    monkeypatch.setattr(ops, "style_adain", checked)
    monkeypatch.setattr(ops, "attention_shared", lambda *a, **kw: shared(*a, **{**kw, "fused": False}))
    slow = _final(gpu, "eager", style_aligned=True)
    assert len(in_place) == 17 * 10 and all(in_place), "every site of every step takes the AdaIN kernel"
    assert torch.equal(slow[1], _aligned(gpu)[1]) and torch.equal(slow, _aligned(gpu))


def test_loop_and_step_mode_agree(gpu):
    assert torch.equal(_final(gpu, "step", style_aligned=True), _aligned(gpu))


def test_comfy_hook_enable_and_disable(gpu):
    from stabletriton_amd import hooks
    dtype = torch.bfloat16
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(gpu, dtype)
    synth.fill_module_(m, 0)
    adapter = hooks.compile_comfy_unet(m, style_aligned_layers=LAYERS)
    x = {k: v.to(gpu, dtype) for k, v in synth.denoise_inputs(4, HW, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim).items()}
    with torch.no_grad():
        y = torch.cat([x["text_embeds"], m.add_time_proj(x["time_ids"].flatten()).reshape(4, -1).to(dtype)], dim=-1)
    call = lambda: adapter(x["latent"], timesteps=torch.full((4,), 300.0, device=gpu), context=x["encoder_hidden_states"], y=y).clone()
    base = call()
    adapter.enable_style_aligned(2)                          # two blocks of two rows: rows 0 and 2 are style rows
    on = call()
    assert torch.equal(on, call()) and torch.equal(on[0::2], base[0::2]) and bool(torch.isfinite(on).all())
    assert not torch.equal(on[1], base[1]) and not torch.equal(on[3], base[3])
    adapter.enable_style_aligned(3)
    with pytest.raises(ValueError, match="does not divide"):
        call()
    adapter.disable_style_aligned()
    assert torch.equal(call(), base)
