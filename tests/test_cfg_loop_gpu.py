"""Classifier-free guidance inside the captured denoise loop (DenoiseLoop(guidance_scale=...), st_cfg_euler_step).

The kernel against a float64 restatement of diffusers' guidance / rescale_noise_cfg / Euler arithmetic; the TINY network
through every loop mode against the oracle's CFG loop; SDXL-base through the reference's CFG protocol against the committed
goldens (oracle/make_golden.py f3_cfg, f3_cfg_f64; oracle/make_rounded_golden.py f3_cfg)."""
import pytest
import torch

from oracle import unet_oracle as orc
from stabletriton_amd import ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests.util import golden

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
STORAGE_FACTOR = 1.3           # as tests/test_unet_gpu.py: what 16-bit storage alone costs, times 1.3


# ------------------------------------------------------------------------------------------------ the kernel alone
def _guarded(shape, dtype, dev, fill):
    """A channels_last tensor inside a larger buffer whose margins hold `fill`: a write out of bounds shows in the margins."""
    n = 1
    for s in shape:
        n *= s
    pad = 64
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    b, c, h, w = shape
    t = buf[pad:pad + n].view(b, h, w, c).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=torch.channels_last)
    return t, buf, pad


def _restated(lat0, eps, g, phi, ds):
    """float64: e = e_neg + g (e_pos - e_neg); diffusers rescale_noise_cfg (std with correction 1 over C, H, W); Euler."""
    b = lat0.shape[0]
    en, ep = eps[:b].double(), eps[b:].double()
    e = en + g * (ep - en)
    mag = en.abs() + abs(g) * (ep.abs() + en.abs())                  # what the fp32 terms of e are made of
    if phi is not None:
        r = ep.std(dim=(1, 2, 3), keepdim=True) / e.std(dim=(1, 2, 3), keepdim=True)
        e = phi * (e * r) + (1.0 - phi) * e
        mag = mag * (abs(phi) * r + abs(1.0 - phi))
    lat = lat0.double() + e * ds
    return lat, mag * abs(ds) + lat0.double().abs()


# one rounding to the dtype: an ulp relative, and (fp16) the spacing of the subnormals
ROUND = {torch.float32: (2.0 ** -23, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hw", [(16, 16), (128, 128), (152, 104)])
def test_cfg_step_kernel_vs_float64(gpu, dtype, batch, hw):
    tables = euler_discrete_tables(50)
    n = tables.n_steps
    i = 37                                                        # read from the device; every table differs per step
    dsigma = torch.tensor(tables.dsigma(), device=gpu)
    in_scale = torch.tensor(tables.in_scale(), device=gpu)
    guidance = torch.linspace(1.0, 9.0, n, device=gpu)
    step = torch.tensor([i], dtype=torch.int32, device=gpu)
    h, w = hw
    shape = (batch, 4, h, w)
    gen = torch.Generator().manual_seed(7 + batch + h)
    lat0 = (torch.randn(shape, generator=gen) * 3.0).to(gpu).contiguous(memory_format=torch.channels_last)
    eps = torch.randn((2 * batch, 4, h, w), generator=gen)
    eps[batch:] = eps[batch:] * 1.5 + 0.25 * eps[:batch]                  # a positive half that differs in scale from the negative
    eps = eps.to(gpu, dtype).contiguous(memory_format=torch.channels_last)
    g, ds = float(guidance[i]), float(dsigma[i])
    sc = float(in_scale[i + 1])
    results = {}
    for phi in (None, 0.0, 0.7, 1.0):
        rescale = None
        if phi is not None:
            rescale = torch.linspace(0.05, 0.95, n, device=gpu)
            rescale[i] = phi
        outs = []
        for _ in range(2):                                        # two calls on the same inputs: bit-equal
            latent, lat_buf, pad = _guarded(shape, torch.float32, gpu, 1234.5)
            latent.copy_(lat0)
            next_in, nxt_buf, npad = _guarded((2 * batch, 4, h, w), dtype, gpu, -77.0)
            ops.cfg_euler_step(latent, eps, next_in, dsigma, in_scale, guidance, step, rescale=rescale)
            torch.cuda.synchronize()
            for buf, p in ((lat_buf, pad), (nxt_buf, npad)):
                assert torch.all(buf[:p] == buf[0]) and torch.all(buf[-p:] == buf[0]), "write outside the tensor"
            outs.append((latent.clone(), next_in.clone()))
        (lat, nxt), (lat2, nxt2) = outs
        assert torch.equal(lat, lat2) and torch.equal(nxt, nxt2)
        ref, mag = _restated(lat0.cpu(), eps.float().cpu(), g, phi, ds)
        err = (lat.cpu().double() - ref).abs()
        # fp32 rounding: a few units of 2^-24 of the magnitudes the result is computed from
        assert float((err - 8 * 2.0 ** -24 * mag).max()) <= 0.0, f"phi {phi}: max abs err {float(err.max()):.3e}"
        # both halves of the next input bit-equal; each within one rounding of the dtype of the float64 value
        assert torch.equal(nxt[:batch], nxt[batch:])
        want = ref * sc
        e_nxt = (nxt[:batch].cpu().double() - want).abs()
        rel, absolute = ROUND[dtype]
        assert float((e_nxt - rel * want.abs() - absolute - 8 * 2.0 ** -24 * mag * sc).max()) <= 0.0
        if dtype != torch.float16:
            assert torch.equal(nxt[:batch], (lat * sc).to(dtype))       # exactly the fp32 product, rounded once
        # (fp16: hipcc may fuse the product and the conversion into one mixed-precision FMA, v_fma_mix*_f16, which rounds the
        #  exact product once; as euler_kernel does.  Within the one-rounding bound above either way.)
        results[phi] = (lat, nxt)
        print(f"{dtype} B={batch} {hw} phi={phi}: latent max abs err vs float64 {float(err.max()):.2e}")
    assert torch.equal(results[0.0][0], results[None][0]) and torch.equal(results[0.0][1], results[None][1])
    assert not torch.equal(results[0.7][0], results[None][0])


def test_cfg_step_op_rejects_bad_shapes(gpu):
    lat = torch.zeros((1, 4, 16, 16), device=gpu).contiguous(memory_format=torch.channels_last)
    eps = torch.zeros((1, 4, 16, 16), device=gpu, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    tbl = torch.ones(10, device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(ops.BackendError, match="2B"):
        ops.cfg_euler_step(lat, eps, eps, tbl, tbl, tbl, step)
    eps2 = torch.zeros((2, 4, 16, 16), device=gpu, dtype=torch.bfloat16)          # NCHW against a channels_last latent
    with pytest.raises(ops.BackendError, match="layout"):
        ops.cfg_euler_step(lat, eps2, eps2, tbl, tbl, tbl, step)
    eps2 = eps2.contiguous(memory_format=torch.channels_last)
    with pytest.raises(ops.BackendError, match="n_steps"):
        ops.cfg_euler_step(lat, eps2, eps2, tbl, tbl, torch.ones(9, device=gpu), step)


# ------------------------------------------------------------------------------------------------ TINY network
def _tiny(dtype, dev, fp8=False):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m, optimize_model(m, cuda_graph=False, fp8=fp8)


def _tiny_loop(gm, dtype, dev, tables, batch=1, **kw):
    return DenoiseLoop(gm, batch, 16, dtype, dev, tables, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, **kw)


def _condition(loop, x, dtype, dev, neg, pos):
    """Rows `neg` of the synthetic inputs are the negative prompt, rows `pos` the positive one."""
    def rows(k, r):
        return x[k][r].to(dev, dtype)
    loop.set_conditioning(rows("encoder_hidden_states", pos), rows("text_embeds", pos), rows("time_ids", pos),
                          rows("encoder_hidden_states", neg), rows("text_embeds", neg), rows("time_ids", neg))


def _final(loop):
    return loop.latent.contiguous(memory_format=torch.contiguous_format).clone().cpu()


def _restated_loop(sd, x, tables, g, phi=None, init=None, strength=1.0):
    """float64 restatement of the guided loop (diffusers' CFG, rescale_noise_cfg, img2img start) around the oracle's UNet;
    row 0 = negative, row 1 = positive conditioning, one latent."""
    n = tables.n_steps
    t_start = max(n - min(int(n * strength), n), 0)
    if init is None:
        lat = x["latent"][:1].double() * tables.init_noise_sigma
    else:
        lat = init.double() + x["latent"][:1].double() * float(tables.sigmas[t_start])
    in_scale, dsigma = tables.in_scale(), tables.dsigma()
    for i in range(t_start, n):
        x_in = torch.cat([lat, lat]).float() * float(in_scale[i])
        eps2 = orc.unet_forward(sd, x_in, torch.tensor(float(tables.timesteps[i])), x["encoder_hidden_states"][:2],
                                x["text_embeds"][:2], x["time_ids"][:2]).double()
        e = eps2[0:1] + g * (eps2[1:2] - eps2[0:1])
        if phi is not None:
            r = eps2[1:2].std(dim=(1, 2, 3), keepdim=True) / e.std(dim=(1, 2, 3), keepdim=True)
            e = phi * (e * r) + (1.0 - phi) * e
        lat = lat + e * float(dsigma[i])
    return lat


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_tiny_cfg_loop_modes(gpu, dtype):
    m, gm = _tiny(dtype, gpu)
    tables = euler_discrete_tables(10)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    finals = {}
    for mode in ("eager", "step", "loop"):
        loop = _tiny_loop(gm, dtype, gpu, tables, guidance_scale=5.0, mode=mode)
        _condition(loop, x, dtype, gpu, slice(0, 1), slice(1, 2))
        with torch.no_grad():
            finals[mode] = loop.denoise(x["latent"][:1]).cpu()
            again = loop.denoise(x["latent"][:1]).cpu()                # a replay repeats bit for bit
        assert torch.equal(finals[mode], again), mode
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    assert torch.isfinite(finals["loop"]).all()
    if dtype == torch.float32:
        sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
        ref = orc.euler_denoise_cfg(
            lambda xi, t: orc.unet_forward(sd, xi, t, x["encoder_hidden_states"], x["text_embeds"], x["time_ids"]),
            x["latent"][:1], tables, 5.0)
        err = float((finals["loop"] - ref).abs().max())
        print(f"tiny CFG 10-step loop fp32: max abs err vs orc.euler_denoise_cfg {err:.2e} (|ref| max {float(ref.abs().max()):.2f})")
        assert err <= ABS_TOL_STRICT


def test_tiny_cfg_loop_batch_rows_match_single(gpu):
    """B = 2, two prompts (negatives rows 0, 1; positives rows 2, 3): each row is its own B = 1 run."""
    m, gm = _tiny(torch.float32, gpu)
    tables = euler_discrete_tables(10)
    x = synth.denoise_inputs(4, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    loop = _tiny_loop(gm, torch.float32, gpu, tables, batch=2, guidance_scale=5.0, mode="loop")
    _condition(loop, x, torch.float32, gpu, slice(0, 2), slice(2, 4))
    with torch.no_grad():
        both = loop.denoise(x["latent"][:2]).cpu()
    for k in range(2):
        one = _tiny_loop(gm, torch.float32, gpu, tables, guidance_scale=5.0, mode="loop")
        _condition(one, x, torch.float32, gpu, slice(k, k + 1), slice(2 + k, 3 + k))
        with torch.no_grad():
            single = one.denoise(x["latent"][k:k + 1]).cpu()
        err = float((both[k:k + 1] - single).abs().max())
        print(f"tiny CFG B=2 row {k} vs its B=1 run: max abs diff {err:.2e}")
        assert err <= ABS_TOL_STRICT
    assert not torch.equal(both[0], both[1])


@pytest.mark.parametrize("mode", ["step", "eager"])
def test_tiny_cfg_img2img_vs_float64(gpu, mode):
    m, gm = _tiny(torch.float32, gpu)
    tables = euler_discrete_tables(10)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    init = synth.normal("img2img.init", (1, 4, 16, 16), 77) * 0.8
    loop = _tiny_loop(gm, torch.float32, gpu, tables, guidance_scale=5.0, mode=mode)
    _condition(loop, x, torch.float32, gpu, slice(0, 1), slice(1, 2))
    with torch.no_grad():
        left = loop.set_image(init, x["latent"][:1], 0.5)
        assert left == 5
        loop.run_steps(left)
    out = _final(loop)
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    ref = _restated_loop(sd, x, tables, 5.0, init=init, strength=0.5)
    err = float((out.double() - ref).abs().max())
    print(f"tiny CFG img2img (strength 0.5, mode {mode}) fp32: max abs err vs float64 restatement {err:.2e}")
    assert err <= ABS_TOL_STRICT


def test_tiny_cfg_rescale_vs_float64(gpu):
    m, gm = _tiny(torch.float32, gpu)
    tables = euler_discrete_tables(10)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    finals = {}
    for mode in ("step", "loop"):
        loop = _tiny_loop(gm, torch.float32, gpu, tables, guidance_scale=5.0, guidance_rescale=0.7, mode=mode)
        _condition(loop, x, torch.float32, gpu, slice(0, 1), slice(1, 2))
        with torch.no_grad():
            finals[mode] = loop.denoise(x["latent"][:1]).cpu()
            assert torch.equal(finals[mode], loop.denoise(x["latent"][:1]).cpu())
    assert torch.equal(finals["step"], finals["loop"])
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    ref = _restated_loop(sd, x, tables, 5.0, phi=0.7)
    plain = _restated_loop(sd, x, tables, 5.0)
    err = float((finals["loop"].double() - ref).abs().max())
    print(f"tiny CFG rescale 0.7 loop fp32: max abs err vs float64 restatement {err:.2e} "
          f"(the rescale moves the latent by {float((ref - plain).abs().max()):.2e})")
    assert err <= ABS_TOL_STRICT


def test_tiny_cfg_set_guidance_needs_no_recapture(gpu):
    """Capture at g = 5, denoise; set_guidance(7.5) and denoise again with the SAME graph: equal to a loop built at 7.5."""
    _, gm = _tiny(torch.bfloat16, gpu)
    tables = euler_discrete_tables(10)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    loop = _tiny_loop(gm, torch.bfloat16, gpu, tables, guidance_scale=5.0, mode="loop")
    _condition(loop, x, torch.bfloat16, gpu, slice(0, 1), slice(1, 2))
    with torch.no_grad():
        at5 = loop.denoise(x["latent"][:1]).cpu()
        graph = loop.graph
        loop.set_guidance(7.5)
        at75 = loop.denoise(x["latent"][:1]).cpu()
    assert loop.graph is graph and not torch.equal(at5, at75)
    fresh = _tiny_loop(gm, torch.bfloat16, gpu, tables, guidance_scale=7.5, mode="loop")
    _condition(fresh, x, torch.bfloat16, gpu, slice(0, 1), slice(1, 2))
    with torch.no_grad():
        assert torch.equal(at75, fresh.denoise(x["latent"][:1]).cpu())


def test_tiny_cfg_fp8_plan_and_refresh(gpu):
    """fp8 plan (delayed scales re-measured per trajectory) and an in-place weight update (refresh_weights) under guidance."""
    _, gm = _tiny(torch.bfloat16, gpu, fp8=True)
    tables = euler_discrete_tables(8)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    loop = _tiny_loop(gm, torch.bfloat16, gpu, tables, guidance_scale=5.0, mode="step")
    _condition(loop, x, torch.bfloat16, gpu, slice(0, 1), slice(1, 2))
    with torch.no_grad():
        first = loop.denoise(x["latent"][:1]).cpu()
        other = loop.denoise(x["latent"][:1] * 3.0 + 1.0).cpu()
        again = loop.denoise(x["latent"][:1]).cpu()
        assert gm.exec_context.fp8 is not None and gm.exec_context.fp8.sites
        assert torch.isfinite(first).all() and not torch.equal(first, other) and torch.equal(first, again)
        assert loop.refresh_weights() >= 0
        assert torch.equal(first, loop.denoise(x["latent"][:1]).cpu())


# ------------------------------------------------------------------------------------------------ SDXL-base, the reference protocol
def _sdxl_cfg(gm, dtype, dev, mode):
    g = golden("f3_cfg50_latent64")
    x = synth.denoise_inputs(2, 64, 1234)                      # row 0 = negative prompt, row 1 = prompt (oracle/make_golden.py f3_cfg)
    loop = DenoiseLoop(gm, 1, 64, dtype, dev, euler_discrete_tables(50), guidance_scale=float(g["guidance_scale"]), mode=mode)
    _condition(loop, x, dtype, dev, slice(0, 1), slice(1, 2))
    with torch.no_grad():
        return loop.denoise(x["latent"][:1]).cpu()


def test_sdxl_cfg_loop_fp32_strict(gpu, sdxl_fp32):
    out = _sdxl_cfg(sdxl_fp32, torch.float32, gpu, "step")
    g64 = golden("f3_cfg50_latent64_f64")
    bound = max(ABS_TOL_STRICT, 2.0 * float(g64["ref_fp32_max_abs"]))     # tests/test_hooks_gpu.py cfg_strict_bound
    err64 = float((out.double() - torch.from_numpy(g64["final"])).abs().max())
    err = float((out - torch.from_numpy(golden("f3_cfg50_latent64")["final"])).abs().max())
    print(f"SDXL CFG loop fp32 (mode step, 50 steps, g 5): max abs err {err64:.2e} vs the reference's float64 run, {err:.2e} vs its "
          f"fp32 run (bound {bound:.1e})")
    assert err64 <= bound


def test_sdxl_cfg_loop_bf16(gpu, sdxl_bf16):
    out = _sdxl_cfg(sdxl_bf16, torch.bfloat16, gpu, "loop")
    ref = torch.from_numpy(golden("f3_cfg50_latent64")["final"])
    rms = float((out - ref).pow(2).mean().sqrt())
    storage = float(golden("f3_cfg50_latent64_rounded")["bf16_rms"])
    print(f"SDXL CFG loop bf16 (mode loop, fp32 state): final latent rms err {rms:.3e} = {rms / storage:.3f} x the storage-alone "
          f"rms {storage:.3e} (fp16-state protocol), max abs {float((out - ref).abs().max()):.2e}")
    assert torch.isfinite(out).all()
    assert rms <= STORAGE_FACTOR * storage
