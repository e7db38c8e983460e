"""DPM-Solver++(2M) inside the captured denoise loop (DenoiseLoop with DPMSolverTables, st_dpmpp2m_step).

The kernel against a float64 restatement of the update (scheduler.py states it); the TINY network through every loop mode
against a float64 DPM++ loop around the oracle's UNet; SDXL-base (synthetic weights) with Karras sigmas and guidance against
a float64 restatement driven by the same compiled UNet's eps."""
import math

import pytest
import torch

from oracle import unet_oracle as orc
from stabletriton_amd import ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
ULP = 2.0 ** -24
# one rounding to the dtype: an ulp relative, and (fp16) the spacing of the subnormals
ROUND = {torch.float32: (2.0 ** -23, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24)}


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
    if torch.isnan(buf[0]):
        return bool(torch.isnan(buf[:pad]).all() and torch.isnan(buf[-pad:]).all())
    return bool(torch.all(buf[:pad] == buf[0]) and torch.all(buf[-pad:] == buf[0]))


def _restated_update(lat0, eps, hist0, row, g, phi, second):
    """float64 DPM++(2M) update with the kernel's fp32 coefficient row; returns (x, d, magnitude of x's terms, of d's)."""
    sigma, a, bb, k = (float(v) for v in row)
    b = lat0.shape[0]
    if g is None:
        e = eps.double()
        emag = e.abs()
    else:
        en, ep = eps[:b].double(), eps[b:].double()
        e = en + g * (ep - en)
        emag = en.abs() + abs(g) * (ep.abs() + en.abs())
        if phi is not None:
            r = ep.std(dim=(1, 2, 3), keepdim=True) / e.std(dim=(1, 2, 3), keepdim=True)
            e = phi * (e * r) + (1.0 - phi) * e
            emag = emag * (abs(phi) * r + abs(1.0 - phi))
    x0 = lat0.double()
    d = x0 - sigma * e
    dmag = x0.abs() + sigma * emag
    if second:
        x = a * x0 + bb * ((1.0 + k) * d - k * hist0.double())
        xmag = a * x0.abs() + bb * ((1.0 + k) * dmag + k * hist0.double().abs())
    else:
        x = a * x0 + bb * d
        xmag = a * x0.abs() + bb * dmag
    return x, d, xmag, dmag


def _run_kernel(gpu, lat0, eps, hist0, dtype, coef, in_scale, step, start, guidance, rescale):
    shape = tuple(lat0.shape)
    latent, lat_buf, pad = _guarded(shape, torch.float32, gpu, 1234.5)
    latent.copy_(lat0)
    history, hist_buf, hpad = _guarded(shape, torch.float32, gpu, -4321.0)
    history.copy_(hist0)
    next_in, nxt_buf, npad = _guarded(tuple(eps.shape), dtype, gpu, -77.0)
    ops.dpmpp2m_step(latent, eps, next_in, history, coef, in_scale, step, start, guidance=guidance, rescale=rescale)
    torch.cuda.synchronize()
    for buf, p in ((lat_buf, pad), (hist_buf, hpad), (nxt_buf, npad)):
        assert _margins_intact(buf, p), "write outside the tensor"
    return latent.clone(), history.clone(), next_in.clone()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hw", [(16, 16), (128, 128), (152, 104)])
def test_dpmpp_step_kernel_vs_float64(gpu, dtype, batch, hw):
    tables = dpmpp_2m_tables(25, karras=True)
    n = tables.n_steps
    i = 11                                                        # a second-order step; read from the device
    coef = torch.tensor(tables.coefficients(), device=gpu)
    row = tables.coefficients()[i]
    assert row[3] != 0.0
    in_scale = torch.tensor(tables.in_scale(), device=gpu)
    guidance = torch.linspace(1.0, 9.0, n, device=gpu)
    step = torch.tensor([i], dtype=torch.int32, device=gpu)
    start = torch.zeros(1, dtype=torch.int32, device=gpu)
    h, w = hw
    shape = (batch, 4, h, w)
    gen = torch.Generator().manual_seed(11 + batch + h)
    lat0 = (torch.randn(shape, generator=gen) * 2.0).to(gpu).contiguous(memory_format=torch.channels_last)
    hist0 = (torch.randn(shape, generator=gen) * 1.5).to(gpu).contiguous(memory_format=torch.channels_last)
    eps2 = torch.randn((2 * batch, 4, h, w), generator=gen)
    eps2[batch:] = eps2[batch:] * 1.5 + 0.25 * eps2[:batch]
    eps2 = eps2.to(gpu, dtype).contiguous(memory_format=torch.channels_last)
    eps1 = eps2[batch:].clone().contiguous(memory_format=torch.channels_last)
    g, sc = float(guidance[i]), float(in_scale[i + 1])
    results = {}
    for variant in ("plain", "cfg", 0.0, 0.7):
        guided = variant != "plain"
        phi = variant if isinstance(variant, float) else None
        eps = eps2 if guided else eps1
        rescale = None
        if phi is not None:
            rescale = torch.linspace(0.05, 0.95, n, device=gpu)
            rescale[i] = phi
        args = (gpu, lat0, eps, hist0, dtype, coef, in_scale, step, start, guidance if guided else None, rescale)
        (lat, hist, nxt), (lat2, hist2, nxt2) = _run_kernel(*args), _run_kernel(*args)
        assert torch.equal(lat, lat2) and torch.equal(hist, hist2) and torch.equal(nxt, nxt2), "two calls differ"
        ref, d, xmag, dmag = _restated_update(lat0.cpu(), eps.float().cpu(), hist0.cpu(), row, g if guided else None, phi, True)
        err = (lat.cpu().double() - ref).abs()
        assert float((err - 8 * ULP * xmag).max()) <= 0.0, f"{variant}: latent max abs err {float(err.max()):.3e}"
        e_d = (hist.cpu().double() - d).abs()
        assert float((e_d - 8 * ULP * dmag).max()) <= 0.0, f"{variant}: history max abs err {float(e_d.max()):.3e}"
        want = ref * sc
        rel, absolute = ROUND[dtype]
        halves = (nxt[:batch], nxt[batch:]) if guided else (nxt,)
        for half in halves:
            e_nxt = (half.cpu().double() - want).abs()
            assert float((e_nxt - rel * want.abs() - absolute - 8 * ULP * xmag * sc).max()) <= 0.0
            if dtype != torch.float16:
                assert torch.equal(half, (lat * sc).to(dtype))          # exactly the fp32 product, rounded once
        # (fp16: hipcc may fuse the product and the conversion into one mixed-precision FMA, as in euler_kernel)
        if guided:
            assert torch.equal(nxt[:batch], nxt[batch:])
        results[variant] = (lat, hist, nxt)
        print(f"{dtype} B={batch} {hw} {variant}: latent max abs err vs float64 {float(err.max()):.2e}")
    for t0, t1 in zip(results[0.0], results["cfg"]):
        assert torch.equal(t0, t1)                                 # phi = 0: the unrescaled bits
    assert not torch.equal(results[0.7][0], results["cfg"][0])


@pytest.mark.parametrize("guided", [False, True])
def test_dpmpp_first_order_ignores_history_and_last_step_is_d(gpu, guided):
    tables = dpmpp_2m_tables(10, karras=True)
    n = tables.n_steps
    c = tables.coefficients()
    coef = torch.tensor(c, device=gpu)
    in_scale = torch.tensor(tables.in_scale(), device=gpu)
    guidance = torch.full((n,), 5.0, device=gpu) if guided else None
    shape = (2, 4, 24, 16)
    gen = torch.Generator().manual_seed(5)
    lat0 = torch.randn(shape, generator=gen).to(gpu).contiguous(memory_format=torch.channels_last)
    eps = torch.randn((4 if guided else 2, 4, 24, 16), generator=gen).to(gpu).contiguous(memory_format=torch.channels_last)
    nan_hist = torch.full_like(lat0, float("nan"))
    for i, start_at in ((4, 4), (0, 0), (n - 1, 0)):                # img2img start with k != 0; trajectory start; last step
        step = torch.tensor([i], dtype=torch.int32, device=gpu)
        start = torch.tensor([start_at], dtype=torch.int32, device=gpu)
        lat, hist, nxt = _run_kernel(gpu, lat0, eps, nan_hist, torch.float32, coef, in_scale, step, start, guidance, None)
        assert torch.isfinite(lat).all() and torch.isfinite(hist).all() and torch.isfinite(nxt).all(), (i, start_at)
        ref, d, xmag, _ = _restated_update(lat0.cpu(), eps.cpu(), torch.zeros(shape, dtype=torch.float64), c[i],
                                           5.0 if guided else None, None, False)
        assert float(((lat.cpu().double() - ref).abs() - 8 * ULP * xmag).max()) <= 0.0
        if i == n - 1:
            assert c[i, 1] == 0.0 and c[i, 2] == 1.0
            assert torch.equal(lat, hist)                          # x = d, bit for bit
    # the same step with start elsewhere reads the history (k != 0): a finite history changes the result
    step, start = torch.tensor([4], dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
    first = _run_kernel(gpu, lat0, eps, torch.zeros_like(lat0), torch.float32, coef, in_scale, step,
                        torch.tensor([4], dtype=torch.int32, device=gpu), guidance, None)[0]
    second = _run_kernel(gpu, lat0, eps, torch.ones_like(lat0), torch.float32, coef, in_scale, step, start, guidance, None)[0]
    assert not torch.equal(first, second)


def test_dpmpp_step_op_rejects_bad_arguments(gpu):
    cl = torch.channels_last
    lat = torch.zeros((1, 4, 16, 16), device=gpu).contiguous(memory_format=cl)
    hist = torch.zeros_like(lat)
    eps = torch.zeros((1, 4, 16, 16), device=gpu, dtype=torch.bfloat16).contiguous(memory_format=cl)
    coef, tbl = torch.ones((10, 4), device=gpu), torch.ones(10, device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    with pytest.raises(ops.BackendError, match="2B"):
        ops.dpmpp2m_step(lat, eps, eps, hist, coef, tbl, step, step, guidance=tbl)
    eps2 = torch.zeros((2, 4, 16, 16), device=gpu, dtype=torch.bfloat16).contiguous(memory_format=cl)
    with pytest.raises(ops.BackendError, match="B, ..."):
        ops.dpmpp2m_step(lat, eps2, eps2, hist, coef, tbl, step, step)
    nchw = torch.zeros((1, 4, 16, 16), device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ops.BackendError, match="layout"):
        ops.dpmpp2m_step(lat, nchw, nchw, hist, coef, tbl, step, step)
    with pytest.raises(ops.BackendError, match="layout"):
        ops.dpmpp2m_step(lat, eps, eps, torch.zeros((1, 4, 16, 16), device=gpu), coef, tbl, step, step)
    with pytest.raises(ops.BackendError, match="fp32"):
        ops.dpmpp2m_step(lat, eps, eps, hist.to(torch.bfloat16), coef, tbl, step, step)
    with pytest.raises(ops.BackendError, match=r"\(10, 4\)"):
        ops.dpmpp2m_step(lat, eps, eps, hist, torch.ones((9, 4), device=gpu), tbl, step, step)
    with pytest.raises(ops.BackendError, match="int32"):
        ops.dpmpp2m_step(lat, eps, eps, hist, coef, tbl, step, step.long())
    with pytest.raises(ops.BackendError, match="rescale needs guidance"):
        ops.dpmpp2m_step(lat, eps, eps, hist, coef, tbl, step, step, rescale=tbl)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.dpmpp2m_step(lat.cpu(), eps, eps, hist, coef, tbl, step, step)


# ------------------------------------------------------------------------------------------------ TINY network
def _tiny(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m, optimize_model(m, cuda_graph=False)


def _tiny_loop(gm, dtype, dev, tables, batch=1, **kw):
    return DenoiseLoop(gm, batch, 16, dtype, dev, tables, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, **kw)


def _condition(loop, x, dtype, dev, pos, neg=None):
    """Rows `pos` of the synthetic inputs are the prompt; rows `neg`, with guidance, the negative prompt."""
    def rows(k, r):
        return x[k][r].to(dev, dtype)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    if neg is None:
        loop.set_conditioning(*(rows(k, pos) for k in keys))
    else:
        loop.set_conditioning(*(rows(k, pos) for k in keys), *(rows(k, neg) for k in keys))


def _final(loop):
    return loop.latent.contiguous(memory_format=torch.contiguous_format).clone().cpu()


def _dpm_coefficients64(sigmas):
    """float64 [sigma, a, b, k] per step from the stored sigmas, k = 0 marking the table's first-order rows."""
    s = [float(v) for v in sigmas]
    n = len(s) - 1
    rows = []
    for i in range(n):
        if s[i + 1] == 0.0:
            rows.append((s[i], 0.0, 1.0, 0.0))
            continue
        h = math.log(s[i]) - math.log(s[i + 1])
        k = 0.0 if i == 0 else 1.0 / (2.0 * ((math.log(s[i - 1]) - math.log(s[i])) / h))
        rows.append((s[i], s[i + 1] / s[i], -math.expm1(-h), k))
    return rows


def _dpm_update64(lat, e, prev, row, first):
    sigma, a, b, k = row
    d = lat - sigma * e
    if first or k == 0.0:
        return a * lat + b * d, d
    return a * lat + b * ((1.0 + k) * d - k * prev), d


def _restated_loop(sd, x, tables, g=None, init=None, strength=1.0, rows=slice(1, 2), neg=slice(0, 1)):
    """float64 DPM++(2M) loop around the oracle's UNet: noise row 0, the prompt in `rows`, with g diffusers' CFG against the
    negative prompt in `neg`; with `init` the img2img start, whose first step is first-order."""
    n = tables.n_steps
    t_start = max(n - min(int(n * strength), n), 0)
    noise = x["latent"][:1].double()
    lat = noise * tables.init_noise_sigma if init is None else init.double() + noise * float(tables.sigmas[t_start])
    coef, in_scale = _dpm_coefficients64(tables.sigmas), tables.in_scale()
    ehs, te, ti = (x[k][rows] for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    if g is not None:
        ehs, te, ti = (torch.cat([x[k][neg], x[k][rows]]) for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    prev = None
    for i in range(t_start, n):
        t = torch.tensor(float(tables.timesteps[i]))
        if g is None:
            e = orc.unet_forward(sd, lat.float() * float(in_scale[i]), t, ehs, te, ti).double()
        else:
            e2 = orc.unet_forward(sd, torch.cat([lat, lat]).float() * float(in_scale[i]), t, ehs, te, ti).double()
            e = e2[:1] + g * (e2[1:] - e2[:1])
        lat, prev = _dpm_update64(lat, e, prev, coef[i], i == t_start)
    return lat


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("cfg", [False, True])
def test_tiny_dpmpp_loop_modes(gpu, dtype, karras, cfg):
    m, gm = _tiny(dtype, gpu)
    tables = dpmpp_2m_tables(10, karras=karras)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    kw = dict(guidance_scale=5.0) if cfg else {}
    finals = {}
    for mode in ("eager", "step", "loop"):
        loop = _tiny_loop(gm, dtype, gpu, tables, mode=mode, **kw)
        _condition(loop, x, dtype, gpu, slice(1, 2), slice(0, 1) if cfg else None)
        with torch.no_grad():
            finals[mode] = loop.denoise(x["latent"][:1]).cpu()
            again = loop.denoise(x["latent"][:1]).cpu()            # a replay repeats bit for bit
        assert torch.equal(finals[mode], again), mode
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    assert torch.isfinite(finals["loop"]).all()
    if dtype == torch.float32:
        sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
        ref = _restated_loop(sd, x, tables, 5.0 if cfg else None)
        err = float((finals["loop"].double() - ref).abs().max())
        print(f"tiny DPM++(2M) 10-step loop fp32 karras={karras} cfg={cfg}: max abs err vs float64 restatement {err:.2e} "
              f"(|ref| max {float(ref.abs().max()):.2f})")
        assert err <= ABS_TOL_STRICT


@pytest.mark.parametrize("mode", ["step", "eager"])
@pytest.mark.parametrize("cfg", [False, True])
def test_tiny_dpmpp_img2img_vs_float64(gpu, mode, cfg):
    m, gm = _tiny(torch.float32, gpu)
    tables = dpmpp_2m_tables(10, karras=True)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    init = synth.normal("img2img.init", (1, 4, 16, 16), 77) * 0.8
    loop = _tiny_loop(gm, torch.float32, gpu, tables, mode=mode, **(dict(guidance_scale=5.0) if cfg else {}))
    _condition(loop, x, torch.float32, gpu, slice(1, 2), slice(0, 1) if cfg else None)
    with torch.no_grad():
        loop.denoise(x["latent"][1:2] * 2.0)                       # a trajectory before: its history must not leak in
        left = loop.set_image(init, x["latent"][:1], 0.5)
        assert left == 5 and int(loop.start) == 5
        loop.run_steps(left)
    out = _final(loop)
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    ref = _restated_loop(sd, x, tables, 5.0 if cfg else None, init=init, strength=0.5)
    err = float((out.double() - ref).abs().max())
    print(f"tiny DPM++(2M) img2img (strength 0.5, mode {mode}, cfg={cfg}) fp32: max abs err vs float64 restatement {err:.2e}")
    assert err <= ABS_TOL_STRICT


def test_tiny_dpmpp_batch_rows_match_single(gpu):
    """B = 2, two prompts: each row is its own B = 1 run."""
    _, gm = _tiny(torch.float32, gpu)
    tables = dpmpp_2m_tables(10, karras=True)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    loop = _tiny_loop(gm, torch.float32, gpu, tables, batch=2, mode="loop")
    _condition(loop, x, torch.float32, gpu, slice(0, 2))
    with torch.no_grad():
        both = loop.denoise(x["latent"][:2]).cpu()
    for k in range(2):
        one = _tiny_loop(gm, torch.float32, gpu, tables, mode="loop")
        _condition(one, x, torch.float32, gpu, slice(k, k + 1))
        with torch.no_grad():
            single = one.denoise(x["latent"][k:k + 1]).cpu()
        err = float((both[k:k + 1] - single).abs().max())
        print(f"tiny DPM++ B=2 row {k} vs its B=1 run: max abs diff {err:.2e}")
        assert err <= ABS_TOL_STRICT
    assert not torch.equal(both[0], both[1])


def test_tiny_dpmpp_and_euler_loops_share_a_module(gpu):
    """A DPM++ loop and an Euler loop over the same compiled module, run in turn: each repeats the bits it gives alone."""
    _, gm = _tiny(torch.bfloat16, gpu)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    dt = torch.bfloat16

    def make(tables, **kw):
        lp = _tiny_loop(gm, dt, gpu, tables, mode="loop", **kw)
        _condition(lp, x, dt, gpu, slice(1, 2), slice(0, 1) if kw else None)
        return lp

    with torch.no_grad():
        dpm = make(dpmpp_2m_tables(10, karras=True), guidance_scale=5.0)
        solo_dpm = dpm.denoise(x["latent"][:1]).cpu()
        eu = make(euler_discrete_tables(10))
        solo_eu = eu.denoise(x["latent"][:1]).cpu()
        for _ in range(2):
            assert torch.equal(dpm.denoise(x["latent"][:1]).cpu(), solo_dpm)
            assert torch.equal(eu.denoise(x["latent"][:1]).cpu(), solo_eu)
    assert not torch.equal(solo_dpm, solo_eu)


# ------------------------------------------------------------------------------------------------ SDXL-base, synthetic weights
def _sdxl_loop(gm, dtype, dev, latent, mode, x):
    loop = DenoiseLoop(gm, 1, latent, dtype, dev, dpmpp_2m_tables(25, karras=True), guidance_scale=5.0, mode=mode)
    _condition(loop, x, dtype, dev, slice(1, 2), slice(0, 1))
    return loop


def test_sdxl_dpmpp_karras_cfg_fp32_strict(gpu, sdxl_fp32):
    """The captured 25-step loop against a float64 restatement of the update driven step by step (mode eager) by the same
    compiled UNet's eps."""
    x = synth.denoise_inputs(2, 64, 1234)
    loop = _sdxl_loop(sdxl_fp32, torch.float32, gpu, 64, "loop", x)
    ev = _sdxl_loop(sdxl_fp32, torch.float32, gpu, 64, "eager", x)
    tables = loop.tables
    coef, in_scale = _dpm_coefficients64(tables.sigmas), tables.in_scale()
    with torch.no_grad():
        out = loop.denoise(x["latent"][:1]).cpu().double()
        lat = x["latent"][:1].double() * tables.init_noise_sigma
        prev = None
        for i in range(tables.n_steps):
            ev.x_in.copy_(torch.cat([lat, lat]).float().mul_(float(in_scale[i])).to(gpu))
            row = tuple(tbl[i] for tbl in ev.time_tables) if ev._tsplit else None
            e2 = ev._unet(ev.timesteps[i], row).double().cpu()
            e = e2[:1] + 5.0 * (e2[1:] - e2[:1])
            lat, prev = _dpm_update64(lat, e, prev, coef[i], i == 0)
    err = float((out - lat).abs().max())
    print(f"SDXL DPM++(2M) Karras 25 steps CFG 5 fp32 (mode loop): max abs err {err:.2e} vs the float64 restatement of the "
          f"update (|ref| max {float(lat.abs().max()):.2f})")
    assert torch.isfinite(out).all()
    assert err <= ABS_TOL_STRICT


def test_sdxl_dpmpp_karras_cfg_bf16_1024(gpu, sdxl_bf16):
    x = synth.denoise_inputs(2, 128, 1234)
    finals = {}
    with torch.no_grad():
        for mode in ("loop", "step"):
            finals[mode] = _sdxl_loop(sdxl_bf16, torch.bfloat16, gpu, 128, mode, x).denoise(x["latent"][:1]).cpu()
    assert torch.equal(finals["loop"], finals["step"])
    assert torch.isfinite(finals["loop"]).all()
    print(f"SDXL DPM++(2M) Karras 25 steps CFG 5 bf16 1024 px: |final| max {float(finals['loop'].abs().max()):.2f}")
