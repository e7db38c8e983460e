"""Euler ancestral and DPM++ 2M SDE inside the captured denoise loop (DenoiseLoop with SDETables, st_sde_step), and the
counter-based generator (st_philox_normal).

The generator against its float64 restatement (rng.py); the update kernel against a float64 restatement driven by the same
noise; the TINY network through every loop mode against a float64 loop around the oracle's UNet; SDXL-base (synthetic
weights) with DPM++ 2M SDE Karras and guidance against a float64 restatement driven by the same compiled UNet's eps."""
import math

import numpy as np
import pytest
import torch

from oracle import unet_oracle as orc
from stabletriton_amd import ops, rng, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.pipeline import DenoiseLoop
from stabletriton_amd.scheduler import (dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_ancestral_tables,
                                        euler_discrete_tables)
from stabletriton_amd.unet import TINY, UNet2DConditionModel

pytestmark = pytest.mark.gpu
ABS_TOL_STRICT = 1e-3
ULP = 2.0 ** -24
Z_TOL = 4e-6                    # a few fp32 ulps of logf, sqrtf and sincospif, relative to max(1, |z|)
ROUND = {torch.float32: (2.0 ** -23, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24)}
SAMPLERS = {"euler_a": euler_ancestral_tables, "dpmpp_2m_sde": dpmpp_2m_sde_tables}


def _seeds(vals, dev):
    return torch.tensor([v - (1 << 64) if v >= 1 << 63 else v for v in vals], dtype=torch.int64, device=dev)


def _unit(seeds, counter, shape):
    """The stream as a float64 (B, 4, H, W) tensor laid out as a channels_last latent: j = (h W + w) 4 + c."""
    b, c, h, w = shape
    z = rng.normal(seeds, counter, c * h * w)
    return torch.from_numpy(z).view(b, h, w, c).permute(0, 3, 1, 2)


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


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("hw", [16, 128])
@pytest.mark.parametrize("counter", [0, 1, 50])
def test_philox_normal_vs_restatement(gpu, hw, counter):
    seeds = [0, 1 << 32, (1 << 64) - 1] + [int(v) for v in np.random.default_rng(hw + counter).integers(0, 1 << 63, 2)]
    shape = (len(seeds), 4, hw, hw)
    out, buf, pad = _guarded(shape, torch.float32, gpu, -55.0)
    sd = _seeds(seeds, gpu)
    ops.philox_normal(out, sd, counter)
    torch.cuda.synchronize()
    assert _margins_intact(buf, pad), "write outside the tensor"
    got = out.cpu().double()
    want = _unit(seeds, counter, shape)
    err = (got - want).abs() / want.abs().clamp(min=1.0)
    print(f"philox_normal {hw}x{hw} counter {counter}: max err / max(1, |z|) {float(err.max()):.2e}")
    assert float(err.max()) <= Z_TOL
    again = torch.empty_like(out)
    ops.philox_normal(again, sd, counter)
    assert torch.equal(again, out)
    # a contiguous (NCHW) tensor takes the same stream in its own memory order
    flat = torch.empty(shape, device=gpu)
    ops.philox_normal(flat, sd, counter)
    z = rng.normal(seeds, counter, 4 * hw * hw).reshape(shape)
    assert float(((flat.cpu().double() - torch.from_numpy(z)).abs() / torch.from_numpy(z).abs().clamp(min=1.0)).max()) <= Z_TOL


# ------------------------------------------------------------------------------------------------ the kernel alone
def _restated_update(lat0, eps, hist0, row, g, phi, second, z):
    """float64 update with the kernel's fp32 row [sigma, a, b, k, c] and noise z; returns (x, d, |x| terms, |d| terms)."""
    sigma, a, bb, k, c = (float(v) for v in row)
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
    x = x + c * z
    xmag = xmag + abs(c) * z.abs() + abs(c) * Z_TOL / ULP * z.abs().clamp(min=1.0)     # the noise's own error, in ulps
    return x, d, xmag, dmag


def _run_kernel(gpu, lat0, eps, hist0, dtype, coef, in_scale, step, start, seeds, guidance, rescale):
    shape = tuple(lat0.shape)
    latent, lat_buf, pad = _guarded(shape, torch.float32, gpu, 1234.5)
    latent.copy_(lat0)
    history, hist_buf, hpad = _guarded(shape, torch.float32, gpu, -4321.0)
    history.copy_(hist0)
    next_in, nxt_buf, npad = _guarded(tuple(eps.shape), dtype, gpu, -77.0)
    ops.sde_step(latent, eps, next_in, history, coef, in_scale, step, start, seeds, guidance=guidance, rescale=rescale)
    torch.cuda.synchronize()
    for buf, p in ((lat_buf, pad), (hist_buf, hpad), (nxt_buf, npad)):
        assert _margins_intact(buf, p), "write outside the tensor"
    return latent.clone(), history.clone(), next_in.clone()


def _inputs(gpu, batch, h, w, dtype, seed):
    shape = (batch, 4, h, w)
    gen = torch.Generator().manual_seed(seed)
    lat0 = (torch.randn(shape, generator=gen) * 2.0).to(gpu).contiguous(memory_format=torch.channels_last)
    hist0 = (torch.randn(shape, generator=gen) * 1.5).to(gpu).contiguous(memory_format=torch.channels_last)
    eps2 = torch.randn((2 * batch, 4, h, w), generator=gen)
    eps2[batch:] = eps2[batch:] * 1.5 + 0.25 * eps2[:batch]
    eps2 = eps2.to(gpu, dtype).contiguous(memory_format=torch.channels_last)
    eps1 = eps2[batch:].clone().contiguous(memory_format=torch.channels_last)
    return lat0, hist0, eps1, eps2


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("hw", [(16, 16), (128, 128)])
def test_sde_step_kernel_vs_float64(gpu, sampler, dtype, batch, hw):
    tables = SAMPLERS[sampler](25, karras=True)
    n = tables.n_steps
    i = 11                                                        # read from the device; second order for DPM++ 2M SDE
    c = tables.coefficients()
    row = c[i]
    assert row[4] != 0.0 and (row[3] != 0.0) == (sampler == "dpmpp_2m_sde")
    coef = torch.tensor(c, device=gpu)
    in_scale = torch.tensor(tables.in_scale(), device=gpu)
    guidance = torch.linspace(1.0, 9.0, n, device=gpu)
    step = torch.tensor([i], dtype=torch.int32, device=gpu)
    start = torch.zeros(1, dtype=torch.int32, device=gpu)
    h, w = hw
    seeds = [12345 + 7 * b for b in range(batch)]
    sd = _seeds(seeds, gpu)
    lat0, hist0, eps1, eps2 = _inputs(gpu, batch, h, w, dtype, 11 + batch + h)
    z = _unit(seeds, i + 1, (batch, 4, h, w))
    g, sc = float(guidance[i]), float(in_scale[i + 1])
    for variant in ("plain", "cfg", 0.7):
        guided = variant != "plain"
        phi = variant if isinstance(variant, float) else None
        eps = eps2 if guided else eps1
        rescale = None
        if phi is not None:
            rescale = torch.linspace(0.05, 0.95, n, device=gpu)
            rescale[i] = phi
        args = (gpu, lat0, eps, hist0, dtype, coef, in_scale, step, start, sd, guidance if guided else None, rescale)
        (lat, hist, nxt), (lat2, hist2, nxt2) = _run_kernel(*args), _run_kernel(*args)
        assert torch.equal(lat, lat2) and torch.equal(hist, hist2) and torch.equal(nxt, nxt2), "two calls differ"
        ref, d, xmag, dmag = _restated_update(lat0.cpu(), eps.float().cpu(), hist0.cpu(), row, g if guided else None, phi,
                                              row[3] != 0.0, z)
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
        if guided:
            assert torch.equal(nxt[:batch], nxt[batch:])
        print(f"{sampler} {dtype} B={batch} {hw} {variant}: latent max abs err vs float64 {float(err.max()):.2e}")


@pytest.mark.parametrize("guided", [False, True])
def test_sde_first_order_ignores_history(gpu, guided):
    """NaN history is never read on first-order rows: an img2img start with k != 0, the trajectory start, the last step and
    every Euler ancestral row (k = 0)."""
    shape = (2, 4, 24, 16)
    gen = torch.Generator().manual_seed(5)
    lat0 = torch.randn(shape, generator=gen).to(gpu).contiguous(memory_format=torch.channels_last)
    eps = torch.randn((4 if guided else 2, 4, 24, 16), generator=gen).to(gpu).contiguous(memory_format=torch.channels_last)
    nan_hist = torch.full_like(lat0, float("nan"))
    sd = _seeds([3, 4], gpu)
    for make, cases in ((dpmpp_2m_sde_tables, ((4, 4), (0, 0), (9, 0))), (euler_ancestral_tables, ((4, 0), (0, 0), (9, 0)))):
        tables = make(10, karras=True)
        c = tables.coefficients()
        coef = torch.tensor(c, device=gpu)
        in_scale = torch.tensor(tables.in_scale(), device=gpu)
        guidance = torch.full((10,), 5.0, device=gpu) if guided else None
        for i, start_at in cases:
            step = torch.tensor([i], dtype=torch.int32, device=gpu)
            start = torch.tensor([start_at], dtype=torch.int32, device=gpu)
            lat, hist, nxt = _run_kernel(gpu, lat0, eps, nan_hist, torch.float32, coef, in_scale, step, start, sd, guidance, None)
            assert torch.isfinite(lat).all() and torch.isfinite(hist).all() and torch.isfinite(nxt).all(), (make, i, start_at)
            z = _unit([3, 4], i + 1, shape)
            ref, _, xmag, _ = _restated_update(lat0.cpu(), eps.cpu(), torch.zeros(shape, dtype=torch.float64), c[i],
                                               5.0 if guided else None, None, False, z)
            assert float(((lat.cpu().double() - ref).abs() - 8 * ULP * xmag).max()) <= 0.0
            if i == 9:
                assert c[i].tolist()[1:] == [0.0, 1.0, 0.0, 0.0]
                assert torch.equal(lat, hist)                          # x = d, bit for bit, no noise


def test_sde_injected_noise_is_the_generator(gpu):
    """A row [0, 1, 0, 0, 1] on a zero latent returns exactly philox_normal's values at counter word step + 1."""
    shape = (2, 4, 32, 24)
    lat0 = torch.zeros(shape, device=gpu).contiguous(memory_format=torch.channels_last)
    eps = torch.randn(shape, device=gpu).contiguous(memory_format=torch.channels_last)
    coef = torch.tensor([[0.0, 1.0, 0.0, 0.0, 1.0]] * 8, device=gpu)
    in_scale = torch.ones(8, device=gpu)
    sd = _seeds([(1 << 64) - 3, 99], gpu)
    for i in (0, 5):
        step = torch.tensor([i], dtype=torch.int32, device=gpu)
        lat, _, nxt = _run_kernel(gpu, lat0, eps, lat0, torch.float32, coef, in_scale, step, step, sd, None, None)
        ref = torch.empty_like(lat0)
        ops.philox_normal(ref, sd, i + 1)
        assert torch.equal(lat, ref) and torch.equal(nxt, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("guided", [False, True])
def test_sde_eta0_is_dpmpp2m_bit_for_bit(gpu, dtype, guided):
    sde_t, dpm_t = dpmpp_2m_sde_tables(25, karras=True, eta=0.0), dpmpp_2m_tables(25, karras=True)
    sde_c, dpm_c = torch.tensor(sde_t.coefficients(), device=gpu), torch.tensor(dpm_t.coefficients(), device=gpu)
    in_scale = torch.tensor(dpm_t.in_scale(), device=gpu)
    guidance = torch.full((25,), 6.0, device=gpu) if guided else None
    lat0, hist0, eps1, eps2 = _inputs(gpu, 2, 32, 32, dtype, 3)
    eps = eps2 if guided else eps1
    sd = _seeds([1, 2], gpu)
    start = torch.zeros(1, dtype=torch.int32, device=gpu)
    for i in (0, 11, 24):
        step = torch.tensor([i], dtype=torch.int32, device=gpu)
        got = _run_kernel(gpu, lat0, eps, hist0, dtype, sde_c, in_scale, step, start, sd, guidance, None)
        latent, history = lat0.clone(), hist0.clone()
        next_in = torch.empty_like(eps)
        ops.dpmpp2m_step(latent, eps, next_in, history, dpm_c, in_scale, step, start, guidance=guidance)
        for a, b in zip(got, (latent, history, next_in)):
            assert torch.equal(a, b), i


@pytest.mark.parametrize("guided", [False, True])
def test_sde_batch_rows_are_independent(gpu, guided):
    tables = dpmpp_2m_sde_tables(25, karras=True)
    coef = torch.tensor(tables.coefficients(), device=gpu)
    in_scale = torch.tensor(tables.in_scale(), device=gpu)
    guidance = torch.full((25,), 5.0, device=gpu) if guided else None
    lat0, hist0, eps1, eps2 = _inputs(gpu, 2, 16, 24, torch.float32, 8)
    step = torch.tensor([7], dtype=torch.int32, device=gpu)
    start = torch.zeros(1, dtype=torch.int32, device=gpu)
    eps = eps2 if guided else eps1
    both = _run_kernel(gpu, lat0, eps, hist0, torch.float32, coef, in_scale, step, start, _seeds([17, 1 << 40], gpu), guidance, None)
    eps_one = torch.cat([eps[1:2], eps[3:4]]) if guided else eps[1:2]
    eps_one = eps_one.contiguous(memory_format=torch.channels_last)
    one = _run_kernel(gpu, lat0[1:2].contiguous(memory_format=torch.channels_last), eps_one,
                      hist0[1:2].contiguous(memory_format=torch.channels_last), torch.float32, coef, in_scale, step, start,
                      _seeds([1 << 40], gpu), guidance, None)
    assert torch.equal(both[0][1:2], one[0]) and torch.equal(both[1][1:2], one[1])
    assert torch.equal(both[2][1:2], one[2][0:1])
    same = _run_kernel(gpu, lat0, eps, hist0, torch.float32, coef, in_scale, step, start, _seeds([17, 1 << 40], gpu), guidance, None)
    assert all(torch.equal(a, b) for a, b in zip(both, same))
    other = _run_kernel(gpu, lat0, eps, hist0, torch.float32, coef, in_scale, step, start, _seeds([18, 1 << 40], gpu), guidance, None)
    assert not torch.equal(other[0][0], both[0][0]) and torch.equal(other[0][1], both[0][1])


def test_sde_step_op_rejects_bad_arguments(gpu):
    cl = torch.channels_last
    lat = torch.zeros((1, 4, 16, 16), device=gpu).contiguous(memory_format=cl)
    hist = torch.zeros_like(lat)
    eps = torch.zeros((1, 4, 16, 16), device=gpu, dtype=torch.bfloat16).contiguous(memory_format=cl)
    coef, tbl = torch.ones((10, 5), device=gpu), torch.ones(10, device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    sd = torch.zeros(1, dtype=torch.int64, device=gpu)
    with pytest.raises(ops.BackendError, match=r"\(10, 5\)"):
        ops.sde_step(lat, eps, eps, hist, torch.ones((10, 4), device=gpu), tbl, step, step, sd)
    with pytest.raises(ops.BackendError, match="int64"):
        ops.sde_step(lat, eps, eps, hist, coef, tbl, step, step, sd.int())
    with pytest.raises(ops.BackendError, match="B = 1"):
        ops.sde_step(lat, eps, eps, hist, coef, tbl, step, step, torch.zeros(2, dtype=torch.int64, device=gpu))
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.sde_step(lat, eps, eps, hist, coef, tbl, step, step, sd.cpu())
    with pytest.raises(ops.BackendError, match="2B"):
        ops.sde_step(lat, eps, eps, hist, coef, tbl, step, step, sd, guidance=tbl)
    with pytest.raises(ops.BackendError, match="layout"):
        ops.sde_step(lat, eps, eps, torch.zeros((1, 4, 16, 16), device=gpu), coef, tbl, step, step, sd)
    with pytest.raises(ops.BackendError, match="fp32"):
        ops.philox_normal(torch.zeros((1, 4, 4, 4), device=gpu, dtype=torch.bfloat16), sd, 0)
    with pytest.raises(ops.BackendError, match="B = 1"):
        ops.philox_normal(torch.zeros((1, 4, 4, 4), device=gpu), torch.zeros(3, dtype=torch.int64, device=gpu), 0)
    with pytest.raises(ops.BackendError, match="32-bit"):
        ops.philox_normal(torch.zeros((1, 4, 4, 4), device=gpu), sd, -1)


# ------------------------------------------------------------------------------------------------ TINY network
def _tiny(dtype, dev):
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(dev, dtype)
    synth.fill_module_(m, 0)
    return m, optimize_model(m, cuda_graph=False)


def _tiny_loop(gm, dtype, dev, tables, batch=1, **kw):
    return DenoiseLoop(gm, batch, 16, dtype, dev, tables, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim, **kw)


def _condition(loop, x, dtype, dev, pos, neg=None):
    def rows(k, r):
        return x[k][r].to(dev, dtype)
    keys = ("encoder_hidden_states", "text_embeds", "time_ids")
    if neg is None:
        loop.set_conditioning(*(rows(k, pos) for k in keys))
    else:
        loop.set_conditioning(*(rows(k, pos) for k in keys), *(rows(k, neg) for k in keys))


def _final(loop):
    return loop.latent.contiguous(memory_format=torch.contiguous_format).clone().cpu()


def _sde_coefficients64(tables):
    """float64 [sigma, a, b, k, c] per step from the stored sigmas (the module docstring's formulas)."""
    s = [float(v) for v in tables.sigmas]
    n = len(s) - 1
    eta, s_noise = tables.eta, tables.s_noise
    rows = []
    for i in range(n):
        if s[i + 1] == 0.0:
            rows.append((s[i], 0.0, 1.0, 0.0, 0.0))
            continue
        sc, sn = s[i], s[i + 1]
        if tables.sampler == "euler_ancestral":
            up = min(sn, eta * math.sqrt(sn ** 2 * (sc ** 2 - sn ** 2) / sc ** 2))
            down = math.sqrt(sn ** 2 - up ** 2)
            rows.append((sc, down / sc, 1.0 - down / sc, 0.0, s_noise * up))
            continue
        h = math.log(sc) - math.log(sn)
        k = 0.0 if i == 0 else 1.0 / (2.0 * ((math.log(s[i - 1]) - math.log(sc)) / h))
        rows.append((sc, sn / sc * math.exp(-eta * h), -math.expm1(-(1.0 + eta) * h), k,
                     s_noise * sn * math.sqrt(-math.expm1(-2.0 * eta * h))))
    return rows


def _sde_update64(lat, e, prev, row, first, z):
    sigma, a, b, k, c = row
    d = lat - sigma * e
    if first or k == 0.0:
        x = a * lat + b * d
    else:
        x = a * lat + b * ((1.0 + k) * d - k * prev)
    return x + c * z, d


def _restated_loop(sd, x, tables, seed, g=None, init=None, strength=1.0):
    """float64 loop around the oracle's UNet: noise row 0 of the inputs, the prompt row 1, with g diffusers' CFG against row
    0; step i adds the rng.normal stream of `seed` at counter word i + 1; with `init` the img2img start."""
    n = tables.n_steps
    t_start = max(n - min(int(n * strength), n), 0)
    noise = x["latent"][:1].double()
    lat = noise * tables.init_noise_sigma if init is None else init.double() + noise * float(tables.sigmas[t_start])
    coef, in_scale = _sde_coefficients64(tables), tables.in_scale()
    rows = slice(1, 2)
    ehs, te, ti = (x[k][rows] for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    if g is not None:
        ehs, te, ti = (torch.cat([x[k][0:1], x[k][rows]]) for k in ("encoder_hidden_states", "text_embeds", "time_ids"))
    prev = None
    for i in range(t_start, n):
        t = torch.tensor(float(tables.timesteps[i]))
        if g is None:
            e = orc.unet_forward(sd, lat.float() * float(in_scale[i]), t, ehs, te, ti).double()
        else:
            e2 = orc.unet_forward(sd, torch.cat([lat, lat]).float() * float(in_scale[i]), t, ehs, te, ti).double()
            e = e2[:1] + g * (e2[1:] - e2[:1])
        lat, prev = _sde_update64(lat, e, prev, coef[i], i == t_start, _unit([seed], i + 1, tuple(lat.shape)))
    return lat


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("cfg", [False, True])
def test_tiny_sde_loop_modes(gpu, sampler, dtype, karras, cfg):
    m, gm = _tiny(dtype, gpu)
    tables = SAMPLERS[sampler](10, karras=karras)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    kw = dict(guidance_scale=5.0) if cfg else {}
    seed = 20261016
    finals = {}
    for mode in ("eager", "step", "loop"):
        loop = _tiny_loop(gm, dtype, gpu, tables, mode=mode, **kw)
        _condition(loop, x, dtype, gpu, slice(1, 2), slice(0, 1) if cfg else None)
        with torch.no_grad():
            finals[mode] = loop.denoise(x["latent"][:1], seed=seed).cpu()
            again = loop.denoise(x["latent"][:1]).cpu()                 # a replay repeats bit for bit (the seed stays)
            other = loop.denoise(x["latent"][:1], seed=seed + 1).cpu()  # a new seed, no new capture: other noise
            back = loop.denoise(x["latent"][:1], seed=seed).cpu()
        assert torch.equal(finals[mode], again) and torch.equal(finals[mode], back), mode
        assert not torch.equal(finals[mode], other), mode
    assert torch.equal(finals["eager"], finals["step"]) and torch.equal(finals["eager"], finals["loop"])
    assert torch.isfinite(finals["loop"]).all()
    if dtype == torch.float32:
        sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
        ref = _restated_loop(sd, x, tables, seed, 5.0 if cfg else None)
        err = float((finals["loop"].double() - ref).abs().max())
        print(f"tiny {sampler} 10-step loop fp32 karras={karras} cfg={cfg}: max abs err vs float64 restatement {err:.2e} "
              f"(|ref| max {float(ref.abs().max()):.2f})")
        assert err <= ABS_TOL_STRICT


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("mode", ["step", "eager"])
@pytest.mark.parametrize("cfg", [False, True])
def test_tiny_sde_img2img_vs_float64(gpu, sampler, mode, cfg):
    m, gm = _tiny(torch.float32, gpu)
    tables = SAMPLERS[sampler](10, karras=True)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    init = synth.normal("img2img.init", (1, 4, 16, 16), 77) * 0.8
    loop = _tiny_loop(gm, torch.float32, gpu, tables, mode=mode, **(dict(guidance_scale=5.0) if cfg else {}))
    _condition(loop, x, torch.float32, gpu, slice(1, 2), slice(0, 1) if cfg else None)
    with torch.no_grad():
        loop.denoise(x["latent"][1:2] * 2.0, seed=5)                   # a trajectory before: its history must not leak in
        left = loop.set_image(init, x["latent"][:1], 0.5, seed=99)
        assert left == 5 and int(loop.start) == 5
        loop.run_steps(left)
    out = _final(loop)
    sd = {k: v.float().cpu() for k, v in m.state_dict().items()}
    ref = _restated_loop(sd, x, tables, 99, 5.0 if cfg else None, init=init, strength=0.5)
    err = float((out.double() - ref).abs().max())
    print(f"tiny {sampler} img2img (strength 0.5, mode {mode}, cfg={cfg}) fp32: max abs err vs float64 restatement {err:.2e}")
    assert err <= ABS_TOL_STRICT


def test_tiny_seeded_start_is_the_generator(gpu):
    """denoise(seed=s) is denoise(philox_normal(s, counter 0)) bit for bit, for Euler (whose graph never reads the seeds)
    and for a stochastic sampler."""
    _, gm = _tiny(torch.bfloat16, gpu)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    for tables in (euler_discrete_tables(10), euler_ancestral_tables(10)):
        loop = _tiny_loop(gm, torch.bfloat16, gpu, tables, mode="loop")
        _condition(loop, x, torch.bfloat16, gpu, slice(1, 2))
        with torch.no_grad():
            seeded = loop.denoise(seed=424242).cpu()
            z = torch.empty_like(loop.latent)
            ops.philox_normal(z, _seeds([424242], gpu), 0)
            from_tensor = loop.denoise(z.clone()).cpu()
        assert torch.equal(seeded, from_tensor)
        zref = _unit([424242], 0, (1, 4, 16, 16))
        assert float(((z.cpu().double() - zref).abs() / zref.abs().clamp(min=1.0)).max()) <= Z_TOL


def test_tiny_sde_batch_rows_match_single(gpu):
    """B = 2 with seeds [s0, s1]: each row is its own B = 1 run with its seed, bit for bit."""
    _, gm = _tiny(torch.float32, gpu)
    tables = dpmpp_2m_sde_tables(10, karras=True)
    x = synth.denoise_inputs(2, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    loop = _tiny_loop(gm, torch.float32, gpu, tables, batch=2, mode="loop")
    _condition(loop, x, torch.float32, gpu, slice(0, 2))
    with torch.no_grad():
        both = loop.denoise(x["latent"][:2], seed=[31, 32]).cpu()
    for k in range(2):
        one = _tiny_loop(gm, torch.float32, gpu, tables, mode="loop")
        _condition(one, x, torch.float32, gpu, slice(k, k + 1))
        with torch.no_grad():
            single = one.denoise(x["latent"][k:k + 1], seed=31 + k).cpu()
        err = float((both[k:k + 1] - single).abs().max())
        print(f"tiny DPM++ 2M SDE B=2 row {k} vs its B=1 run: max abs diff {err:.2e}")
        assert err <= ABS_TOL_STRICT
    assert not torch.equal(both[0], both[1])


# ------------------------------------------------------------------------------------------------ SDXL-base, synthetic weights
def test_sdxl_dpmpp_2m_sde_karras_cfg_fp32_strict(gpu, sdxl_fp32):
    """The captured 25-step loop against a float64 restatement of the update driven step by step (mode eager) by the same
    compiled UNet's eps and the generator's noise."""
    x = synth.denoise_inputs(2, 64, 1234)
    tables = dpmpp_2m_sde_tables(25, karras=True)
    seed = 77

    def make(mode):
        lp = DenoiseLoop(sdxl_fp32, 1, 64, torch.float32, gpu, tables, guidance_scale=5.0, mode=mode)
        _condition(lp, x, torch.float32, gpu, slice(1, 2), slice(0, 1))
        return lp

    loop, ev = make("loop"), make("eager")
    coef, in_scale = _sde_coefficients64(tables), tables.in_scale()
    with torch.no_grad():
        out = loop.denoise(x["latent"][:1], seed=seed).cpu().double()
        lat = x["latent"][:1].double() * tables.init_noise_sigma
        prev = None
        for i in range(tables.n_steps):
            ev.x_in.copy_(torch.cat([lat, lat]).float().mul_(float(in_scale[i])).to(gpu))
            row = tuple(tbl[i] for tbl in ev.time_tables) if ev._tsplit else None
            e2 = ev._unet(ev.timesteps[i], row).double().cpu()
            e = e2[:1] + 5.0 * (e2[1:] - e2[:1])
            lat, prev = _sde_update64(lat, e, prev, coef[i], i == 0, _unit([seed], i + 1, (1, 4, 64, 64)))
    err = float((out - lat).abs().max())
    print(f"SDXL DPM++ 2M SDE Karras 25 steps CFG 5 fp32 (mode loop): max abs err {err:.2e} vs the float64 restatement of "
          f"the update (|ref| max {float(lat.abs().max()):.2f})")
    assert torch.isfinite(out).all()
    assert err <= ABS_TOL_STRICT
