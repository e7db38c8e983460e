"""Perturbed-attention guidance, the kernels: st_attention_pag (attention with an identity tail, csrc/pag.hip) against
ops.attention on the sub-batch and the v rows, bit for bit, with its strict-mode split image; the three-way update kernels
(st_pag_euler_step, st_pag_dpmpp2m_step, st_pag_sde_step) against the tests' float64 restatement (tests/pag_util.py) and, with
the pag table at 0, against the existing two-way kernels bit for bit."""
import math

import pytest
import torch

from stabletriton_amd import _C, ops, synth
from stabletriton_amd.optimization import optimize_model
from stabletriton_amd.scheduler import dpmpp_2m_sde_tables, dpmpp_2m_tables, euler_discrete_tables
from stabletriton_amd.unet import TINY, UNet2DConditionModel
from tests import pag_util as PU

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -24
Z_TOL = 4e-6                    # tests/test_sde_loop_gpu.py: the generator's own error relative to max(1, |z|)
ROUND = {torch.float32: (2.0 ** -23, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24)}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _margins_intact(buf, pad):
    return bool(torch.all(buf[:pad] == buf[0]) and torch.all(buf[-pad:] == buf[0]))


# ------------------------------------------------------------------------------------------------ attention with an identity tail
# (B, T, H, D): T = 96 is no multiple of the 64- and 128-row tiles; (2, 256, 4, 64) whole tiles, more than one block; SDXL's mid
# block at latent 128; head size 32 takes the generic kernel
ATT_SHAPES = [(3, 96, 2, 64), (2, 256, 4, 64), (3, 1024, 20, 64), (3, 64, 4, 32)]


def _qkv(gpu, dtype, B, T, H, D, fused):
    C = H * D
    if fused:
        buf = synth.normal(f"pag.qkv.{B}.{T}.{C}", (B, T, 3 * C), 3).to(gpu, dtype)
        return buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    return tuple(synth.normal(f"pag.{n}.{B}.{T}.{C}", (B, T, C), 3).to(gpu, dtype) for n in "qkv")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("shape", ATT_SHAPES)
def test_attention_pag_bits(gpu, dtype, fused, shape):
    B, T, H, D = shape
    C = H * D
    q, k, v = _qkv(gpu, dtype, B, T, H, D, fused)
    scale = D ** -0.5
    lib = _C.load()
    ld = q.stride(1)
    for ident in (0, 1, B):
        lead = B - ident
        got = ops.attention_pag(q, k, v, H, scale, ident)
        again = ops.attention_pag(q, k, v, H, scale, ident)
        assert torch.equal(got, again), "two calls differ"
        if lead:
            want = ops.attention(q[:lead], k[:lead], v[:lead], H, scale)
            assert torch.equal(got[:lead], want), f"ident {ident}: unperturbed entries differ from ops.attention on the sub-batch"
        if ident:
            assert torch.equal(got[lead:], v[lead:]), f"ident {ident}: perturbed entries are not v"
        # the entry point itself, into a guarded output: nothing outside `out`
        pad = 256
        buf = torch.full((B * T * C + 2 * pad,), -77.0, dtype=dtype, device=gpu)
        out = buf[pad:pad + B * T * C].view(B, T, C)
        _C.check(lib.st_attention_pag(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, T, T, H, D, ld, ld, ld, C,
                                      float(scale), _C.dtype_code(dtype), ident, _C.stream_ptr()), "attention_pag")
        torch.cuda.synchronize()
        assert _margins_intact(buf, pad), "write outside the tensor"
        assert torch.equal(out, got)


def test_attention_pag_rejections(gpu):
    lib = _C.load()
    q = torch.zeros((2, 64, 128), device=gpu, dtype=torch.bfloat16)
    kv = torch.zeros((2, 77, 128), device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ops.BackendError, match="T == S"):
        ops.attention_pag(q, kv, kv, 2, 0.125, 1)
    out = torch.empty_like(q)
    args = lambda **kw: [kw.get("q", q.data_ptr()), kv.data_ptr(), kw.get("v", kv.data_ptr()), out.data_ptr(), 2, 64, kw.get("S", 77), 2, 64,
                         128, 128, kw.get("ldv", 128), 128, 0.125, _C.ST_BF16, kw.get("ident", 1), None]
    assert lib.st_attention_pag(*args()) != 0 and b"T == S" in lib.st_last_error()
    assert lib.st_attention_pag(*args(S=64, ident=3)) != 0 and b"ident_count" in lib.st_last_error()
    assert lib.st_attention_pag(*args(S=64, ident=-1)) != 0 and b"ident_count" in lib.st_last_error()
    assert lib.st_attention_pag(*args(S=64, ldv=132)) != 0 and b"16-byte" in lib.st_last_error()
    assert lib.st_attention_pag(*args(S=64, v=q.data_ptr() + 2)) != 0 and b"16-byte" in lib.st_last_error()
    # T != S without a tail is ordinary cross-attention
    got = ops.attention_pag(q, kv, kv, 2, 0.125, 0)
    assert torch.equal(got, ops.attention(q, kv, kv, 2, 0.125))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ident", [1, 3])
def test_attention_pag_split_image_is_complete(gpu, fused, ident):
    """Strict mode: the image the two launches leave for the output projection equals st_split_f32 of the output, every row."""
    B, T, H, D = 3, 96, 2, 64
    q, k, v = _qkv(gpu, torch.float32, B, T, H, D, fused)
    out = ops.attention_pag(q, k, v, H, D ** -0.5, ident)
    note = ops._split_notes(out.device)[-1]
    assert note[0] is out and note[2:4] == (B * T, H * D), "the producer's image must have been noted"
    noted = note[4]
    fresh = ops.split_rows(out.view(B * T, H * D)).s
    assert torch.equal(noted.view(torch.int32), fresh.view(torch.int32))


def test_strict_step_with_and_without_emitted_images(gpu):
    """An fp32 compiled TINY step with PAG: producers' split images on (the identity tail completes attention's) against
    every consumer splitting for itself - the same bits."""
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(gpu, torch.float32)
    synth.fill_module_(m, 0)
    gm = optimize_model(m, cuda_graph=False, pag_layers=("mid",))
    assert gm.rewrite_stats["pag_sites"] == 2
    x = synth.denoise_inputs(3, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    args = (x["latent"].to(gpu), torch.tensor(500.0, device=gpu), x["encoder_hidden_states"].to(gpu),
            {"text_embeds": x["text_embeds"].to(gpu), "time_ids": x["time_ids"].to(gpu)})
    outs = {}
    keep = ops.EMIT_SPLIT
    try:
        for emit in (True, False):
            ops.EMIT_SPLIT = emit
            with torch.no_grad(), gm.pag.using(3):
                outs[emit] = gm(*args)[0].clone()
        with torch.no_grad():
            plain = gm(*args)[0].clone()
    finally:
        ops.EMIT_SPLIT = keep
    assert torch.equal(outs[True], outs[False])
    # the unperturbed rows are the plain module's (the attention launch sees a sub-batch: the project's strict gate, not bits)
    assert float((outs[True][:2] - plain[:2]).abs().max()) <= 1e-3 and float((outs[True][2] - plain[2]).abs().max()) > 1e-2


# ------------------------------------------------------------------------------------------------ the update kernels
def _guarded(shape, dtype, dev, fill):
    n = math.prod(shape)
    pad = 64
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    b, c, h, w = shape
    t = buf[pad:pad + n].view(b, h, w, c).permute(0, 3, 1, 2)
    assert t.is_contiguous(memory_format=torch.channels_last)
    return t, buf, pad


def _seeds(vals, dev):
    return torch.tensor(vals, dtype=torch.int64, device=dev)


class _Case:
    """One sampler row: tables on the device, the step, and how to launch the three-way and the two-way kernel."""

    def __init__(self, kind, gpu):
        self.kind = kind
        if kind == "euler":
            t = euler_discrete_tables(50)
            self.i, self.start_at = 37, 0
            self.dsigma = torch.tensor(t.dsigma(), device=gpu)
            self.row = (float(t.dsigma()[self.i]),)
        elif kind in ("dpm_first", "dpm_second"):
            t = dpmpp_2m_tables(25, karras=True)
            self.i = 11
            self.start_at = 11 if kind == "dpm_first" else 0          # i == start: first order, the history is not read
            self.coef = torch.tensor(t.coefficients(), device=gpu)
            self.row = tuple(float(v) for v in t.coefficients()[self.i])
            assert self.row[3] != 0.0
        else:
            t = dpmpp_2m_sde_tables(25, karras=True)
            self.i, self.start_at = 11, 0
            self.coef = torch.tensor(t.coefficients(), device=gpu)
            self.row = tuple(float(v) for v in t.coefficients()[self.i])
            assert self.row[3] != 0.0 and self.row[4] != 0.0
        self.n = t.n_steps
        self.in_scale = torch.tensor(t.in_scale(), device=gpu)
        self.sc = float(self.in_scale[self.i + 1])
        self.step = torch.tensor([self.i], dtype=torch.int32, device=gpu)
        self.start = torch.tensor([self.start_at], dtype=torch.int32, device=gpu)
        self.second = kind in ("dpm_second", "sde")

    def launch(self, latent, eps, next_in, history, seeds, guidance, rescale, pag):
        k = self.kind
        if k == "euler":
            if pag is not None:
                ops.pag_euler_step(latent, eps, next_in, self.dsigma, self.in_scale, guidance, pag, self.step, rescale=rescale)
            else:
                ops.cfg_euler_step(latent, eps, next_in, self.dsigma, self.in_scale, guidance, self.step, rescale=rescale)
        elif k == "sde":
            if pag is not None:
                ops.pag_sde_step(latent, eps, next_in, history, self.coef, self.in_scale, self.step, self.start, seeds, pag,
                                 guidance=guidance, rescale=rescale)
            else:
                ops.sde_step(latent, eps, next_in, history, self.coef, self.in_scale, self.step, self.start, seeds, guidance=guidance,
                             rescale=rescale)
        elif pag is not None:
            ops.pag_dpmpp2m_step(latent, eps, next_in, history, self.coef, self.in_scale, self.step, self.start, pag, guidance=guidance,
                                 rescale=rescale)
        else:
            ops.dpmpp2m_step(latent, eps, next_in, history, self.coef, self.in_scale, self.step, self.start, guidance=guidance,
                             rescale=rescale)

    def run(self, gpu, lat0, eps, hist0, dtype, seeds, guidance, rescale, pag):
        shape = tuple(lat0.shape)
        latent, lat_buf, pad = _guarded(shape, torch.float32, gpu, 1234.5)
        latent.copy_(lat0)
        history, hist_buf, hpad = _guarded(shape, torch.float32, gpu, -4321.0)
        history.copy_(hist0)
        next_in, nxt_buf, npad = _guarded(tuple(eps.shape), dtype, gpu, -77.0)
        self.launch(latent, eps, next_in, history, seeds, guidance, rescale, pag)
        torch.cuda.synchronize()
        for buf, p in ((lat_buf, pad), (hist_buf, hpad), (nxt_buf, npad)):
            assert _margins_intact(buf, p), "write outside the tensor"
        return latent.clone(), history.clone(), next_in.clone()

    def restated(self, lat0, e, emag, hist0, z):
        """float64 update from the guided e with the kernel's fp32 row; (x, d or None, |x| terms, |d| terms or None)."""
        x0 = lat0.double()
        if self.kind == "euler":
            ds = self.row[0]
            return x0 + e * ds, None, emag * abs(ds) + x0.abs(), None
        sigma, a, bb, k = self.row[:4]
        d = x0 - sigma * e
        dmag = x0.abs() + sigma * emag
        if self.second:
            x = a * x0 + bb * ((1.0 + k) * d - k * hist0.double())
            xmag = a * x0.abs() + bb * ((1.0 + k) * dmag + k * hist0.double().abs())
        else:
            x = a * x0 + bb * d
            xmag = a * x0.abs() + bb * dmag
        if self.kind == "sde":
            c = self.row[4]
            x = x + c * z
            xmag = xmag + abs(c) * z.abs() + abs(c) * Z_TOL / ULP * z.abs().clamp(min=1.0)
        return x, d, xmag, dmag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("hw", [(16, 16), (152, 104)])
@pytest.mark.parametrize("variant", ["cfg", "cfg_rescale", "alone"])
@pytest.mark.parametrize("kind", ["euler", "dpm_first", "dpm_second", "sde"])
def test_pag_step_kernels_vs_float64(gpu, kind, variant, hw, batch, dtype):
    case = _Case(kind, gpu)
    n, i = case.n, case.i
    cfg = variant != "alone"
    phi = 0.7 if variant == "cfg_rescale" else None
    blocks = 3 if cfg else 2
    h, w = hw
    shape = (batch, 4, h, w)
    gen = torch.Generator().manual_seed(23 + batch + h)
    cl = torch.channels_last
    lat0 = (torch.randn(shape, generator=gen) * 2.0).to(gpu).contiguous(memory_format=cl)
    hist0 = (torch.randn(shape, generator=gen) * 1.5).to(gpu).contiguous(memory_format=cl)
    if kind == "dpm_first":
        hist0 = torch.full_like(hist0, float("nan"))                # first order: never read
    e3 = torch.randn((3 * batch, 4, h, w), generator=gen)
    e3[batch:2 * batch] = e3[batch:2 * batch] * 1.5 + 0.25 * e3[:batch]              # positive: another scale than the negative
    e3[2 * batch:] = e3[2 * batch:] * 0.6 + 0.5 * e3[batch:2 * batch]                # perturbed: another scale than the positive
    eps = (e3 if cfg else e3[batch:]).to(gpu, dtype).contiguous(memory_format=cl)
    guidance = torch.linspace(1.0, 9.0, n, device=gpu) if cfg else None
    pag = torch.linspace(0.5, 4.5, n, device=gpu)
    rescale = None
    if phi is not None:
        rescale = torch.linspace(0.05, 0.95, n, device=gpu)
        rescale[i] = phi
    g = float(guidance[i]) if cfg else None
    s = float(pag[i])
    seed_vals = [12345 + 7 * b for b in range(batch)]
    seeds = _seeds(seed_vals, gpu)
    z = None
    if kind == "sde":
        from stabletriton_amd import rng
        z = torch.from_numpy(rng.normal(seed_vals, i + 1, 4 * h * w)).view(batch, h, w, 4).permute(0, 3, 1, 2)
    args = (gpu, lat0, eps, hist0, dtype, seeds, guidance, rescale)
    (lat, hist, nxt), (lat2, hist2, nxt2) = case.run(*args, pag), case.run(*args, pag)
    assert torch.equal(lat, lat2) and torch.equal(nxt, nxt2), "two calls differ"
    if kind != "euler":
        assert torch.equal(hist, hist2), "two calls differ"
    ef = eps.float().cpu()
    parts = list(ef.split(batch))
    e_neg = parts.pop(0) if cfg else None
    e_pos, e_pert = parts
    e = PU.guide64(e_neg, e_pos, e_pert, g, s, phi)
    emag = PU.guide_magnitude(e_neg, e_pos, e_pert, g, s, phi)
    ref, d, xmag, dmag = case.restated(lat0.cpu(), e, emag, hist0.cpu(), z)
    err = (lat.cpu().double() - ref).abs()
    print(f"{kind} {variant} {dtype} B={batch} {hw}: latent max abs err vs float64 {float(err.max()):.2e}")
    assert float((err - 8 * ULP * xmag).max()) <= 0.0, f"latent max abs err {float(err.max()):.3e}"
    if d is not None:
        e_d = (hist.cpu().double() - d).abs()
        assert float((e_d - 8 * ULP * dmag).max()) <= 0.0, f"history max abs err {float(e_d.max()):.3e}"
    want = ref * case.sc
    rel, absolute = ROUND[dtype]
    for r in range(blocks):
        blk = nxt[r * batch:(r + 1) * batch]
        assert torch.equal(blk, nxt[:batch]), "row blocks of next_in differ"
    e_nxt = (nxt[:batch].cpu().double() - want).abs()
    assert float((e_nxt - rel * want.abs() - absolute - 8 * ULP * xmag * case.sc).max()) <= 0.0
    # the pag table at 0: the existing kernel on the rows without the perturbed block, bit for bit
    zero = torch.zeros(n, device=gpu)
    lat_z, hist_z, nxt_z = case.run(*args, zero)
    if cfg or kind != "euler":                     # (Euler without guidance is euler_step, another kernel: nothing to compare bits with)
        two = eps[:(blocks - 1) * batch].contiguous(memory_format=cl)
        lat_t, hist_t, nxt_t = case.run(gpu, lat0, two, hist0, dtype, seeds, guidance, rescale, None)
        assert torch.equal(lat_z, lat_t), "pag = 0 differs from the two-way kernel"
        if kind != "euler":
            assert torch.equal(hist_z, hist_t)
        assert torch.equal(nxt_z[:batch], nxt_t[:batch])
    assert not torch.equal(lat_z, lat)


def test_pag_step_ops_reject_bad_arguments(gpu):
    cl = torch.channels_last
    lat = torch.zeros((1, 4, 16, 16), device=gpu).contiguous(memory_format=cl)
    hist = torch.zeros_like(lat)
    mk = lambda rows: torch.zeros((rows, 4, 16, 16), device=gpu, dtype=torch.bfloat16).contiguous(memory_format=cl)
    e1, e2, e3 = mk(1), mk(2), mk(3)
    tbl, coef4, coef5 = torch.ones(10, device=gpu), torch.ones((10, 4), device=gpu), torch.ones((10, 5), device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    seeds = torch.zeros(1, dtype=torch.int64, device=gpu)
    short = torch.ones(9, device=gpu)
    with pytest.raises(ops.BackendError, match="3B"):
        ops.pag_euler_step(lat, e2, e2, tbl, tbl, tbl, tbl, step)                    # guided: 3B rows
    with pytest.raises(ops.BackendError, match="2B"):
        ops.pag_euler_step(lat, e3, e3, tbl, tbl, None, tbl, step)                   # unguided: 2B rows
    with pytest.raises(ops.BackendError, match="2B"):
        ops.pag_dpmpp2m_step(lat, e1, e1, hist, coef4, tbl, step, step, tbl)
    with pytest.raises(ops.BackendError, match="3B"):
        ops.pag_sde_step(lat, e2, e2, hist, coef5, tbl, step, step, seeds, tbl, guidance=tbl)
    with pytest.raises(ops.BackendError, match="n_steps"):
        ops.pag_euler_step(lat, e3, e3, tbl, tbl, tbl, short, step)
    with pytest.raises(ops.BackendError, match="n_steps"):
        ops.pag_dpmpp2m_step(lat, e2, e2, hist, coef4, tbl, step, step, short)
    with pytest.raises(ops.BackendError, match=r"\(10, 5\)"):
        ops.pag_sde_step(lat, e2, e2, hist, coef4, tbl, step, step, seeds, tbl)
    with pytest.raises(ops.BackendError, match="rescale needs guidance"):
        ops.pag_euler_step(lat, e2, e2, tbl, tbl, None, tbl, step, rescale=tbl)
    with pytest.raises(ops.BackendError, match="layout"):
        nchw = torch.zeros((2, 4, 16, 16), device=gpu, dtype=torch.bfloat16)
        ops.pag_euler_step(lat, nchw, nchw, tbl, tbl, None, tbl, step)
    with pytest.raises(ops.BackendError, match="int32"):
        ops.pag_dpmpp2m_step(lat, e2, e2, hist, coef4, tbl, step, step.long(), tbl)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.pag_euler_step(lat.cpu(), e2, e2, tbl, tbl, None, tbl, step)
    lib = _C.load()
    rc = lib.st_pag_euler_step(lat.data_ptr(), e2.data_ptr(), e2.data_ptr(), tbl.data_ptr(), tbl.data_ptr(), None, None, None, step.data_ptr(),
                               1, 1024, 10, _C.ST_BF16, None, 0, None)
    assert rc != 0 and b"null" in lib.st_last_error()
