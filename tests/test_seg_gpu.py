"""Smoothed energy guidance, the kernels: st_seg_blur (the query blur, csrc/seg.hip) against the tests' float64 statement
(tests/seg_util.py) within a bound that follows from the arithmetic, with guarded outputs, repeatability and the in-place switch of
its device parameter row; st_attention_seg (attention with a blurred-query tail) against ops.attention on the sub-batch and
ops.attention(ops.seg_blur(q_tail), ...) bit for bit, its rejections and its strict-mode split image."""
import functools

import pytest
import torch

from stabletriton_amd import _C, ops, seg, synth
from tests import seg_util as SU

pytestmark = pytest.mark.gpu
INF = float("inf")
ROUND = {torch.float32: (2.0 ** -23, 0.0), torch.bfloat16: (2.0 ** -8, 0.0), torch.float16: (2.0 ** -10, 2.0 ** -24)}      # test_pag_gpu.py
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
SIGMAS = [0.5, 1.0, 3.0, 10.0, INF]

# (n, h, w, C): the clamp makes k exceed the side; a rectangle with reflect on the short axis; odd sides; SDXL's mid block at latent
# 128; more than one LDS plane pair for 16-bit elements: the general form; C no multiple of 64
BLUR_SHAPES = [(1, 4, 4, 128), (2, 6, 4, 128), (1, 5, 7, 64), (1, 32, 32, 1280), (1, 64, 64, 640), (1, 12, 20, 136)]


def _margins_intact(buf, pad):
    return bool(torch.all(buf[:pad] == buf[0]) and torch.all(buf[-pad:] == buf[0]))


def _row(gpu, sigma, h, w):
    return torch.tensor(seg.param_row(sigma, h, w), dtype=torch.float32, device=gpu)


@functools.lru_cache(maxsize=None)
def _queries(shape, dtype):
    """CPU values of one shape in one dtype (what the kernel reads), shared by its cases."""
    n, h, w, C = shape
    return synth.normal(f"seg.q.{n}.{h}.{w}.{C}", (n, h * w, 3 * C), 3).to(dtype)


@functools.lru_cache(maxsize=16)             # (one shape's three dtypes x five sigmas: the fused and the dense case share them)
def _blur_reference(shape, dtype, sigma):
    """(float64 blur, elementwise bound) of the q columns of _queries, computed once per case."""
    n, h, w, C = shape
    q = _queries(shape, dtype)[..., :C]
    return SU.blur64(q, (h, w), sigma), SU.blur_bound(q, (h, w), sigma, ROUND[dtype])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "dense"])
@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=str)
def test_seg_blur_vs_float64(gpu, shape, fused, dtype):
    n, h, w, C = shape
    T = h * w
    buf = _queries(shape, dtype).to(gpu)
    q = buf[..., :C] if fused else buf[..., :C].contiguous()
    assert q.stride(1) == (3 * C if fused else C)
    lib = _C.load()
    row = _row(gpu, 1.0, h, w)
    address = row.data_ptr()
    results = {}
    for sigma in SIGMAS:
        row.copy_(torch.tensor(seg.param_row(sigma, h, w), dtype=torch.float32))       # the same device row, rewritten in place
        assert row.data_ptr() == address
        got = ops.seg_blur(q, (h, w), row)
        assert got.shape == (n, T, C) and got.is_contiguous() and got.dtype == dtype
        assert torch.equal(got, ops.seg_blur(q, (h, w), row)), f"sigma {sigma}: two calls differ"
        want, bound = _blur_reference(shape, dtype, sigma)
        err = (got.double().cpu() - want).abs()
        print(f"{shape} {dtype} {'fused' if fused else 'dense'} sigma {sigma}: max abs err vs float64 {float(err.max()):.3e}, "
              f"largest err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert float((err - bound).max()) <= 0.0, f"sigma {sigma}: max abs err {float(err.max()):.3e}"
        if sigma == INF:
            assert torch.equal(got, got[:, :1].expand_as(got)), "every token of a plane is the plane's mean, the same bits"
        results[sigma] = got
        # the entry point itself, into a guarded output: nothing outside the n * T rows
        pad = 512
        guard = torch.full((n * T * C + 2 * pad,), -77.0, dtype=dtype, device=gpu)
        out = guard[pad:pad + n * T * C].view(n, T, C)
        nbytes = lib.st_seg_blur_workspace_bytes(n, h, w, C, _C.dtype_code(dtype))
        ws = torch.full((nbytes // 4 + 2 * pad,), -77.0, dtype=torch.float32, device=gpu)
        _C.check(lib.st_seg_blur(q.data_ptr(), out.data_ptr(), row.data_ptr(), n, h, w, C, q.stride(1), C, _C.dtype_code(dtype),
                                 ws[pad:].data_ptr() if nbytes else None, nbytes, _C.stream_ptr()), "seg_blur")
        torch.cuda.synchronize()
        assert _margins_intact(guard, pad) and _margins_intact(ws, pad), "write outside the tensor"
        assert torch.equal(out, got)
    # the same row switched between two finite sigmas and infinity changes what the same launch computes
    assert not torch.equal(results[1.0], results[3.0]) and not torch.equal(results[1.0], results[INF])
    assert torch.equal(buf, _queries(shape, dtype).to(gpu)), "the input is not written"


def test_seg_blur_reads_its_row_when_it_runs_and_clamps_it(gpu):
    """A row holding a tap count beyond the grid's limit (or an even one) cannot make the kernel index outside the plane: it is
    clamped on the device to the rule's range."""
    h, w, C = 6, 4, 64
    q = synth.normal("seg.clamp", (1, h * w, C), 3).to(gpu, torch.float32)
    good = _row(gpu, 10.0, h, w)
    assert int(good[1]) == 5
    bad = good.clone()
    bad[1] = 99.0
    assert torch.equal(ops.seg_blur(q, (h, w), bad), ops.seg_blur(q, (h, w), good))
    bad[1] = 6.0
    assert torch.equal(ops.seg_blur(q, (h, w), bad), ops.seg_blur(q, (h, w), good))
    with pytest.raises(ops.BackendError, match="params_row"):
        ops.seg_blur(q, (h, w), good[:8])
    with pytest.raises(ops.BackendError, match="token grid"):
        ops.seg_blur(q, (h, w + 1), good)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.seg_blur(q.cpu(), (h, w), good)


# ------------------------------------------------------------------------------------------------ attention with a blurred tail
# (B, h, w, H, D): T = 96 is no multiple of the 64- and 128-row tiles; whole tiles, more than one block; SDXL's mid block at latent
# 128; head size 32 takes the generic kernel
ATT_SHAPES = [(3, 8, 12, 2, 64), (2, 16, 16, 4, 64), (3, 32, 32, 20, 64), (3, 8, 8, 4, 32)]


def _qkv(gpu, dtype, B, T, H, D, fused):
    C = H * D
    if fused:
        buf = synth.normal(f"seg.qkv.{B}.{T}.{C}", (B, T, 3 * C), 3).to(gpu, dtype)
        return buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    return tuple(synth.normal(f"seg.{n}.{B}.{T}.{C}", (B, T, C), 3).to(gpu, dtype) for n in "qkv")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "dense"])
@pytest.mark.parametrize("shape", ATT_SHAPES, ids=str)
def test_attention_seg_bits(gpu, dtype, fused, shape):
    B, h, w, H, D = shape
    T, C = h * w, H * D
    q, k, v = _qkv(gpu, dtype, B, T, H, D, fused)
    scale = D ** -0.5
    lib = _C.load()
    ld = q.stride(1)
    for sigma in (1.0, INF):
        row = _row(gpu, sigma, h, w)
        for tail in (0, 1, B):
            lead = B - tail
            got = ops.attention_seg(q, k, v, H, scale, tail, (h, w), row)
            assert torch.equal(got, ops.attention_seg(q, k, v, H, scale, tail, (h, w), row)), "two calls differ"
            if lead:
                want = ops.attention(q[:lead], k[:lead], v[:lead], H, scale)
                assert torch.equal(got[:lead], want), f"tail {tail}: unperturbed entries differ from ops.attention on the sub-batch"
            if tail:
                blurred = ops.seg_blur(q[lead:], (h, w), row)
                assert torch.equal(got[lead:], ops.attention(blurred, k[lead:], v[lead:], H, scale)), f"tail {tail}: the composition differs"
                assert not torch.equal(got[lead:], ops.attention(q[lead:], k[lead:], v[lead:], H, scale)), "the tail must differ from plain attention"
            # the entry point itself, into guarded output and scratch: nothing outside them
            pad = 256
            buf = torch.full((B * T * C + 2 * pad,), -77.0, dtype=dtype, device=gpu)
            out = buf[pad:pad + B * T * C].view(B, T, C)
            sbuf = torch.full((max(tail, 1) * T * C + 2 * pad,), -77.0, dtype=dtype, device=gpu)
            nbytes = lib.st_seg_blur_workspace_bytes(max(tail, 1), h, w, C, _C.dtype_code(dtype))
            ws = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=gpu)
            _C.check(lib.st_attention_seg(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), sbuf[pad:].data_ptr(), B, T, T, H, D, ld, ld,
                                          ld, C, float(scale), _C.dtype_code(dtype), tail, h, w, row.data_ptr(), ws.data_ptr(), nbytes,
                                          _C.stream_ptr()), "attention_seg")
            torch.cuda.synchronize()
            assert _margins_intact(buf, pad) and _margins_intact(sbuf, pad), "write outside the tensor"
            assert torch.equal(out, got)


def test_attention_seg_rejections(gpu):
    lib = _C.load()
    q = torch.zeros((2, 64, 128), device=gpu, dtype=torch.bfloat16)
    kv = torch.zeros((2, 77, 128), device=gpu, dtype=torch.bfloat16)
    row = _row(gpu, 1.0, 8, 8)
    with pytest.raises(ops.BackendError, match="T == S"):
        ops.attention_seg(q, kv, kv, 2, 0.125, 1, (8, 8), row)
    with pytest.raises(ops.BackendError, match="token grid"):
        ops.attention_seg(q, q, q, 2, 0.125, 1, (8, 4), row)
    with pytest.raises(ops.BackendError, match="tail_count"):
        ops.attention_seg(q, q, q, 2, 0.125, 3, (8, 8), row)
    with pytest.raises(ops.BackendError, match="tail_count"):
        ops.attention_seg(q, q, q, 2, 0.125, -1, (8, 8), row)
    big = torch.zeros((1, 129 * 2, 64), device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ops.BackendError, match="larger than 128 x 128"):
        ops.attention_seg(big, big, big, 1, 0.125, 1, (129, 2), row)
    out, scratch = torch.empty_like(q), torch.empty_like(q)
    args = lambda **kw: [kw.get("q", q.data_ptr()), kv.data_ptr(), kw.get("v", kv.data_ptr()), out.data_ptr(), kw.get("scratch", scratch.data_ptr()),
                         2, 64, kw.get("S", 77), 2, 64, 128, 128, kw.get("ldv", 128), 128, 0.125, _C.ST_BF16, kw.get("tail", 1),
                         kw.get("h", 8), 8, row.data_ptr(), None, 0, None]
    assert lib.st_attention_seg(*args()) != 0 and b"T == S" in lib.st_last_error()
    assert lib.st_attention_seg(*args(S=64, h=4)) != 0 and b"token grid" in lib.st_last_error()
    assert lib.st_attention_seg(*args(S=64, tail=3)) != 0 and b"tail_count" in lib.st_last_error()
    assert lib.st_attention_seg(*args(S=64, ldv=132)) != 0 and b"16-byte" in lib.st_last_error()
    assert lib.st_attention_seg(*args(S=64, v=q.data_ptr() + 2)) != 0 and b"16-byte" in lib.st_last_error()
    assert lib.st_attention_seg(*args(S=64, scratch=scratch.data_ptr() + 2)) != 0 and b"16-byte" in lib.st_last_error()
    # T != S without a tail is ordinary cross-attention
    got = ops.attention_seg(q, kv, kv, 2, 0.125, 0, (8, 8), row)
    assert torch.equal(got, ops.attention(q, kv, kv, 2, 0.125))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "dense"])
@pytest.mark.parametrize("tail", [1, 3])
def test_attention_seg_split_image_is_complete(gpu, fused, tail):
    """Strict mode: the image the two attention launches leave for the output projection equals st_split_f32 of the output, every row."""
    B, h, w, H, D = 3, 8, 12, 2, 64
    T = h * w
    q, k, v = _qkv(gpu, torch.float32, B, T, H, D, fused)
    out = ops.attention_seg(q, k, v, H, D ** -0.5, tail, (h, w), _row(gpu, 1.0, h, w))
    note = ops._split_notes(out.device)[-1]
    assert note[0] is out and note[2:4] == (B * T, H * D), "the producer's image must have been noted"
    fresh = ops.split_rows(out.view(B * T, H * D)).s
    assert torch.equal(note[4].view(torch.int32), fresh.view(torch.int32))


def test_strict_step_with_and_without_emitted_images(gpu):
    """An fp32 compiled TINY step with SEG: producers' split images on (the K / V images of the fused projection feed BOTH attention
    launches of a site through st_attention_split) against every consumer splitting for itself - the same bits."""
    from stabletriton_amd.optimization import optimize_model
    from stabletriton_amd.unet import TINY, UNet2DConditionModel
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False).to(gpu, torch.float32)
    synth.fill_module_(m, 0)
    gm = optimize_model(m, cuda_graph=False, seg_layers=("down_blocks.1", "mid"))
    assert gm.rewrite_stats["seg_sites"] == 4
    x = synth.denoise_inputs(3, 16, 1234, cross_dim=TINY.cross_dim, pooled_dim=TINY.pooled_dim)
    args = (x["latent"].to(gpu), torch.tensor(500.0, device=gpu), x["encoder_hidden_states"].to(gpu),
            {"text_embeds": x["text_embeds"].to(gpu), "time_ids": x["time_ids"].to(gpu)})
    gm.seg.bind((16, 16), gpu)
    outs = {}
    keep = ops.EMIT_SPLIT
    try:
        for emit in (True, False):
            ops.EMIT_SPLIT = emit
            with torch.no_grad(), gm.seg.using(3, (16, 16)):
                outs[emit] = gm(*args)[0].clone()
        with torch.no_grad():
            plain = gm(*args)[0].clone()
    finally:
        ops.EMIT_SPLIT = keep
    assert torch.equal(outs[True], outs[False])
    # the unperturbed rows are the plain module's (the attention launch sees a sub-batch: the project's strict gate, not bits)
    assert float((outs[True][:2] - plain[:2]).abs().max()) <= 1e-3 and float((outs[True][2] - plain[2]).abs().max()) > 1e-2
