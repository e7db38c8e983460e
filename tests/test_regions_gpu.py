"""Regional cross-attention, the kernel: st_attention_regions / ops.attention_regions (csrc/attention_regions.hip) against
ops.attention on the segment slices - bit for bit with one-hot weights, and for general weights inside a bound made of the
roundings alone (below) - segment independence, the slow path (fp32, head size 32), and the entry point's rejections."""
import pytest
import torch

from stabletriton_amd import _C, ops, synth
from tests.test_pag_gpu import ROUND          # (relative, absolute) rounding error of a stored value, per dtype

pytestmark = pytest.mark.gpu
D = 64
# (B, T, H, R, L):
#   (2, 96, 2, 2, 77)   T no multiple of the 64-row block; the tail tile's masked keys are the next segment's real keys
#   (3, 256, 4, 3, 77)  several blocks; odd R: the ring's slot parity across the seams
#   (1, 64, 1, 4, 64)   one whole tile per segment (no tail at all)
#   (2, 128, 2, 2, 150) three tiles per segment: the ring wraps inside a segment
#   (1, 48, 1, 1, 77)   R = 1, less than one block of rows
SHAPES = [(2, 96, 2, 2, 77), (3, 256, 4, 3, 77), (1, 64, 1, 4, 64), (2, 128, 2, 2, 150), (1, 48, 1, 1, 77)]
DTYPES = [torch.bfloat16, torch.float16]


def _qkv(gpu, dtype, B, T, H, R, L, sliced, d=D):
    """q (B, T, C), k / v (B, R*L, C): dense, or column slices of wider buffers (q beside 64 other columns, k | v side by side as the
    fused context projection leaves them)."""
    C = H * d
    tag = f"{B}.{T}.{H}.{R}.{L}.{d}"
    if sliced:
        qb = synth.normal(f"regions.qbuf.{tag}", (B, T, C + 64), 3).to(gpu, dtype)
        kv = synth.normal(f"regions.kvbuf.{tag}", (B, R * L, 2 * C), 4).to(gpu, dtype)
        return qb[..., 64:], kv[..., :C], kv[..., C:]
    q = synth.normal(f"regions.q.{tag}", (B, T, C), 3).to(gpu, dtype)
    k = synth.normal(f"regions.k.{tag}", (B, R * L, C), 4).to(gpu, dtype)
    v = synth.normal(f"regions.v.{tag}", (B, R * L, C), 5).to(gpu, dtype)
    return q, k, v


def _segments(q, k, v, H, scale, R, L):
    """A_r = ops.attention on segment r's slice (the existing launch, not the code under test), float64 on the host."""
    return [ops.attention(q, k[:, r * L:(r + 1) * L], v[:, r * L:(r + 1) * L], H, scale) for r in range(R)]


def _weights(kind, B, R, T, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((B, R, T), generator=g)
    if kind == "normalised":
        return w / w.sum(dim=1, keepdim=True)
    if kind == "zeros":                               # rows where whole segments have weight exactly 0, the rest normalised
        w = w * (torch.rand((B, R, T), generator=g) > 0.5)
        w[:, 0] += (w.sum(dim=1) == 0).float()
        return w / w.sum(dim=1, keepdim=True)
    w = w * 3.0 - 1.0                                 # un-normalised: negative values, values above 1
    w[:, 0, 0] = 1.7
    w[:, R - 1, T - 1] = -0.6
    return w


def _check_bound(got, segs, w, dtype, what):
    """|got - want| <= rho (|want| + sum |w_r| |A_r|) + 2^-20 sum |w_r| |A_r| + a, elementwise: one rounding per A_r (the kernel sums the
    un-rounded segment results, the reference the rounded ones), one for the output, and the fp32 accumulation; (rho, a) = ROUND."""
    rho, a = ROUND[dtype]
    w64 = w.double().cpu()
    want = sum(w64[:, r].unsqueeze(-1) * s.double().cpu() for r, s in enumerate(segs))
    mag = sum(w64[:, r].abs().unsqueeze(-1) * s.double().cpu().abs() for r, s in enumerate(segs))
    err = (got.double().cpu() - want).abs()
    slack = rho * (want.abs() + mag) + 2.0 ** -20 * mag + a
    worst = float((err / slack).max())
    print(f"{what}: max abs err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert torch.isfinite(got).all(), what
    assert float((err - slack).max()) <= 0.0, f"{what}: max abs err {float(err.max()):.3e}, worst err / bound {worst:.3f}"


def _margins_intact(buf, pad):
    return bool(torch.all(buf[:pad] == buf[0]) and torch.all(buf[-pad:] == buf[0]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_hot_weights_are_attention_on_the_segment(gpu, dtype, sliced, shape):
    B, T, H, R, L = shape
    C = H * D
    q, k, v = _qkv(gpu, dtype, B, T, H, R, L, sliced)
    scale = D ** -0.5
    segs = _segments(q, k, v, H, scale, R, L)
    lib = _C.load()
    for r in range(R):
        w = torch.zeros((B, R, T), device=gpu)
        w[:, r] = 1.0
        got = ops.attention_regions(q, k, v, w, H, scale, L)
        assert torch.equal(got, segs[r]), f"one-hot on segment {r} differs from ops.attention on its slice"
        assert torch.equal(got, ops.attention_regions(q, k, v, w, H, scale, L)), "two calls differ"
        # the entry point itself, into a guarded output: nothing outside `out`
        pad = 256
        buf = torch.full((B * T * C + 2 * pad,), -77.0, dtype=dtype, device=gpu)
        out = buf[pad:pad + B * T * C].view(B, T, C)
        _C.check(lib.st_attention_regions(q.data_ptr(), k.data_ptr(), v.data_ptr(), w.data_ptr(), out.data_ptr(), B, T, R, L, H, D,
                                          q.stride(1), k.stride(1), v.stride(1), C, float(scale), _C.dtype_code(dtype), _C.stream_ptr()),
                 "attention_regions")
        torch.cuda.synchronize()
        assert _margins_intact(buf, pad), "write outside the tensor"
        assert torch.equal(out, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_weighted_sum_within_the_rounding_bound(gpu, dtype, sliced, shape):
    B, T, H, R, L = shape
    q, k, v = _qkv(gpu, dtype, B, T, H, R, L, sliced)
    scale = D ** -0.5
    segs = _segments(q, k, v, H, scale, R, L)
    for i, kind in enumerate(("normalised", "zeros", "unnormalised")):
        w = _weights(kind, B, R, T, 11 + i).to(gpu)
        got = ops.attention_regions(q, k, v, w, H, scale, L)
        assert torch.equal(got, ops.attention_regions(q, k, v, w, H, scale, L)), "two calls differ"
        _check_bound(got, segs, w, dtype, f"{shape} {dtype} sliced={sliced} {kind}")
        if kind == "zeros" and R > 1:
            assert bool((w == 0).any())
            # a row whose other segments all have weight 0 is that segment's attention row exactly
            alone = (w == 1.0)
            for r in range(R):
                rows = alone[:, r]
                if bool(rows.any()):
                    assert torch.equal(got[rows], segs[r][rows]), f"weight 1 on segment {r}, 0 elsewhere: that segment's bits"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 96, 2, 2, 77), (3, 256, 4, 3, 77), (2, 128, 2, 2, 150)])
def test_segments_share_no_softmax_state(gpu, dtype, shape):
    """Segment 0's keys times 8: its scores dwarf every other segment's.  A running maximum or row sum shared between segments would
    wipe the others out (or overflow); with their own, every output stays finite and inside the same bound."""
    B, T, H, R, L = shape
    q, k, v = _qkv(gpu, dtype, B, T, H, R, L, False)
    k = k.clone()
    k[:, :L] *= 8.0
    scale = D ** -0.5
    segs = _segments(q, k, v, H, scale, R, L)
    w = _weights("normalised", B, R, T, 29).to(gpu)
    got = ops.attention_regions(q, k, v, w, H, scale, L)
    _check_bound(got, segs, w, dtype, f"{shape} {dtype} segment 0 keys x 8")
    # the other segments must matter: without segment 0 the result moves by much more than the bound
    rest = sum(w[:, r].unsqueeze(-1).double().cpu() * segs[r].double().cpu() for r in range(1, R))
    assert float(rest.abs().max()) > 0.05


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 128, 2), (2, 256, 4)])
def test_off_pair_is_the_fused_query_projection_and_attention(gpu, dtype, shape):
    """What holds a compiled-in-but-off regional model to the bits of the model compiled without regions where that model takes
    the ONE-launch form: st_ln_linear_xattn (the attention core as a GEMM epilogue, another translation unit) against
    ln_linear + st_attention_regions with weight 1 on segment 0, second segment a different prompt."""
    B, T, H = shape
    C, L = H * D, 77
    tag = f"{B}.{T}.{H}"
    x0 = synth.normal(f"regions.xattn.x.{tag}", (B, T, C), 21).to(gpu, dtype)
    wp = (synth.normal(f"regions.xattn.wp.{tag}", (C, C), 22) * C ** -0.5).to(gpu, dtype)
    res = synth.normal(f"regions.xattn.res.{tag}", (B, T, C), 23).to(gpu, dtype)
    x, stats = ops.linear(x0, wp, None, residual=res, emit_stats=True)
    wq = (synth.normal(f"regions.xattn.wq.{tag}", (C, C), 24) * C ** -0.5).to(gpu, dtype)
    bq = (synth.normal(f"regions.xattn.bq.{tag}", (C,), 25) * 0.1).to(gpu, dtype)
    gamma = (1.0 + 0.1 * synth.normal(f"regions.xattn.g.{tag}", (C,), 26)).to(gpu, dtype)
    beta = (0.1 * synth.normal(f"regions.xattn.b.{tag}", (C,), 27)).to(gpu, dtype)
    wf, c, d = ops.fold_layer_norm(gamma, beta, wq, bq)
    kv = synth.normal(f"regions.xattn.kv.{tag}", (B, 2 * L, 2 * C), 28).to(gpu, dtype)
    k, v = kv[..., :C], kv[..., C:]
    k1, v1 = k[:, :L].contiguous(), v[:, :L].contiguous()
    scale = D ** -0.5
    assert ops.xattn_fusable(x, k1, H)
    fused = ops.ln_linear_xattn(x, stats, wf, c, d, 1e-5, k1, v1, H, scale)
    w = torch.zeros((B, 2, T), device=gpu)
    w[:, 0] = 1.0
    q = ops.ln_linear(x, stats, wf, c, d, 1e-5)
    off = ops.attention_regions(q, k, v, w, H, scale, L)
    assert torch.isfinite(fused).all()
    assert torch.equal(off, fused), f"{int((off != fused).sum())} of {off.numel()} values differ from the fused launch"


@pytest.mark.parametrize("dtype,d", [(torch.float32, 64), (torch.bfloat16, 32)])
def test_slow_path(gpu, dtype, d):
    """fp32 (strict mode) and the other head sizes: R attention launches and a torch fp32 weighted sum, rounded once."""
    B, T, H, R, L = 2, 96, 2, 2, 77
    q, k, v = _qkv(gpu, dtype, B, T, H, R, L, True, d)
    scale = d ** -0.5
    segs = _segments(q, k, v, H, scale, R, L)
    for r in range(R):
        w = torch.zeros((B, R, T), device=gpu)
        w[:, r] = 1.0
        assert torch.equal(ops.attention_regions(q, k, v, w, H, scale, L), segs[r])
    for i, kind in enumerate(("normalised", "zeros", "unnormalised")):
        w = _weights(kind, B, R, T, 41 + i).to(gpu)
        got = ops.attention_regions(q, k, v, w, H, scale, L)
        assert got.dtype == dtype
        _check_bound(got, segs, w, dtype, f"slow path {dtype} D={d} {kind}")
    if dtype == torch.float32:
        # the result is a torch tensor without a split image: a GEMM that consumes it splits it itself, and gets the bits it gets
        # from a fresh copy (whose memory no producer can have noted)
        w = _weights("normalised", B, R, T, 47).to(gpu)
        got = ops.attention_regions(q, k, v, w, H, scale, L)
        assert all(ent[0] is not got for ent in ops._split_notes(got.device))
        wt = synth.normal("regions.slow.proj", (H * d, H * d), 9).to(gpu) * (H * d) ** -0.5
        assert torch.equal(ops.linear(got, wt), ops.linear(got.clone(), wt))


def test_ops_argument_errors(gpu):
    q = torch.zeros((2, 64, 128), device=gpu, dtype=torch.bfloat16)
    kv = torch.zeros((2, 154, 128), device=gpu, dtype=torch.bfloat16)
    w = torch.zeros((2, 2, 64), device=gpu)
    for bad in (w[:, :, :32], w[:1], w.half(), w[0]):
        with pytest.raises(ops.BackendError, match="weights"):
            ops.attention_regions(q, kv, kv, bad, 2, 0.125, 77)
    with pytest.raises(ops.BackendError, match=r"R\*seg_len"):
        ops.attention_regions(q, kv, kv, w, 2, 0.125, 64)
    with pytest.raises(ops.BackendError, match=r"R\*seg_len"):
        ops.attention_regions(q, kv, kv[:, :77], w, 2, 0.125, 77)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.attention_regions(q.cpu(), kv, kv, w, 2, 0.125, 77)
    nine = torch.zeros((2, 9, 64), device=gpu)
    with pytest.raises(ops.BackendError, match="R 9"):
        ops.attention_regions(q, torch.zeros((2, 9 * 8, 128), device=gpu, dtype=torch.bfloat16),
                              torch.zeros((2, 9 * 8, 128), device=gpu, dtype=torch.bfloat16), nine, 2, 0.125, 8)


def test_entry_point_rejections(gpu):
    lib = _C.load()
    B, T, H, R, L = 2, 64, 2, 2, 77
    q = torch.zeros((B, T, 128), device=gpu, dtype=torch.bfloat16)
    kv = torch.zeros((B, 9 * 256, 128), device=gpu, dtype=torch.bfloat16)      # large enough for every (R, seg_len) tried below
    w = torch.zeros((B, 9, T), device=gpu)
    out = torch.empty_like(q)

    def call(**kw):
        a = dict(q=q.data_ptr(), k=kv.data_ptr(), v=kv.data_ptr(), w=w.data_ptr(), out=out.data_ptr(), R=R, L=L, D=64, ldq=128, ldk=128,
                 ldv=128, ldo=128, dtype=_C.ST_BF16)
        a.update(kw)
        return lib.st_attention_regions(a["q"], a["k"], a["v"], a["w"], a["out"], B, T, a["R"], a["L"], H, a["D"], a["ldq"], a["ldk"],
                                        a["ldv"], a["ldo"], 0.125, a["dtype"], None)

    for kw, word in ((dict(dtype=_C.ST_F32), b"dtype"), (dict(D=32), b"head_dim"), (dict(R=9), b"R 9"), (dict(L=256), b"seg_len 256"),
                     (dict(w=None), b"weights"), (dict(k=kv.data_ptr() + 2), b"k must be 16-byte"), (dict(ldv=132), b"ldv 132")):
        assert call(**kw) != 0, kw
        assert word in lib.st_last_error(), (kw, lib.st_last_error())
    assert call() == 0
    torch.cuda.synchronize()
