"""Ragged segmented cross-attention, the kernel: st_attention_segments / ops.attention_segments (csrc/attention_segments.hip)
against ops.attention on every segment - bit for bit under a one-hot scale, bit for bit against the regional kernel where that can
express the call, and for general weights and scales inside the regional test's bound of the roundings alone - the skip rule, the
barrier rule (segment 0 skipped), segment independence, the fused off pair, a captured launch that follows in-place writes, the slow
path and the rejections."""
import pytest
import torch

from stabletriton_amd import _C, ops, synth
from tests.test_pag_gpu import ROUND          # noqa: F401  (the bound's constants, used by _check_bound)
from tests.test_regions_gpu import SHAPES as REGION_SHAPES
from tests.test_regions_gpu import _check_bound, _margins_intact
from tests.test_regions_gpu import _qkv as _region_qkv
from tests.test_regions_gpu import _weights as _region_weights

pytestmark = pytest.mark.gpu
D = 64
# (B, T, H, lens):
#   (2, 96, 2, (77, 4))        T no multiple of the 64-row block; a 4-key segment behind a tail tile
#   (1, 64, 1, (77, 16))       the Plus token count
#   (3, 256, 4, (77, 16, 4))   odd S: the ring's slot parity across the seams
#   (2, 128, 2, (150, 77, 1))  the ring wraps inside a segment; a length of 1
#   (1, 48, 1, (64, 64))       whole tiles, less than one block of rows
SHAPES = [(2, 96, 2, (77, 4)), (1, 64, 1, (77, 16)), (3, 256, 4, (77, 16, 4)), (2, 128, 2, (150, 77, 1)), (1, 48, 1, (64, 64))]
DTYPES = [torch.bfloat16, torch.float16]
FORMS = ["dense", "sliced"]


def _inputs(gpu, dtype, B, T, H, lens, form, d=D):
    """q (B, T, C) and one (k, v) pair per segment: all dense tensors, or ("sliced") the text segment as the k | v column halves of
    one (B, L, 2C) buffer and every image segment as the halves of its own (B, N, 2C) buffer - another token stride and another
    batch stride per segment, as the hoisted context cache and the adapter state leave them."""
    C = H * d
    tag = f"{B}.{T}.{H}.{'-'.join(map(str, lens))}.{d}"
    q = synth.normal(f"ipseg.q.{tag}", (B, T, C), 3).to(gpu, dtype)
    segs = []
    for r, n in enumerate(lens):
        if form == "sliced":
            kv = synth.normal(f"ipseg.kv{r}.{tag}", (B, n, 2 * C), 4 + r).to(gpu, dtype)
            segs.append((kv[..., :C], kv[..., C:]))
        else:
            segs.append((synth.normal(f"ipseg.k{r}.{tag}", (B, n, C), 4 + r).to(gpu, dtype),
                         synth.normal(f"ipseg.v{r}.{tag}", (B, n, C), 14 + r).to(gpu, dtype)))
    return q, segs


def _each(q, segs, H, scale):
    """A_r = ops.attention on segment r (the existing launch, not the code under test)."""
    return [ops.attention(q, k, v, H, scale) for k, v in segs]


def _w_eff(w, sc):
    """fl32(seg_scale[r] * weights[b,r,t]) in fp32 torch."""
    return w.float() * sc.float()[None, :, None]


def _general(B, S, T, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((B, S, T), generator=g) * 2.0 - 0.5          # negative values, values above 1
    w[:, 0, 0] = 1.7
    sc = torch.rand((S,), generator=g) * 3.0 - 1.0              # negative scales, scales above 1
    sc[0] = 1.0
    sc[S - 1] = -0.6 if S > 1 else 1.0
    return w, sc


def _raw(lib, q, segs, S, w, sc, out, B, T, H, scale, dtype):
    table = (_C.KVSegment * S)()
    for r, (k, v) in enumerate(segs):
        table[r] = _C.KVSegment(k.data_ptr(), v.data_ptr(), k.stride(1), v.stride(1), k.stride(0), v.stride(0), k.shape[1])
    return lib.st_attention_segments(q.data_ptr(), table, S, w.data_ptr(), None if sc is None else sc.data_ptr(), out.data_ptr(), B, T, H, D,
                                     q.stride(1), H * D, float(scale), _C.dtype_code(dtype), _C.stream_ptr())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_one_hot_scale_is_attention_on_the_segment(gpu, dtype, form, shape):
    B, T, H, lens = shape
    C, S = H * D, len(lens)
    q, segs = _inputs(gpu, dtype, B, T, H, lens, form)
    scale = D ** -0.5
    each = _each(q, segs, H, scale)
    ones = torch.ones((B, S, T), device=gpu)
    lib = _C.load()
    for r in range(S):
        sc = torch.zeros(S, device=gpu)
        sc[r] = 1.0
        got = ops.attention_segments(q, segs, ones, sc, H, scale)
        assert torch.equal(got, each[r]), f"one-hot on segment {r} (len {lens[r]}) differs from ops.attention on it"
        assert torch.equal(got, ops.attention_segments(q, segs, ones, sc, H, scale)), "two calls differ"
        # the same through the weights alone (no segment skipped: fma(0, y, x) = x)
        w = torch.zeros((B, S, T), device=gpu)
        w[:, r] = 1.0
        assert torch.equal(ops.attention_segments(q, segs, w, None, H, scale), each[r])
        # the entry point itself, into a guarded output: nothing outside `out`
        pad = 256
        buf = torch.full((B * T * C + 2 * pad,), -77.0, dtype=dtype, device=gpu)
        out = buf[pad:pad + B * T * C].view(B, T, C)
        _C.check(_raw(lib, q, segs, S, ones, sc, out, B, T, H, scale, dtype), "attention_segments")
        torch.cuda.synchronize()
        assert _margins_intact(buf, pad), "write outside the tensor"
        assert torch.equal(out, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", REGION_SHAPES)
def test_equal_lengths_in_one_buffer_are_the_regional_kernel(gpu, dtype, shape):
    B, T, H, R, L = shape
    q, k, v = _region_qkv(gpu, dtype, B, T, H, R, L, False)
    segs = [(k[:, r * L:(r + 1) * L], v[:, r * L:(r + 1) * L]) for r in range(R)]
    scale = D ** -0.5
    for i, kind in enumerate(("normalised", "zeros", "unnormalised")):
        w = _region_weights(kind, B, R, T, 11 + i).to(gpu)
        want = ops.attention_regions(q, k, v, w, H, scale, L)
        got = ops.attention_segments(q, segs, w, None, H, scale)
        assert torch.equal(got, want), f"{shape} {dtype} {kind}: {int((got != want).sum())} of {got.numel()} values differ from the regional kernel"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_weights_times_scales_within_the_rounding_bound(gpu, dtype, form, shape):
    B, T, H, lens = shape
    S = len(lens)
    q, segs = _inputs(gpu, dtype, B, T, H, lens, form)
    scale = D ** -0.5
    each = _each(q, segs, H, scale)
    for seed in (11, 12):
        w, sc = _general(B, S, T, seed)
        assert bool((sc < 0).any()) or S == 1
        got = ops.attention_segments(q, segs, w.to(gpu), sc.to(gpu), H, scale)
        assert torch.equal(got, ops.attention_segments(q, segs, w.to(gpu), sc.to(gpu), H, scale)), "two calls differ"
        _check_bound(got, each, _w_eff(w, sc), dtype, f"{shape} {dtype} {form} seed {seed}")
        # host floats fold into the weights with the same single fp32 rounding
        assert torch.equal(ops.attention_segments(q, segs, w.to(gpu), sc.tolist(), H, scale), got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_segment_at_scale_0_is_skipped(gpu, dtype, form, shape):
    """Its K / V are never read (all NaN here), the result is the call without it - also when it is segment 0, where a barrier rule
    of `r > 0` would put a barrier in front of the first segment that runs and none in front of the second - and all scales 0 is 0."""
    B, T, H, lens = shape
    S = len(lens)
    q, segs = _inputs(gpu, dtype, B, T, H, lens, form)
    scale = D ** -0.5
    w, sc = _general(B, S, T, 21)
    w = w.to(gpu)
    for skip in range(S):
        poisoned = list(segs)
        if form == "sliced":
            kv = torch.full((B, lens[skip], 2 * H * D), float("nan"), dtype=dtype, device=gpu)
            poisoned[skip] = (kv[..., :H * D], kv[..., H * D:])
        else:
            poisoned[skip] = (torch.full_like(segs[skip][0], float("nan")), torch.full_like(segs[skip][1], float("nan")))
        s0 = sc.clone()
        s0[skip] = 0.0
        got = ops.attention_segments(q, poisoned, w, s0.to(gpu), H, scale)
        assert torch.isfinite(got).all(), f"segment {skip} at scale 0 was read"
        keep = [r for r in range(S) if r != skip]
        if keep:
            want = ops.attention_segments(q, [segs[r] for r in keep], w[:, keep].contiguous(), s0[keep].to(gpu), H, scale)
            assert torch.equal(got, want), f"skipping segment {skip} differs from the call without it"
        # for finite data the skip is the bits of the non-skipping form: weight 0 instead of scale 0
        w0 = w.clone()
        w0[:, skip] = 0.0
        s1 = sc.clone()
        s1[skip] = 1.0
        assert torch.equal(ops.attention_segments(q, segs, w0, s1.to(gpu), H, scale), ops.attention_segments(q, segs, w, s0.to(gpu), H, scale))
    zeros = ops.attention_segments(q, segs, w, torch.zeros(S, device=gpu), H, scale)
    assert torch.equal(zeros, torch.zeros_like(q)), "every segment skipped: zeros"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 96, 2, (77, 4)), (3, 256, 4, (77, 16, 4)), (2, 128, 2, (150, 77, 1))])
def test_segments_share_no_softmax_state(gpu, dtype, shape):
    """Segment 0's keys times 8: its scores dwarf every other segment's.  A running maximum or row sum shared between segments would
    wipe the others out (or overflow); with their own, every output stays finite and inside the same bound."""
    B, T, H, lens = shape
    S = len(lens)
    q, segs = _inputs(gpu, dtype, B, T, H, lens, "dense")
    segs[0] = (segs[0][0] * 8.0, segs[0][1])
    scale = D ** -0.5
    each = _each(q, segs, H, scale)
    w = torch.rand((B, S, T), generator=torch.Generator().manual_seed(29))
    sc = torch.tensor([1.0] + [0.8] * (S - 1))
    got = ops.attention_segments(q, segs, w.to(gpu), sc.to(gpu), H, scale)
    _check_bound(got, each, _w_eff(w, sc), dtype, f"{shape} {dtype} segment 0 keys x 8")
    rest = sum(_w_eff(w, sc)[:, r].unsqueeze(-1).double() * each[r].double().cpu() for r in range(1, S))
    assert float(rest.abs().max()) > 0.05, "the other segments must matter"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 128, 2), (2, 256, 4)])
def test_off_pair_is_the_fused_query_projection_and_attention(gpu, dtype, shape):
    """What holds a compiled-in-but-off IP-Adapter model to the bits of the model compiled without it where that model takes the
    ONE-launch form: st_ln_linear_xattn against ln_linear + st_attention_segments with scales (1, 0)."""
    B, T, H = shape
    C, L, N = H * D, 77, 4
    tag = f"{B}.{T}.{H}"
    x0 = synth.normal(f"ipseg.xattn.x.{tag}", (B, T, C), 21).to(gpu, dtype)
    wp = (synth.normal(f"ipseg.xattn.wp.{tag}", (C, C), 22) * C ** -0.5).to(gpu, dtype)
    res = synth.normal(f"ipseg.xattn.res.{tag}", (B, T, C), 23).to(gpu, dtype)
    x, stats = ops.linear(x0, wp, None, residual=res, emit_stats=True)
    wq = (synth.normal(f"ipseg.xattn.wq.{tag}", (C, C), 24) * C ** -0.5).to(gpu, dtype)
    bq = (synth.normal(f"ipseg.xattn.bq.{tag}", (C,), 25) * 0.1).to(gpu, dtype)
    gamma = (1.0 + 0.1 * synth.normal(f"ipseg.xattn.g.{tag}", (C,), 26)).to(gpu, dtype)
    beta = (0.1 * synth.normal(f"ipseg.xattn.b.{tag}", (C,), 27)).to(gpu, dtype)
    wf, c, d = ops.fold_layer_norm(gamma, beta, wq, bq)
    kv = synth.normal(f"ipseg.xattn.kv.{tag}", (B, L, 2 * C), 28).to(gpu, dtype)
    img = synth.normal(f"ipseg.xattn.img.{tag}", (B, N, 2 * C), 29).to(gpu, dtype)
    k, v = kv[..., :C], kv[..., C:]
    k1, v1 = k.contiguous(), v.contiguous()
    scale = D ** -0.5
    assert ops.xattn_fusable(x, k1, H)
    fused = ops.ln_linear_xattn(x, stats, wf, c, d, 1e-5, k1, v1, H, scale)
    q = ops.ln_linear(x, stats, wf, c, d, 1e-5)
    off = ops.attention_segments(q, [(k, v), (img[..., :C], img[..., C:])], torch.ones((B, 2, T), device=gpu),
                                 torch.tensor([1.0, 0.0], device=gpu), H, scale)
    assert torch.isfinite(fused).all()
    assert torch.equal(off, fused), f"{int((off != fused).sum())} of {off.numel()} values differ from the fused launch"


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_captured_launch_follows_in_place_writes(gpu, dtype):
    B, T, H, lens = 2, 96, 2, (77, 4)
    S = len(lens)
    q, segs = _inputs(gpu, dtype, B, T, H, lens, "sliced")
    scale = D ** -0.5
    w = torch.ones((B, S, T), device=gpu)
    sc = torch.tensor([1.0, 0.0], device=gpu)
    ops.attention_segments(q, segs, w, sc, H, scale)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.attention_segments(q, segs, w, sc, H, scale)
    g.replay()
    assert torch.equal(out, ops.attention(q, segs[0][0], segs[0][1], H, scale)), "off: the text attention"
    w2, sc2 = _general(B, S, T, 31)
    for new_w, new_sc in ((w2, sc2), (w2.flip(2), torch.tensor([1.0, 0.6])), (torch.ones(B, S, T), torch.tensor([1.0, 0.0]))):
        w.copy_(new_w)
        sc.copy_(new_sc)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.attention_segments(q, segs, w, sc, H, scale)), "the replay must follow seg_scale and weights"
    assert torch.equal(out, ops.attention(q, segs[0][0], segs[0][1], H, scale))


@pytest.mark.parametrize("dtype,d", [(torch.float32, 64), (torch.bfloat16, 32)])
def test_slow_path(gpu, dtype, d):
    """fp32 (strict mode) and the other head sizes: S attention launches and a torch fp32 weighted sum, rounded once."""
    B, T, H, lens = 2, 96, 2, (77, 4)
    S = len(lens)
    q, segs = _inputs(gpu, dtype, B, T, H, lens, "sliced", d)
    scale = d ** -0.5
    each = _each(q, segs, H, scale)
    ones = torch.ones((B, S, T), device=gpu)
    for r in range(S):
        sc = torch.zeros(S)
        sc[r] = 1.0
        assert torch.equal(ops.attention_segments(q, segs, ones, sc.to(gpu), H, scale), each[r])
        assert torch.equal(ops.attention_segments(q, segs, ones, sc.tolist(), H, scale), each[r])
    w, sc = _general(B, S, T, 41)
    got = ops.attention_segments(q, segs, w.to(gpu), sc.to(gpu), H, scale)
    assert got.dtype == dtype
    _check_bound(got, each, _w_eff(w, sc), dtype, f"slow path {dtype} D={d}")
    # host floats skip: the segment at 0 may hold anything; a device table multiplies (finite K / V are the caller's duty)
    nan = torch.full_like(segs[1][0], float("nan"))
    assert torch.equal(ops.attention_segments(q, [segs[0], (nan, nan)], ones, [1.0, 0.0], H, scale), each[0])
    assert torch.equal(ops.attention_segments(q, segs, ones, [0.0, 0.0], H, scale), torch.zeros_like(q))


def test_ops_argument_errors(gpu):
    q = torch.zeros((2, 64, 128), device=gpu, dtype=torch.bfloat16)
    text = torch.zeros((2, 77, 128), device=gpu, dtype=torch.bfloat16)
    img = torch.zeros((2, 4, 128), device=gpu, dtype=torch.bfloat16)
    segs = [(text, text), (img, img)]
    w = torch.ones((2, 2, 64), device=gpu)
    sc = torch.ones(2, device=gpu)
    for bad in (w[:, :, :32], w[:1], w.half(), w[0], torch.ones((2, 3, 64), device=gpu)):
        with pytest.raises(ops.BackendError, match="weights"):
            ops.attention_segments(q, segs, bad, sc, 2, 0.125)
    for bad in (torch.ones(3, device=gpu), sc.half(), [1.0], torch.ones(4, device=gpu)[::2]):
        with pytest.raises(ops.BackendError, match="seg_scale"):
            ops.attention_segments(q, segs, w, bad, 2, 0.125)
    with pytest.raises(ops.BackendError, match="segment 1"):
        ops.attention_segments(q, [(text, text), (img, img[:, :2])], w, sc, 2, 0.125)
    with pytest.raises(ops.BackendError, match="segment 1.*dtype"):
        ops.attention_segments(q, [(text, text), (img.half(), img.half())], w, sc, 2, 0.125)
    with pytest.raises(ops.BackendError, match="segment 0"):
        ops.attention_segments(q, [(text[:1], text[:1]), (img, img)], w, sc, 2, 0.125)
    with pytest.raises(ops.BackendError, match="pairs"):
        ops.attention_segments(q, [text, img], w, sc, 2, 0.125)
    with pytest.raises(ops.BackendError, match="S 9"):
        ops.attention_segments(q, [(img, img)] * 9, torch.ones((2, 9, 64), device=gpu), None, 2, 0.125)
    with pytest.raises(ops.BackendError, match="no CPU fallback"):
        ops.attention_segments(q.cpu(), segs, w, sc, 2, 0.125)
    long = torch.zeros((2, 256, 128), device=gpu, dtype=torch.bfloat16)
    with pytest.raises(ops.BackendError, match="segment 1: len 256"):
        ops.attention_segments(q, [(text, text), (long, long)], w, sc, 2, 0.125)


def test_entry_point_rejections(gpu):
    lib = _C.load()
    B, T, H = 2, 64, 2
    q = torch.zeros((B, T, 128), device=gpu, dtype=torch.bfloat16)
    kv = torch.zeros((B, 256, 128), device=gpu, dtype=torch.bfloat16)
    w = torch.ones((B, 8, T), device=gpu)
    sc = torch.ones(8, device=gpu)
    out = torch.empty_like(q)

    def call(segs=({}, dict(len=4)), **kw):
        a = dict(q=q.data_ptr(), w=w.data_ptr(), sc=sc.data_ptr(), out=out.data_ptr(), D=64, ldq=128, ldo=128, dtype=_C.ST_BF16, S=len(segs))
        a.update(kw)
        table = (_C.KVSegment * max(len(segs), 1))()
        for r, s in enumerate(segs):
            d = dict(k=kv.data_ptr(), v=kv.data_ptr(), ldk=128, ldv=128, bsk=256 * 128, bsv=256 * 128, len=77)
            d.update(s)
            table[r] = _C.KVSegment(d["k"], d["v"], d["ldk"], d["ldv"], d["bsk"], d["bsv"], d["len"])
        return lib.st_attention_segments(a["q"], table, a["S"], a["w"], a["sc"], a["out"], B, T, H, a["D"], a["ldq"], a["ldo"], 0.125, a["dtype"], None)

    for kw, word in ((dict(dtype=_C.ST_F32), b"dtype"), (dict(D=32), b"head_dim"), (dict(S=9), b"S 9"), (dict(w=None), b"weights"),
                     (dict(segs=({}, dict(len=256))), b"segment 1: len 256"), (dict(segs=(dict(k=kv.data_ptr() + 2),)), b"segment 0: k must be 16-byte"),
                     (dict(segs=({}, {}, dict(ldv=132))), b"segment 2: ldv 132"), (dict(segs=({}, dict(v=None))), b"segment 1: v is null")):
        assert call(**kw) != 0, kw
        assert word in lib.st_last_error(), (kw, lib.st_last_error())
    assert call() == 0
    assert call(sc=None) == 0, "seg_scale NULL = all 1"
    torch.cuda.synchronize()
