"""Kernels and tile edges the operator suite never launched: the register-staged ragged-K GEMM (csrc/gemm_reg.h), the generic
branch of the thin conv (csrc/conv_thin.h), halo / implicit-GEMM conv geometries other than square ones, GroupNorm / LayerNorm
vector and group edges, one attention case per kernel with a guarded output.  Short-K cases are gated per element against
float64 (tests/edge_util.py); every operand sits in NaN-poisoned memory, so a read outside it that reaches a result shows as NaN."""
import pytest
import torch
import torch.nn.functional as F

from stabletriton_amd import ops
from tests import edge_util as eu
from tests.util import HALF_DTYPES, assert_close

pytestmark = pytest.mark.gpu
DTYPES = eu.DTYPES
CL = torch.channels_last


def _name(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, (tuple, list)):
        return "-".join(str(int(e)) for e in v)
    return None


def _report(group, dtype, what, ratio):
    print(f"RATIO {group} {_name(dtype)} {what}: {ratio:.3f} of the budget")


def _dev(t, gpu, dtype, row_gap=0, cl=False):
    t = t.to(gpu, dtype)
    if cl:
        t = t.contiguous(memory_format=CL)
    return eu.poisoned(t, row_gap=row_gap)


# ================================================================================================ ragged-K linear (gemm_kernel)
def _linear_operands(M, K, rows):
    return eu.normal(f"e.x{M}.{K}", (M, K)), eu.normal(f"e.w{rows}.{K}", (rows, K), K ** -0.5), eu.normal(f"e.b{rows}", (rows,))


def _check_linear(gpu, dtype, M, K, N, *, bias=True, silu=False, geglu=False, residual=False, shape3d=None, group="linear"):
    rows = 2 * N if geglu else N
    x, w, b = _linear_operands(M, K, rows)
    r = eu.normal(f"e.r{M}.{N}", (M, N)) if residual else None
    xg = _dev(x, gpu, dtype, row_gap=eu.ROW_GAP) if shape3d is None else _dev(x.view(*shape3d, K), gpu, dtype)
    wg, bg = _dev(w, gpu, dtype), (_dev(b, gpu, dtype) if bias else None)
    rg = None if r is None else _dev(r if shape3d is None else r.view(*shape3d, N), gpu, dtype, row_gap=eu.ROW_GAP)
    out = ops.linear(xg, wg, bg, silu=silu, geglu=geglu, residual=rg)
    again = ops.linear(xg, wg, bg, silu=silu, geglu=geglu, residual=rg)
    assert torch.equal(out, again), "two launches of the same problem differ"
    ref, mag, extra = eu.linear_ref64(x, w, b if bias else None, dtype, silu=silu, geglu=geglu, residual=r)
    what = f"linear {(M, K, N)}" + ("+bias" if bias else "") + ("+silu" if silu else "") + ("+geglu" if geglu else "") + ("+residual" if residual else "")
    ratio = eu.assert_elementwise(out.reshape(M, N), ref, mag, K, dtype, what, extra)
    _report(group, dtype, what, ratio)
    return out, (xg, wg, bg, rg)


_LINEAR = [(d, s) for d in DTYPES for s in eu.linear_cases(d)]


@pytest.mark.parametrize("dtype,shape", _LINEAR, ids=_name)
def test_ragged_k_linear(gpu, dtype, shape):
    """K % 64 != 0 (16-bit) / K % 32 != 0 (fp32): gemm_kernel on 64 x 64 tiles, 128 x 64 at >= 200 of those tiles, 128 x 128 at
    >= 240; a single partial K tile (K = 8 / 4), ragged M and N on every tile, M = 1."""
    _check_linear(gpu, dtype, *shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", eu.LINEAR_GEGLU, ids=_name)
def test_ragged_k_linear_geglu(gpu, dtype, shape):
    """The GEGLU instantiation: gate rows at `ncol + half * Ng`, value / gate n-tiles paired inside a wave."""
    _check_linear(gpu, dtype, *shape, geglu=True, group="linear-geglu")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("epi", ["none", "bias", "bias+silu", "bias+residual", "3d"])
def test_ragged_k_linear_epilogues(gpu, dtype, epi):
    M, K, N = 70, 72, 200
    _check_linear(gpu, dtype, M, K, N, bias=epi != "none", silu=epi == "bias+silu", residual=epi == "bias+residual",
                  shape3d=(2, 35) if epi == "3d" else None, group="linear-epilogues")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_ragged_k_linear_statistics_requests(gpu, dtype):
    """The register-staged kernel emits no partials: LayerNorm row statistics are refused loudly, GroupNorm column statistics
    come back as None with the plain launch's bits."""
    M, K, N = 70, 72, 200
    x, w, b = _linear_operands(M, K, N)
    xg, wg, bg = _dev(x.view(2, 35, K), gpu, dtype), _dev(w, gpu, dtype), _dev(b, gpu, dtype)
    plain = ops.linear(xg, wg, bg)
    with pytest.raises(ops.BackendError, match="row statistics"):
        ops.linear(xg, wg, bg, emit_stats=True)
    out, stats = ops.linear(xg, wg, bg, emit_colstats=True)
    assert stats is None
    assert torch.equal(out, plain)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [(70, 72, 200), (2000, 72, 1912)], ids=_name)
def test_ragged_k_linear_stays_inside_its_output(gpu, dtype, shape):
    M, K, N = shape
    x, w, b = _linear_operands(M, K, N)
    xg, wg, bg = _dev(x, gpu, dtype, row_gap=eu.ROW_GAP), _dev(w, gpu, dtype), _dev(b, gpu, dtype)
    out, buf = eu.guarded((M, N), dtype, gpu)
    eu.linear_into(out, xg, wg, bg)
    eu.assert_margins_intact(buf, f"linear {shape}")
    assert torch.isfinite(out.float()).all(), "an output element was never stored (or a poisoned read leaked)"
    assert torch.equal(out, ops.linear(xg, wg, bg))


# ================================================================================================ convs
def _conv_operands(cfg):
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    return (eu.normal(f"e.cx{Cin}.{H}.{W}", (N, Cin, H, W)), eu.normal(f"e.cw{Cout}.{Cin}.{k}", (Cout, Cin, k, k), (Cin * k * k) ** -0.5),
            eu.normal(f"e.cb{Cout}", (Cout,)))


def _check_conv(gpu, dtype, cfg, group, gate=True):
    """Plain (+bias) and with row bias + residual; per-element gate in every type (gate=False: the suite's assert_close)."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    x, w, b = _conv_operands(cfg)
    xg, wg, bg = _dev(x, gpu, dtype, cl=True), _dev(w, gpu, dtype, cl=True), _dev(b, gpu, dtype)
    ref, mag = eu.conv_ref64(x, w, b, dtype, stride, pad, ups)
    rb, res = eu.normal(f"e.crb{Cout}", (N, Cout)), eu.normal(f"e.cres{Cout}.{H}", tuple(ref.shape))
    ref2, mag2 = eu.conv_ref64(x, w, b, dtype, stride, pad, ups, rowbias=rb, residual=res)
    out = ops.conv2d(xg, wg, bg, stride, pad, upsample2x=ups)
    out2 = ops.conv2d(xg, wg, bg, stride, pad, upsample2x=ups, rowbias=_dev(rb, gpu, dtype), residual=_dev(res, gpu, dtype, cl=True))
    for o, rf, mg, what in ((out, ref, mag, f"conv {cfg}"), (out2, ref2, mag2, f"conv {cfg}+rowbias+residual")):
        assert o.is_contiguous(memory_format=CL)
        assert torch.isfinite(o.float()).all(), f"{what}: non-finite output"
        if gate:
            _report(group, dtype, what, eu.assert_elementwise(o, rf, mg, k * k * Cin, dtype, what))
        else:
            assert_close(o, rf.float(), dtype, what)
    return xg, wg, bg


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cfg", eu.THIN_CONVS, ids=_name)
def test_thin_conv(gpu, dtype, cfg):
    """conv_thin_kernel beyond SDXL's conv_in: the channel-by-channel loader (1x1 with 8..48 channels, 3x3 with 3 / 6 / 7), the
    unrolled Cin = 4 branch at stride 2 and with upsampling, row bias and residual.  (fp32 with Cin = 32 is a whole split
    segment and takes the implicit GEMM.)"""
    _check_conv(gpu, dtype, cfg, "thin-conv")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_thin_conv_stays_inside_its_output(gpu, dtype):
    cfg = (1, 8, 9, 7, 32, 1, 1, 0, False)                  # 63 pixels: an M tail inside a 256-pixel block
    x, w, b = _conv_operands(cfg)
    xg, wg, bg = _dev(x, gpu, dtype, cl=True), _dev(w, gpu, dtype, cl=True), _dev(b, gpu, dtype)
    out, buf = eu.guarded((1, 32, 9, 7), dtype, gpu, channels_last=True)
    eu.conv2d_into(out, xg, wg, bg, 1, 0)
    eu.assert_margins_intact(buf, f"conv {cfg}")
    assert torch.isfinite(out.float()).all()
    assert torch.equal(out, ops.conv2d(xg, wg, bg, 1, 0))


def _check_taps(gpu, dtype, cfg):
    """A single 1.0 input pixel reproduces the weight taps at the right output pixels, exactly: weights are multiples of 1/8
    below 2, so the (at most four, with upsampling) taps that meet in one output sum without rounding in every type."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    g = torch.Generator().manual_seed(11)
    w = torch.randint(-15, 16, (Cout, Cin, k, k), generator=g).float() / 8
    wg = _dev(w, gpu, dtype, cl=True)
    for (n, c, y, xx) in {(0, 0, 0, 0), (N - 1, Cin - 1, H - 1, W - 1), (0, Cin // 2, H // 2, W // 3)}:
        x = torch.zeros(N, Cin, H, W)
        x[n, c, y, xx] = 1.0
        xd = F.interpolate(x.double(), scale_factor=2.0, mode="nearest") if ups else x.double()
        ref = F.conv2d(xd, w.double(), None, stride=stride, padding=pad)
        out = ops.conv2d(_dev(x, gpu, dtype, cl=True), wg, None, stride, pad, upsample2x=ups)
        assert torch.equal(out.double().cpu(), ref), f"conv {cfg}: the taps of input pixel {(n, c, y, xx)} land at the wrong outputs"


_HALO = [(d, (n, c, h, w, co, 3, 1, 1, False)) for d in DTYPES for (n, c, h, w, co) in eu.HALO_CONVS if not (d == torch.float32 and w == 16)] + \
        [(d, (n, c, h, w, co, 3, 1, 1, True)) for d in DTYPES for (n, c, h, w, co) in eu.HALO_CONVS_UPS]


@pytest.mark.parametrize("dtype,cfg", _HALO, ids=_name)
def test_halo_conv_edges(gpu, dtype, cfg):
    """The halo conv away from square images: H = 1 (both halo rows are padding), H = 3, a tile that is a whole image (two
    images), 24 x 32 with a ragged channel tile, 16-pixel rows, and the upsampling form from Hin = 2 and 1."""
    _check_conv(gpu, dtype, cfg, "halo-conv", gate=True)
    _check_taps(gpu, dtype, cfg)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("cfg", eu.IGEMM_CONVS, ids=_name)
def test_implicit_gemm_conv_edges(gpu, dtype, cfg):
    """3x3 without padding, 1x1 at stride 2, 3x3 with upsampling at odd sizes."""
    _check_conv(gpu, dtype, cfg, "igemm-conv", gate=True)
    _check_taps(gpu, dtype, cfg)


# ================================================================================================ norms
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", [(1, 96, 5, 7, 32), (2, 32, 3, 3, 32), (1, 64, 4, 4, 1), (1, 40, 1, 1, 8), (1, 8, 33, 31, 2)], ids=_name)
def test_group_norm_edges(gpu, dtype, nhwc, shape):
    """Three channels per group (a 16-byte vector straddles three groups), G == C, G == 1, one pixel, two wide groups."""
    N, C, H, W, G = shape
    x = eu.normal(f"e.gn{C}.{H}", (N, C, H, W)) * 1.5 + 0.7
    w, b = eu.normal(f"e.gnw{C}", (C,)) * 0.2 + 1.0, eu.normal(f"e.gnb{C}", (C,)) * 0.2
    ref = F.group_norm(eu.r64(x, dtype), G, eu.r64(w, dtype), eu.r64(b, dtype), 1e-5)
    xg, wg, bg = _dev(x, gpu, dtype, cl=nhwc), _dev(w, gpu, dtype), _dev(b, gpu, dtype)
    for silu in (False, True):
        out, buf = eu.guarded((N, C, H, W), dtype, gpu, channels_last=nhwc)
        eu.group_norm_into(out, xg, G, wg, bg, 1e-5, silu, nhwc)
        eu.assert_margins_intact(buf, f"group_norm {shape}")
        assert_close(out, (F.silu(ref) if silu else ref).float(), dtype, f"group_norm {shape} silu={silu}")


# (vectors per thread: 64 threads a row, 4 fp32 / 8 16-bit values a vector - 1432 and 1720 are <6> and <7> in fp32, 2864 and 3440 in 16 bits)
_LN = [(d, s) for d in DTYPES for s in [(5, 1432), (6, 1720), (7, 4096), (1, 8)] if not (d == torch.float32 and s[1] == 4096)] + \
      [(d, s) for d in HALF_DTYPES for s in [(5, 2864), (6, 3440)]]


@pytest.mark.parametrize("dtype,shape", _LN, ids=_name)
def test_layer_norm_edges(gpu, dtype, shape):
    """ln_kernel<T, 6>, <T, 7>, the 16-bit <8> (C = 4096) and a single vector per row."""
    rows, C = shape
    x = eu.normal(f"e.ln{C}", (rows, C)) * 2 - 0.5
    w, b = eu.normal(f"e.lnw{C}", (C,)) * 0.2 + 1.0, eu.normal(f"e.lnb{C}", (C,)) * 0.2
    ref = F.layer_norm(eu.r64(x, dtype), (C,), eu.r64(w, dtype), eu.r64(b, dtype), 1e-5)
    out, buf = eu.guarded((rows, C), dtype, gpu)
    eu.layer_norm_into(out, _dev(x, gpu, dtype), _dev(w, gpu, dtype), _dev(b, gpu, dtype), 1e-5)
    eu.assert_margins_intact(buf, f"layer_norm {shape}")
    assert_close(out, ref.float(), dtype, f"layer_norm {shape}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_geglu_small_strided_halves(gpu, dtype):
    rows, Fh = 3, 8
    xp = eu.normal("e.geglu", (rows, 2 * Fh)) * 2
    xg = _dev(xp, gpu, dtype, row_gap=eu.ROW_GAP)
    xd = eu.r64(xp, dtype)
    out, buf = eu.guarded((rows, Fh), dtype, gpu)
    eu.geglu_into(out, xg[:, :Fh], xg[:, Fh:])
    eu.assert_margins_intact(buf, "geglu (3, 8)")
    assert_close(out, (xd[:, :Fh] * eu.gelu64(xd[:, Fh:])).float(), dtype, "geglu (3, 8)")


# ================================================================================================ attention
def _attention64(q, k, v, H, scale):
    B, T, C = q.shape
    D = C // H
    qh, kh, vh = (t.view(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, T, C)


@pytest.mark.parametrize("dtype", HALF_DTYPES, ids=_name)
@pytest.mark.parametrize("B,T,S,H,D", [(1, 65, 77, 1, 64), (1, 97, 257, 1, 64), (1, 33, 100, 2, 32)],
                         ids=["attn16v2", "attn32i-three-waves", "attn_anyd"])
def test_attention_stays_inside_its_output(gpu, dtype, B, T, S, H, D):
    """One case per attention kernel with a ragged last query block and a ragged last key tile: the output sits between guard
    margins, and K / V are followed (and their rows separated) by NaN, so key rows read beyond S - 1 must not reach a result."""
    C = H * D
    q, k, v = eu.normal(f"e.q{T}", (B, T, C)), eu.normal(f"e.k{S}", (B, S, C)), eu.normal(f"e.v{S}", (B, S, C))
    qg, kg, vg = (_dev(t, gpu, dtype, row_gap=eu.ROW_GAP) for t in (q, k, v))
    out, buf = eu.guarded((B, T, C), dtype, gpu)
    eu.attention_into(out, qg, kg, vg, H, D ** -0.5)
    eu.assert_margins_intact(buf, f"attention {(B, T, S, H, D)}")
    assert torch.isfinite(out.float()).all(), "attention: non-finite output (a key / value row beyond S - 1 reached a result, or a row was never stored)"
    ref = _attention64(eu.r64(q, dtype), eu.r64(k, dtype), eu.r64(v, dtype), H, D ** -0.5)
    assert_close(out, ref.float(), dtype, f"attention {(B, T, S, H, D)}")
    assert torch.equal(out, ops.attention(qg, kg, vg, H, D ** -0.5))
