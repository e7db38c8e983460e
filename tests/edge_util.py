"""Helpers of the edge tests (tests/test_edge_gate_host.py, tests/test_edges_gpu.py): a per-element float64 gate with a derived
budget, NaN-poisoned operands, guarded outputs, and C-ABI callers that write into an output the test owns."""
import math

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------ the gate
# Every constant of the budget, and where it comes from:
#  U_OUT       unit roundoff of the stored type (half the spacing of neighbouring values, relative): 8 / 11 / 24 significand
#              bits.  Elem<T>::from_f is a plain conversion, so a store rounds to nearest: one error of at most U_OUT * |exact|.
#  U_ACC       unit roundoff of the fp32 accumulator every kernel sums in.
#  ACC_FACTOR  the textbook worst case of an n-term fp32 sum is n * U_ACC * sum|terms| when every add rounds to nearest; the
#              adds inside an MFMA need not (they may truncate: twice the error per add), hence 2.
#  EPI_OPS     the fp32 operations of the longest epilogue behind the sum (bias, row bias, residual, the two of a SiLU / the
#              product of a GEGLU, dequantisation-free paths have fewer): each adds at most U_ACC * (magnitude so far).
#  ACT_SLOPE   SiLU and GELU have |f'| <= 1.13 (SiLU 1.0998 at x = 2.4, GELU 1.129 at x = 1.41): an error in the
#              pre-activation grows by at most that.
# Products of two bf16 / fp16 values are exact in fp32 (16 or 22 significand bits), so the sum is the only inexact step in
# front of the epilogue; an fp32 x fp32 product rounds once more per term, which the factor 2 also covers (measured on the
# CPU emulation: under 0.15 of the budget).
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
U_ACC = 2.0 ** -24
ACC_FACTOR = 2.0
EPI_OPS = 8
ACT_SLOPE = 1.13
# Absolute error of the device activations themselves against the exact function, for arguments in [-ACT_RANGE, ACT_RANGE]:
#  GELU_EXACT_ABS_ERR  csrc/common.h states 6.8e-7 for gelu_erf_f (the fp32 kernels);
#  GELU_FAST_ABS_ERR   gelu_erf_fast_f (Abramowitz & Stegun 7.1.26, the 16-bit kernels): its float32 restatement measures 4.7e-7 (bounded at 5.0e-7)
#                      (tests/test_edge_gate_host.py::test_activation_error_constants); the device's v_rcp_f32 and v_exp_f32 are
#                      good to one ulp where the restatement's division and exp2 round correctly - one ulp of t or e moves the
#                      result by at most 0.5 * 8 * 2^-23 = 4.8e-7 each at |x| = 8, so 5.0e-7 + 2 * 4.8e-7 = 1.46e-6, rounded up;
#  SILU_ABS_ERR        x / (1 + expf(-x)): restatement 7.0e-7 (bounded at 7.5e-7); expf on the device is good to 2 ulp, which moves the
#                      quotient by at most 2 * 2^-23 * |silu| <= 1.9e-6 at |x| = 8: 2.66e-6, rounded up.
ACT_RANGE = 8.0
GELU_EXACT_ABS_ERR = 6.8e-7
GELU_FAST_ABS_ERR = 1.5e-6
SILU_ABS_ERR = 2.7e-6


def gelu_abs_err(dtype) -> float:
    return GELU_EXACT_ABS_ERR if dtype == torch.float32 else GELU_FAST_ABS_ERR


def acc_bound(n_terms: int, mag64: torch.Tensor) -> torch.Tensor:
    """Worst-case error of an fp32 sum of n_terms exact products and the epilogue behind it, per element."""
    return ACC_FACTOR * (n_terms + EPI_OPS) * U_ACC * mag64


def budget(ref64, mag64, n_terms, dtype, extra64=None):
    b = U_OUT[dtype] * ref64.abs() + acc_bound(n_terms, mag64)
    return b if extra64 is None else b + extra64


def gate_ratio(out, ref64, mag64, n_terms, dtype, extra64=None):
    """(worst |out - ref| / budget, flat index of that element)."""
    o = out.detach().double().cpu()
    err = (o - ref64).abs()
    ratio = err / budget(ref64, mag64, n_terms, dtype, extra64).clamp_min(1e-300)
    ratio = torch.where(torch.isfinite(o), ratio, torch.full_like(ratio, math.inf))
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), i


def assert_elementwise(out, ref64, mag64, n_terms, dtype, what, extra64=None):
    """Every element: |out - ref64| <= U_OUT * |ref64| + 2 * (n_terms + 8) * 2^-24 * mag64 (+ extra64, the activation's own
    absolute error where there is one).  ref64: the operation in float64 on the values the kernel sees; mag64: the same on
    absolute values.  Returns the worst ratio to the budget (tests print it)."""
    assert tuple(out.shape) == tuple(ref64.shape), f"{what}: shape {tuple(out.shape)} vs {tuple(ref64.shape)}"
    ref64, mag64 = ref64.contiguous(), mag64.contiguous()
    o = out.detach().double().cpu().contiguous()
    assert torch.isfinite(o).all(), f"{what}: non-finite output ({int((~torch.isfinite(o)).sum())} elements, first at " \
                                    f"{tuple(int(v) for v in (~torch.isfinite(o)).nonzero()[0])})"
    worst, i = gate_ratio(o, ref64, mag64, n_terms, dtype, extra64)
    if worst > 1.0:
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), o.shape))
        bad = int(((o - ref64).abs() > budget(ref64, mag64, n_terms, dtype, extra64)).sum())
        raise AssertionError(f"{what}: element {idx} = {float(o.reshape(-1)[i])!r}, float64 reference {float(ref64.reshape(-1)[i])!r}: "
                             f"{worst:.3g} x its budget ({bad} of {o.numel()} elements over theirs)")
    return worst


def r64(t: torch.Tensor, dtype) -> torch.Tensor:
    """The value the kernel sees (rounded to dtype), in float64."""
    return t.to(dtype).double()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * (0.5 ** 0.5)))


def silu64(x):
    return x / (1.0 + torch.exp(-x))


def linear_ref64(x, w, bias, dtype, *, silu=False, geglu=False, residual=None):
    """(ref64, mag64, extra64) of ops.linear's epilogue order: +bias, SiLU or GEGLU, +residual - float64 on the rounded operands."""
    xd, wd = r64(x, dtype), r64(w, dtype)
    K = xd.shape[-1]
    pre = xd @ wd.T
    mag = xd.abs() @ wd.abs().T
    if bias is not None:
        bd = r64(bias, dtype)
        pre, mag = pre + bd, mag + bd.abs()
    extra = None
    if geglu:
        Fh = pre.shape[-1] // 2
        v, g, mv, mg = pre[..., :Fh], pre[..., Fh:], mag[..., :Fh], mag[..., Fh:]
        assert float(g.abs().max()) < ACT_RANGE
        # out = v * gelu(g): the value's error times |gelu(g)| (as the kernel has it: off by its own error and the gate's), the
        # gate's error through the slope times |v|; gelu's own error times |v|
        ge = gelu_abs_err(dtype)
        ref = v * gelu64(g)
        mag = (gelu64(g).abs() + ge + ACT_SLOPE * acc_bound(K, mg)) * mv + ACT_SLOPE * v.abs() * mg
        extra = v.abs() * ge
    elif silu:
        assert float(pre.abs().max()) < ACT_RANGE
        ref, mag = silu64(pre), ACT_SLOPE * mag
        extra = torch.full_like(ref, SILU_ABS_ERR)
    else:
        ref = pre
    if residual is not None:
        rd = r64(residual, dtype)
        ref, mag = ref + rd, mag + rd.abs()
    return ref, mag, extra


def conv_ref64(x, w, bias, dtype, stride, pad, ups, rowbias=None, residual=None):
    """(ref64, mag64) of ops.conv2d: nearest 2x upsampling, conv, +bias, +rowbias per image, +residual."""
    xd, wd = r64(x, dtype), r64(w, dtype)
    if ups:
        xd = F.interpolate(xd, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xd, wd, None, stride=stride, padding=pad)
    mag = F.conv2d(xd.abs(), wd.abs(), None, stride=stride, padding=pad)
    for t in (None if bias is None else r64(bias, dtype)[None, :, None, None],
              None if rowbias is None else r64(rowbias, dtype)[:, :, None, None],
              None if residual is None else r64(residual, dtype)):
        if t is not None:
            ref, mag = ref + t, mag + t.abs()
    return ref, mag


# ------------------------------------------------------------------------------------------------ the cases (shared by the CPU proof and the GPU tests)
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# ragged K (K % 64 != 0 for 16-bit, K % 32 != 0 for fp32): the register-staged gemm_kernel, (M, K, N)
LINEAR_64x64 = [(70, 72, 200), (130, 8, 64), (64, 136, 72), (1, 120, 8)]
LINEAR_64x64_F32 = [(70, 36, 200), (33, 4, 64), (64, 100, 72)]
LINEAR_128x64 = [(1280, 72, 1280)]            # 200 tiles of 128 x 64, 100 of 128 x 128
LINEAR_128x128 = [(2048, 72, 1920), (2000, 72, 1912)]      # 240 tiles; ragged M and N on the large tile
LINEAR_GEGLU = [(100, 72, 40), (70, 136, 104), (1280, 72, 1280),      # 64 x 64, 64 x 64, 128 x 64 (400 tiles over value + gate rows)
                (2048, 72, 1920)]                                    # 128 x 128: 480 tiles


def linear_cases(dtype):
    return LINEAR_64x64 + (LINEAR_64x64_F32 if dtype == torch.float32 else []) + LINEAR_128x64 + LINEAR_128x128


# (N, Cin, H, W, Cout, k, stride, pad, upsample)
THIN_CONVS = [(1, 8, 9, 7, 32, 1, 1, 0, False), (2, 32, 16, 16, 64, 1, 1, 0, False), (1, 48, 5, 5, 16, 1, 2, 0, False),
              (1, 3, 9, 7, 32, 3, 1, 1, False), (1, 7, 8, 8, 16, 3, 2, 1, False), (1, 6, 5, 7, 48, 3, 1, 1, True),
              # the unrolled Cin = 4 branch at stride 2 and with upsampling
              (1, 4, 9, 7, 320, 3, 2, 1, False), (1, 4, 5, 7, 32, 3, 1, 1, True)]
# (N, Cin, H, W, Cout): 3x3, stride 1, pad 1
HALO_CONVS = [(1, 64, 1, 128, 64), (1, 64, 3, 128, 160), (2, 64, 4, 64, 64), (1, 64, 24, 32, 72), (1, 64, 32, 16, 64)]
HALO_CONVS_UPS = [(1, 64, 2, 32, 64), (1, 64, 1, 64, 160)]
IGEMM_CONVS = [(1, 64, 9, 7, 64, 3, 1, 0, False), (1, 64, 9, 7, 64, 1, 2, 0, False), (1, 64, 5, 7, 64, 3, 1, 1, True)]


def normal(name: str, shape, scale: float = 1.0) -> torch.Tensor:
    """Seeded N(0, scale^2) values (CPU, fp32); the name picks the stream."""
    g = torch.Generator().manual_seed(int.from_bytes(name.encode(), "little") % (2 ** 63 - 1))
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ poisoned operands, guarded outputs
PAD = 64          # elements on each side: a multiple of 8, so the view keeps the buffer's 16-byte alignment in every dtype
ROW_GAP = 8       # NaN elements between the rows of a 2-D / 3-D activation (16 bytes in 16-bit types, 32 in fp32)


def poisoned(t: torch.Tensor, pad: int = PAD, row_gap: int = 0) -> torch.Tensor:
    """`t`'s values as a view inside a larger NaN-filled buffer: a read before the tensor, behind it or (row_gap > 0: rows of the
    last dimension at stride shape[-1] + row_gap) between its rows returns NaN, and a NaN that leaks into a result shows.
    Memory order is t's own (contiguous or channels_last); weights take row_gap = 0 and stay contiguous inside the buffer."""
    assert pad % 8 == 0 and row_gap % 8 == 0
    if row_gap:
        assert t.dim() in (2, 3) and t.is_contiguous()
        K = t.shape[-1]
        rows = t.numel() // K
        buf = torch.full((2 * pad + rows * (K + row_gap),), math.nan, dtype=t.dtype, device=t.device)
        v = buf[pad:pad + rows * (K + row_gap)].view(rows, K + row_gap)[:, :K]
        v.copy_(t.reshape(rows, K))
        if t.dim() == 3:
            v = v.as_strided(t.shape, (t.shape[1] * (K + row_gap), K + row_gap, 1), v.storage_offset())
        return v
    buf = torch.full((2 * pad + t.numel(),), math.nan, dtype=t.dtype, device=t.device)
    v = buf[pad:pad + t.numel()].as_strided(t.shape, t.stride())
    assert t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)
    v.copy_(t)
    return v


def guarded(shape, dtype, device, fill=math.nan, pad: int = PAD, channels_last: bool = False):
    """(tensor, buffer): a dense tensor of `shape` whose memory sits inside a larger buffer; tensor and margins hold `fill`.  A
    store out of bounds shows in the margins (assert_margins_intact), an element never stored keeps `fill`."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * pad,), fill, dtype=dtype, device=device)
    t = buf[pad:pad + n]
    if channels_last:
        b, c, h, w = shape
        t = t.view(b, h, w, c).permute(0, 3, 1, 2)
    else:
        t = t.view(shape)
    return t, buf


def assert_margins_intact(buf: torch.Tensor, what: str, pad: int = PAD) -> None:
    lo, hi = buf[:pad], buf[-pad:]
    ok = (torch.isnan(lo).all() and torch.isnan(hi).all()) if bool(torch.isnan(buf[0])) else \
        (bool(torch.all(lo == buf[0])) and bool(torch.all(hi == buf[0])))
    assert ok, f"{what}: a store landed outside the output (guard margins changed)"


# ------------------------------------------------------------------------------------------------ C-ABI callers: the output is the caller's
# (ops.* allocates its own output; the argument plumbing below is the matching ops.* function's)
def _ops():
    from stabletriton_amd import _C, ops
    return _C, ops


def linear_into(out, x, w, bias=None, *, silu=False, geglu=False, residual=None):
    """st_linear of (M, K) x (row stride free) and contiguous (N or 2N, K) w into the dense (M, N) `out`."""
    _C, ops = _ops()
    x2, M, lda = ops._rows2d(x)
    K = x.shape[-1]
    N = w.shape[0] // 2 if geglu else w.shape[0]
    assert w.is_contiguous() and out.is_contiguous() and out.numel() == M * N and out.dtype == x.dtype == w.dtype
    assert not ops.split_usable(x.dtype, K), "the split-operand path keeps its images in ops.linear"
    epi = (_C.EPI_BIAS if bias is not None else 0) | (_C.EPI_SILU if silu else 0) | (_C.EPI_GEGLU if geglu else 0)
    ldr = 0
    if residual is not None:
        residual, _, ldr = ops._rows2d(residual)
        epi |= _C.EPI_RESIDUAL
    gws = ops._gemm_workspace(x.device)
    _C.check(_C.load().st_linear(x2.data_ptr(), w.data_ptr(), ops._ptr(bias), ops._ptr(residual), None, out.data_ptr(), M, N, K,
                                 lda, N, ldr, 0, epi, _C.dtype_code(x.dtype), gws.data_ptr(), gws.numel(), None, 0, None, None, 0, None,
                                 None, 0, _C.stream_ptr()), "linear")
    return out


def conv2d_into(out, x, w, bias, stride, padding, *, upsample2x=False, rowbias=None, residual=None):
    """st_conv2d of channels_last x and w into the channels_last `out` (N, Cout, Ho, Wo)."""
    _C, ops = _ops()
    cl = torch.channels_last
    assert x.is_contiguous(memory_format=cl) and w.is_contiguous(memory_format=cl) and out.is_contiguous(memory_format=cl)
    N, Cin, H, W = x.shape
    Cout, _, R, S = w.shape
    He, We = (2 * H, 2 * W) if upsample2x else (H, W)
    assert tuple(out.shape) == (N, Cout, (He + 2 * padding - R) // stride + 1, (We + 2 * padding - S) // stride + 1)
    epi = (_C.EPI_BIAS if bias is not None else 0) | (_C.EPI_ROWBIAS if rowbias is not None else 0) | \
          (_C.EPI_RESIDUAL if residual is not None else 0)
    assert residual is None or residual.is_contiguous(memory_format=cl)
    code, xs, ws = _C.dtype_code(x.dtype), x, w
    if ops.split_usable(x.dtype, Cin):          # strict mode: split images of the pixels and the taps, as ops.conv2d
        xs = ops._split_of(x, N * H * W, Cin, Cin)
        ws, code = ops._split_weight(w, ops._conv_weight_rows)[0], _C.ST_F32S
    gws = ops._gemm_workspace(x.device)
    _C.check(_C.load().st_conv2d(xs.data_ptr(), ws.data_ptr(), ops._ptr(bias), ops._ptr(residual), ops._ptr(rowbias), out.data_ptr(),
                                 N, H, W, Cin, Cout, R, S, stride, padding, int(upsample2x), epi, code, gws.data_ptr(), gws.numel(),
                                 None, 0, None, None, 0, _C.stream_ptr()), "conv2d")
    return out


def attention_into(out, q, k, v, num_heads, scale):
    """st_attention of (B, T, H*D) q and (B, S, H*D) k / v (token stride free, dense batches) into the dense `out`."""
    _C, ops = _ops()
    B, T, Cc = q.shape
    S = k.shape[1]
    for t in (q, k, v):
        assert t.stride(2) == 1 and t.stride(0) == t.stride(1) * t.shape[1]
    assert out.is_contiguous() and tuple(out.shape) == (B, T, Cc)
    _C.check(_C.load().st_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, T, S, num_heads, Cc // num_heads,
                                    q.stride(1), k.stride(1), v.stride(1), Cc, float(scale), _C.dtype_code(q.dtype), _C.stream_ptr()),
             "attention")
    return out


def group_norm_into(out, x, groups, weight, bias, eps, silu, nhwc: bool):
    """st_group_norm into `out` (x's memory order: NCHW-contiguous, or channels_last with nhwc)."""
    _C, ops = _ops()
    lib = _C.load()
    N, Cc = x.shape[0], x.shape[1]
    HW = x.numel() // (N * Cc)
    assert x.is_contiguous(memory_format=torch.channels_last) if nhwc else x.is_contiguous()
    assert out.shape == x.shape and (out.is_contiguous(memory_format=torch.channels_last) if nhwc else out.is_contiguous())
    ws = torch.empty(lib.st_group_norm_workspace_bytes(N, Cc, HW, groups), dtype=torch.uint8, device=x.device)
    _C.check(lib.st_group_norm(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), N, Cc, HW, groups, float(eps),
                               int(bool(silu)), _C.ST_NHWC if nhwc else _C.ST_NCHW, _C.dtype_code(x.dtype), ws.data_ptr(),
                               _C.stream_ptr()), "group_norm")
    return out


def layer_norm_into(out, x, weight, bias, eps):
    _C, ops = _ops()
    Cc = x.shape[-1]
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape
    _C.check(_C.load().st_layer_norm(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), x.numel() // Cc, Cc, float(eps),
                                     _C.dtype_code(x.dtype), _C.stream_ptr()), "layer_norm")
    return out


def geglu_into(out, state, gate):
    """st_geglu of two (rows, F) operands with free row strides (the halves of one projection) into the dense `out`."""
    _C, ops = _ops()
    rows, Fh = state.shape
    assert state.stride(1) == 1 and gate.stride(1) == 1 and out.is_contiguous() and tuple(out.shape) == (rows, Fh)
    _C.check(_C.load().st_geglu(state.data_ptr(), gate.data_ptr(), out.data_ptr(), rows, Fh, state.stride(0), gate.stride(0), Fh,
                                _C.dtype_code(state.dtype), _C.stream_ptr()), "geglu")
    return out
