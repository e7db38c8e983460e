"""Helpers of the edge tests (tests/test_edge_gate_host.py, tests/test_edges_gpu.py, tests/test_dma_gate_host.py,
tests/test_dma_edges_gpu.py, tests/test_conv_gate_host.py, tests/test_conv_edges_gpu.py, tests/test_fp8_gate_host.py,
tests/test_fp8_edges_gpu.py): a per-element float64 gate with a derived
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
#              An in-launch K split (gemm_dma.h: splitk_combine) sums its sk fp32 slabs in slice order: sk - 1 more fp32 adds
#              of partial sums of the same terms, at most 7 for sk <= 8 - inside these 8 (the split launches carry bias and
#              residual only: two operations of their own; a slice's sum is shorter by what the other slices hold).
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


def _epilogue64(pre, mag, K, dtype, *, silu=False, geglu=False, residual=None):
    """SiLU or GEGLU, then +residual, on a pre-activation `pre` whose error is bounded by acc_bound(K, mag)."""
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


def linear_ref64(x, w, bias, dtype, *, silu=False, geglu=False, residual=None, split_operands=False, products=None, K=None):
    """(ref64, mag64, extra64) of ops.linear's epilogue order: +bias, SiLU or GEGLU, +residual - float64 on the rounded operands.
    split_operands: the fp32 operands meet the matrix pipe as split images (as_magnitude(split_term(...)) joins mag64);
    products: (x @ w.T, |x| @ |w|.T) in float64 where the caller keeps them (tests share them between epilogues; with K given,
    x and w are not needed at all: the fp8 gate's products are those of bytes and scales)."""
    K = x.shape[-1] if K is None else K
    if products is None:
        xd, wd = r64(x, dtype), r64(w, dtype)
        products = (xd @ wd.T, xd.abs() @ wd.abs().T)
    pre, mag = products
    if split_operands:
        mag = mag + as_magnitude(split_term(mag), K)
    if bias is not None:
        bd = r64(bias, dtype)
        pre, mag = pre + bd, mag + bd.abs()
    return _epilogue64(pre, mag, K, dtype, silu=silu, geglu=geglu, residual=residual)


# ------------------------------------------------------------------------------------------------ the LDS-DMA GEMM's own terms
# (tests/test_dma_gate_host.py measures every constant below on the fp32 emulation of the kernel's arithmetic; the GPU tests
#  of tests/test_dma_edges_gpu.py use them as they stand)
#
# Split fp32 operands (csrc/split.h, Mma<fsp>): a value x meets the matrix pipe as hi + lo * 2^-11, hi = f16(x),
# lo = f16((x - hi) * 2^11).  |x - hi| <= 2^-11 |x| is exact in fp32, and its half keeps 11 bits of it: the image is off by
# at most 2^-22 |x| (normal halves); the kernel multiplies hi.hi + (hi.lo + lo.hi) * 2^-11 and drops lo.lo <= 2^-22 |x w|.
# So a product is off by at most 3 * 2^-22 |x w|.  The suite states the image's accuracy as "22 significant bits", 2^-21 per
# operand (tests/test_split_gpu.py, tests/test_ops_gpu.py::test_ln_linear): SPLIT_OPERAND_U, two operands a product,
# 2 * 2^-21 = 4 * 2^-22 - which covers the dropped lo.lo as well.  The float64 reference multiplies the fp32 values themselves.
SPLIT_OPERAND_U = 2.0 ** -21


def split_term(mag_product64):
    """Error of a sum of products of split fp32 operands that comes from the 22-bit images: 2 * 2^-21 * sum |x| |w|."""
    return 2.0 * SPLIT_OPERAND_U * mag_product64


def as_magnitude(err64, n_terms):
    """An absolute error bound as the magnitude that gives it in acc_bound(n_terms, .): errors in front of an activation
    travel through the epilogue with the accumulation error this way."""
    return err64 / (ACC_FACTOR * (n_terms + EPI_OPS) * U_ACC)


# LayerNorm folded into the GEMM (gemm_dma.h, gemm_args.h: ln_fold): y = fma(rstd, fma(-mean, c, acc), d) with
#     a1 = sum of the producer's per-tile row sums, a2 = the same of the squares (fp32, fixed order: LnRowSum),
#     mean = a1 / K,   rstd = rsqrtf(max(a2 / K - mean * mean, 0) + eps).
# With S = sum_k x w' exact, mu / rho the exact mean / rstd of the row, m1 = sum |x| / K and q = sum x^2 / K:
#  d_mean  a1 is a K-term fp32 sum in blocks (<= BN columns inside the producer's tile, then the tiles): its worst case is
#          K U_ACC sum|x|, a bound no data of the tests comes near (rounding errors of both signs add like sqrt(K)).  The
#          constants are therefore MEASURED on the emulation, in units of U_ACC * m1, and doubled at most (the device
#          adds in another order): LN_MEAN_ULPS.  The division by K rounds once more: inside it.
#  d_rstd  var = a2 / K - mean^2 cancels: both terms carry their absolute errors into a difference that is q / var times
#          smaller.  d_var <= LN_VAR_ULPS * U_ACC * q + 2 |mu| d_mean (a2 / K measured like a1 / K, plus the two roundings of
#          mean * mean and the subtraction), and rstd = (var + eps)^-1/2 moves by rho / 2 * d_var / (var + eps); rsqrtf itself
#          is good to 2 ulp = 4 U_ACC on the device (1 ulp in the emulation).
#  the two FMAs round once each: U_ACC (|S - mu c| rho + |y|), two of the EPI_OPS on the magnitude rho (mag_S + |mu c|) + |d|.
# Per element the fold adds   rho |c| d_mean + d_rstd |S - mu c|   to the error of acc (rho * acc_bound(K, mag_S)).
LN_MEAN_ULPS = 2.5        # measured 1.32 (tests/test_dma_gate_host.py::test_emulated_row_statistics prints it): x 2, rounded down
LN_VAR_ULPS = 8.0         # measured 4.03
RSQRT_ULPS = 4.0


def ln_stat_bounds(x64, eps):
    """(mu, rho, d_mean, d_rstd) per row of the float64 activations x64 (rows, K): exact statistics and the bounds above."""
    mu, q, m1 = x64.mean(-1), (x64 * x64).mean(-1), x64.abs().mean(-1)
    var = (q - mu * mu).clamp_min(0.0)
    rho = (var + eps).rsqrt()
    d_mean = LN_MEAN_ULPS * U_ACC * m1
    d_var = LN_VAR_ULPS * U_ACC * q + 2.0 * mu.abs() * d_mean
    d_rstd = rho * (0.5 * d_var / (var + eps) + RSQRT_ULPS * U_ACC)
    return mu, rho, d_mean, d_rstd


def ln_linear_ref64(x, wf, c, d, dtype, eps, *, geglu=False, split_operands=False, products=None):
    """(ref64, mag64, extra64) of ops.ln_linear on the operands the kernel sees: x (rows, K) as stored by its producer, the
    folded weight wf, the fp32 vectors c and d of ops.fold_layer_norm (split operands: c of the weight's image).
    products: (S, |S| term by term) in float64 where the product is not x @ wf.T - the fp8 GEMM takes the row statistics from
    the 16-bit tensor x and multiplies its dequantised e4m3 copy (wf is then unused)."""
    xd = r64(x, dtype)
    K = xd.shape[-1]
    cd, dd = c.double(), d.double()
    mu, rho, d_mean, d_rstd = (t[:, None] for t in ln_stat_bounds(xd, eps))
    if products is None:
        wd = r64(wf, dtype)
        products = (xd @ wd.T, xd.abs() @ wd.abs().T)
    S, magS = products
    if split_operands:
        magS = magS + as_magnitude(split_term(magS), K)
    centred = S - mu * cd
    pre = rho * centred + dd
    mag = rho * (magS + mu.abs() * cd.abs()) + dd.abs()
    mag = mag + as_magnitude(rho * cd.abs() * d_mean + d_rstd * centred.abs(), K)
    return _epilogue64(pre, mag, K, dtype, geglu=geglu)


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


# ---- the LDS-DMA kernel (gemm_dma_kernel: K a whole number of 128-byte K tiles), tests/test_dma_edges_gpu.py ----------------
# (tile gemm_dispatch takes in bf16 / fp16, (M, K, N)); every shape has a partial last M tile and a partial last N tile, N % 8 == 0.
# 64 x 320 wins only where M <= 64 leaves every other tile more than one round of 256 blocks: N > 40960.
DMA_PLAIN = [("64x64", (1, 64, 8)), ("64x64", (70, 64, 200)), ("128x64", (197, 64, 4128)), ("64x128", (259, 64, 4128)),
             ("128x128", (400, 64, 5128)), ("128x80", (450, 64, 3368)), ("128x160", (771, 64, 4648)), ("256x128", (1027, 64, 4488)),
             ("128x320", (1539, 64, 4648)), ("64x320", (33, 64, 40968))]
DMA_GEGLU = [("64x64", (1, 64, 8)), ("64x64", (100, 64, 40)), ("128x64", (71, 64, 4168)), ("64x128", (134, 64, 3088)),
             ("128x128", (197, 64, 4128)), ("128x160", (400, 64, 4128)), ("256x128", (400, 64, 5128)), ("128x320", (771, 64, 4128)),
             ("64x320", (33, 64, 20488))]                       # (BN = 80 is not offered to GEGLU)
# split fp32 operands: no BN = 320, no 256 x 128 - those shapes land on 128 x 128 (64 x 128 for the 64 x 320 one), which the
# 128 x 128 shape has already: left out
DMA_F32_TILES = ("64x64", "128x64", "64x128", "128x128", "128x80", "128x160")
DMA_WIDE_TILES = ("128x160", "128x320", "256x128")
# K tiles against ring stages (four; 256 x 128 three, 128 x 320 two): 2, 3, 4, 5 K tiles - and the single one of the lists above
DMA_RING_K = {2: (128, 192, 256, 320), 4: (64, 96, 128, 160)}       # by element size: a K tile is 64 / 32 values
# K split with slices of unequal length (nk % sk != 0): (sk, tile, shape) in bf16 / fp16 ...
DMA_UNEVEN_SPLITS = [(2, "64x64", (1, 2752, 4488)), (3, "128x64", (71, 4160, 3448)), (3, "64x128", (71, 4160, 4168)),
                     (3, "128x128", (197, 4160, 4248)), (4, "64x64", (1, 1088, 8)), (4, "128x80", (71, 4160, 3408)),
                     (6, "64x64", (1, 2112, 928)), (6, "128x80", (71, 4160, 2248)), (8, "64x64", (1, 2112, 8))]
# ... and what the same shapes take as split fp32 operands (K tiles of 32: nk = 86, 130, 34, 66 - every split uneven again)
DMA_UNEVEN_SPLITS_F32 = [(6, "64x128", (1, 2752, 4488)), (8, "128x128", (71, 4160, 3448)), (4, "128x80", (71, 4160, 4168)),
                         (3, "128x128", (197, 4160, 4248)), (8, "64x64", (1, 1088, 8)), (8, "128x128", (71, 4160, 3408)),
                         (8, "64x64", (1, 2112, 928)), (6, "128x80", (71, 4160, 2248)), (8, "64x64", (1, 2112, 8))]
DMA_LN_K = (128, 640)
# row statistics: the buffer holds 64 N tiles (ops.STATS_MAX_CHUNKS), so the 128 x 64 shape above (65 tiles) and the 64 x 320
# one (129) cannot emit them; 128 x 64 has a shape of its own, 64 x 320 is out of the buffer's reach at any N that selects it
DMA_STATS = [(t, (257, 64, 3272) if t == "128x64" else s) for t, s in DMA_PLAIN if t != "64x320"]
# eight-phase kernel (whole tiles only): the smallest M x N that gemm8p_applies accepts and the model prices under the small
# tiles (which need more than 256 of their largest tiles before they lose), at two and at five K tiles
GEMM8P = [("256x256", (768, 128, 11008)), ("256x256", (768, 320, 11008)), ("256x160", (5632, 128, 1440)), ("256x160", (5632, 320, 1440))]
GEMM8P_F32 = [("256x160", (768, 64, 6880)), ("256x160", (768, 160, 6880))]


def dma_plain(dtype):
    return [(t, s) for t, s in DMA_PLAIN if dtype != torch.float32 or t in DMA_F32_TILES]


def dma_geglu(dtype):
    return [(t, s) for t, s in DMA_GEGLU if dtype != torch.float32 or t in DMA_F32_TILES]


def dma_ring(dtype):
    """The plain shape of every tile at 2, 3, 4 and 5 K tiles."""
    return [(t, (M, k, N)) for t, (M, _, N) in dma_plain(dtype) if M > 1 for k in DMA_RING_K[4 if dtype == torch.float32 else 2]]


def dma_wide(dtype):
    return [(t, s) for t, s in dma_plain(dtype) if t in DMA_WIDE_TILES]


def dma_splits(dtype):
    return DMA_UNEVEN_SPLITS_F32 if dtype == torch.float32 else DMA_UNEVEN_SPLITS


def dma_ln(dtype):
    """(tile, shape, geglu): the plain and the GEGLU shape of every tile at K = 128 and 640."""
    return [(t, (M, k, N), g) for g, lst in ((False, dma_plain(dtype)), (True, dma_geglu(dtype))) for t, (M, _, N) in lst
            if M > 1 for k in DMA_LN_K]


def dma_stats(dtype):
    return [(t, s) for t, s in DMA_STATS if dtype != torch.float32 or t in DMA_F32_TILES]


def gemm8p(dtype):
    return GEMM8P_F32 if dtype == torch.float32 else GEMM8P


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


def dma_operands(M, K, rows):
    """(x, w, bias) of an LDS-DMA case: pre-activations of about unit variance, so that |gate| stays under ACT_RANGE among millions."""
    return normal(f"d.x{M}.{K}", (M, K)), normal(f"d.w{rows}.{K}", (rows, K), K ** -0.5), normal(f"d.b{rows}", (rows,), 0.5)


def dma_ln_operands(M, K, rows):
    """(x, gamma, beta, w, bias) of a LayerNorm-fold case: rows with a non-zero mean (0.4 against a deviation of 1.7)."""
    return (normal(f"d.lx{M}.{K}", (M, K)) * 1.7 + 0.4, normal(f"d.g{K}", (K,), 0.2) + 1.0, normal(f"d.be{K}", (K,), 0.2),
            normal(f"d.lw{rows}.{K}", (rows, K), K ** -0.5), normal(f"d.lb{rows}", (rows,), 0.5))


# ------------------------------------------------------------------------------------------------ poisoned operands, guarded outputs
PAD = 64          # elements on each side: a multiple of 8, so the view keeps the buffer's 16-byte alignment in every dtype
ROW_GAP = 8       # NaN elements between the rows of a 2-D / 3-D activation (16 bytes in 16-bit types, 32 in fp32)
E4M3_NAN = 0x7F   # the poison of uint8 tensors (e4m3 bytes): the NaN of OCP e4m3; a product with it is NaN
ROW_GAP_U8 = 16   # between rows of e4m3 bytes (st_linear_fp8 wants row strides that are multiples of 16)


def _poison(dtype):
    return E4M3_NAN if dtype == torch.uint8 else math.nan


def poisoned(t: torch.Tensor, pad: int = PAD, row_gap: int = 0) -> torch.Tensor:
    """`t`'s values as a view inside a larger NaN-filled buffer (uint8: filled with the e4m3 NaN byte): a read before the tensor, behind it or (row_gap > 0: rows of the
    last dimension at stride shape[-1] + row_gap) between its rows returns NaN, and a NaN that leaks into a result shows.
    Memory order is t's own (contiguous or channels_last); weights take row_gap = 0 and stay contiguous inside the buffer."""
    assert pad % 8 == 0 and row_gap % 8 == 0
    if row_gap:
        assert t.dim() in (2, 3) and t.is_contiguous()
        K = t.shape[-1]
        rows = t.numel() // K
        buf = torch.full((2 * pad + rows * (K + row_gap),), _poison(t.dtype), dtype=t.dtype, device=t.device)
        v = buf[pad:pad + rows * (K + row_gap)].view(rows, K + row_gap)[:, :K]
        v.copy_(t.reshape(rows, K))
        if t.dim() == 3:
            v = v.as_strided(t.shape, (t.shape[1] * (K + row_gap), K + row_gap, 1), v.storage_offset())
        return v
    buf = torch.full((2 * pad + t.numel(),), _poison(t.dtype), dtype=t.dtype, device=t.device)
    v = buf[pad:pad + t.numel()].as_strided(t.shape, t.stride())
    assert t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last)
    v.copy_(t)
    return v


def guarded(shape, dtype, device, fill=None, pad: int = PAD, channels_last: bool = False):
    """(tensor, buffer): a dense tensor of `shape` whose memory sits inside a larger buffer; tensor and margins hold `fill` (NaN;
    uint8: the e4m3 NaN byte).  A store out of bounds shows in the margins (assert_margins_intact), an element never stored keeps
    `fill`."""
    n = math.prod(shape)
    fill = _poison(dtype) if fill is None else fill
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
    code = _C.dtype_code(x.dtype)
    if ops.split_usable(x.dtype, K):            # strict mode: split images of both operands, as ops.linear
        x2, lda, w, code = ops._split_of(x2, M, K, lda), K, ops._split_weight(w)[0], _C.ST_F32S
    epi = (_C.EPI_BIAS if bias is not None else 0) | (_C.EPI_SILU if silu else 0) | (_C.EPI_GEGLU if geglu else 0)
    ldr = 0
    if residual is not None:
        residual, _, ldr = ops._rows2d(residual)
        epi |= _C.EPI_RESIDUAL
    gws = ops._gemm_workspace(x.device)
    _C.check(_C.load().st_linear(x2.data_ptr(), w.data_ptr(), ops._ptr(bias), ops._ptr(residual), None, out.data_ptr(), M, N, K,
                                 lda, N, ldr, 0, epi, code, gws.data_ptr(), gws.numel(), None, 0, None, None, 0, None,
                                 None, 0, _C.stream_ptr()), "linear")
    return out


def _fp8_epilogue(_C, ops, bias, silu, geglu, residual):
    epi = (_C.EPI_BIAS if bias is not None else 0) | (_C.EPI_SILU if silu else 0) | (_C.EPI_GEGLU if geglu else 0)
    ldr = 0
    if residual is not None:
        assert residual.dtype == torch.bfloat16
        residual, _, ldr = ops._rows2d(residual)
        epi |= _C.EPI_RESIDUAL
    return epi, residual, ldr


def linear_fp8_into(out, xq, row_scale, wq, w_scale, bias=None, *, silu=False, geglu=False, residual=None):
    """st_linear_fp8 of e4m3 bytes xq (M, K) (row stride free, a multiple of 16) with one fp32 scale per row and contiguous
    (N or 2N, K) wq with one per weight row into the dense bf16 (M, N) `out`."""
    _C, ops = _ops()
    M, K = xq.shape
    N = wq.shape[0] // 2 if geglu else wq.shape[0]
    assert xq.dtype == wq.dtype == torch.uint8 and xq.stride(1) == 1 and wq.is_contiguous() and wq.shape[1] == K
    assert row_scale.dtype == w_scale.dtype == torch.float32 and row_scale.numel() == M and w_scale.numel() == wq.shape[0]
    assert out.is_contiguous() and out.numel() == M * N and out.dtype == torch.bfloat16 and (bias is None or bias.dtype == torch.bfloat16)
    epi, residual, ldr = _fp8_epilogue(_C, ops, bias, silu, geglu, residual)
    gws = ops._gemm_workspace(wq.device)
    _C.check(_C.load().st_linear_fp8(xq.data_ptr(), row_scale.data_ptr(), wq.data_ptr(), w_scale.data_ptr(), ops._ptr(bias), ops._ptr(residual),
                                     out.data_ptr(), M, N, K, xq.stride(0), N, ldr, epi, gws.data_ptr(), gws.numel(), None, 0, _C.stream_ptr()),
             "linear_fp8")
    return out


def linear_fp8x_into(out, xq, a_scale, wq, w_scale, bias=None, *, geglu=False, residual=None, ln=None, row_stats=None, q8=None,
                     q8_inv_scale=None, q8_amax=None):
    """st_linear_fp8x: activation scale per tensor (a_scale has one entry) or per row (M entries); ln = (RowStats partials
    (M, chunks, 2), c, d, eps) folds a LayerNorm; `out` dense bf16 (M, N) or None (only the copy: the GEGLU form); row_stats:
    an fp32 (M, capacity, 2) buffer for the output's row partials; q8 dense uint8 (M, N) with its inverse scale (one fp32) and
    its amax slots (ops.FP8_AMAX_SLOTS int32).  Returns the number of statistics chunks written per row (0 without row_stats)."""
    import ctypes
    _C, ops = _ops()
    M, K = xq.shape
    N = wq.shape[0] // 2 if geglu else wq.shape[0]
    assert xq.dtype == wq.dtype == torch.uint8 and xq.stride(1) == 1 and wq.is_contiguous() and wq.shape[1] == K
    assert a_scale.dtype == w_scale.dtype == torch.float32 and a_scale.numel() in (1, M) and w_scale.numel() == wq.shape[0]
    assert out is None or (out.is_contiguous() and out.numel() == M * N and out.dtype == torch.bfloat16)
    assert q8 is None or (q8.is_contiguous() and q8.numel() == M * N and q8.dtype == torch.uint8 and q8_inv_scale.dtype == torch.float32
                          and q8_amax.numel() == ops.FP8_AMAX_SLOTS and q8_amax.dtype == torch.int32)
    stride = 1 if (a_scale.numel() == M and M > 1) else 0
    epi, residual, ldr = _fp8_epilogue(_C, ops, bias, False, geglu, residual)
    st_in, chunks_in, c, d, eps = (None, 0, None, None, 0.0) if ln is None else (ln[0], ln[0].shape[1], ln[1], ln[2], ln[3])
    assert st_in is None or (st_in.is_contiguous() and st_in.dtype == c.dtype == d.dtype == torch.float32)
    chunks = ctypes.c_int(0)
    gws = ops._gemm_workspace(wq.device)
    _C.check(_C.load().st_linear_fp8x(xq.data_ptr(), a_scale.data_ptr(), stride, wq.data_ptr(), w_scale.data_ptr(), ops._ptr(bias), ops._ptr(residual),
                                      ops._ptr(out), M, N, K, xq.stride(0), N, ldr, epi, ops._ptr(st_in), chunks_in, ops._ptr(c), ops._ptr(d), float(eps),
                                      ops._ptr(row_stats), 0 if row_stats is None else row_stats.shape[1],
                                      None if row_stats is None else ctypes.byref(chunks), ops._ptr(q8), N, ops._ptr(q8_inv_scale),
                                      ops._ptr(q8_amax), gws.data_ptr(), gws.numel(), None, 0, _C.stream_ptr()), "linear_fp8x")
    return chunks.value


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


def attention_split_into(out, q, k_img, v_img, num_heads, scale):
    """st_attention_split of fp32 (B, T, H*64) q and the split images of K and V ((B*S, H*64) float32-typed tensors of
    ops.split_rows) into the dense `out`."""
    _C, ops = _ops()
    B, T, Cc = q.shape
    S = k_img.shape[0] // B
    assert q.dtype == torch.float32 and q.stride(2) == 1 and q.stride(0) == q.stride(1) * T
    assert k_img.is_contiguous() and v_img.is_contiguous() and k_img.shape == v_img.shape == (B * S, Cc)
    assert out.is_contiguous() and tuple(out.shape) == (B, T, Cc)
    _C.check(_C.load().st_attention_split(q.data_ptr(), k_img.data_ptr(), v_img.data_ptr(), out.data_ptr(), B, T, S, num_heads,
                                          Cc // num_heads, q.stride(1), Cc, Cc, Cc, float(scale), _C.stream_ptr()), "attention_split")
    return out


# ------------------------------------------------------------------------------------------------ attention: reference, budget, cases
# (tests/test_attention_gate_host.py proves the gate on a CPU emulation of the kernels' arithmetic and measures the two
#  constants that cannot be derived; tests/test_attention_edges_gpu.py applies it to every attention kernel)
#
# What the kernels are documented to compute (csrc/attention_core.h, attention.hip, attention_anyd.hip, attention_f32.hip):
#     q' = round_E(fp32(q) * c),  c = fp32(scale) * fp32(log2 e) in fp32   (fp32 tensors: q' = the fp32 product, then split)
#     s_k = q' . k_k (fp32 accumulation, started at -m_ref),   P_k = round_E(2^(s_k - m_ref)),   out = round(sum P_k v_k / sum P_k)
# The reference is that in float64 WITH the documented rounding of q' (it is the design, not an error), a base-2 softmax p, and
# ref = sum p_k v_k, mag = sum p_k |v_k|.  Every error of a P_k that is RELATIVE (P_k = p_k (1 + e_k), |e_k| <= e) enters the
# numerator and - the row sum comes from the same P through the ones block - the denominator alike:
#     out' - ref = sum e_k p_k (v_k - ref) / (1 + sum e_k p_k),     |out' - ref| <= e * sum p_k |v_k - ref|  (/ (1 - e)).
# sum p_k |v_k - ref| is at most mag + |ref| (the plain first-order form) and, by Cauchy-Schwarz, at most the softmax-weighted
# deviation sd = sqrt(sum p_k v_k^2 - ref^2), which one more product gives: W = min(mag + |ref|, sd) is the weight of every
# relative term.  (The lazy maximum keeps P <= 2^ATT_LAG, a shift of the exponent: no relative bound changes.)  The terms:
#  store       U_OUT |ref|                                       one rounding of fp32 -> E at the store
#  P rounding  u_P W, u_P = U_OUT[E]; fp32 tensors: SPLIT_OPERAND_U (P is split in registers: a 22-bit image)
#  scores      an fp32 sum of D exact products from -m_ref: acc_bound(D, smag) with smag = max_k sum_d |q'_d k_kd| + |m| + ATT_LAG
#              (m: the row's true maximum; the reference maximum lags it by at most ATT_LAG; the subtraction of delta when
#              it moves is one of the EPI_OPS).  An absolute error d of a base-2 exponent is a relative error ln 2 * d of P.
#              fp32 tensors: plus the images of q' and K, ATT_SPLIT_MULT * split_term(max_k sum |q' k|), the same way.
#  v_exp_f32   ATT_EXP2_ULPS * 2^-23 W                           (measured, below)
#  O sum       numerator and denominator are fp32 sums of S products each, exact in fp32 for 16-bit operands:
#              acc_bound(S, mag + |ref|) - the existing form 2 (n + 8) 2^-24 on the magnitude of both; its eight extra
#              operations hold the rescales by alpha (each a rounding of O and of the row sum, and alpha's own exp2 error on
#              everything summed so far), 1 / l and the product with it.
#              fp32 tensors: plus the images of P and V in the products, ATT_SPLIT_MULT * split_term(mag + |ref|).
#  subnormal P (fp16) a P under 2^-14 rounds with an ABSOLUTE error of 2^-25, not a relative one.  The row sum is at least 1 in
#              the units of m_ref (the key that set m_ref has P = 1, and a key that moves it again has P = 1 afterwards), so
#              every such key moves the output by at most 2^-25 (|v_k| + |ref|): 2^-25 (sum_k |v_k| + S |ref|).  The lo half
#              of a split P under 2^-14 is off by 2^-36 in the same way (csrc/split.h); bf16 has fp32's exponent range.
ATT_LAG = 6.0
ATT_SUBNORMAL_P = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25, torch.float32: 2.0 ** -36}
# The two constants measured on the CPU emulation against float64 (tests/test_attention_gate_host.py::test_measured_constants
# prints them and holds them to "covers the measured value, at most twice it"), never against GPU output:
#  ATT_EXP2_ULPS    error of the fp32 exp2 at the emulation's own arguments, in ulp (2^-23 relative): measured 0.58; x 2 = 1.16,
#                   rounded down to the 1 ulp the instruction set documents for v_exp_f32
#  ATT_SPLIT_MULT   what the split images of q', K, P and V move an fp32 output by, as a multiple of the worst-case terms
#                   above (emulation with split operands against the same emulation on the fp32 values): measured 0.454 x 2, rounded down
ATT_EXP2_ULPS = 1.0
ATT_SPLIT_MULT = 0.9
ATT_SPOT_GAINS = (0.35, 1.0, 2.0)
ATT_SPOT_MIN_P = 0.05


def attention_prescale(q, scale, dtype):
    """q' = round_E(fp32(q) * c), c = fp32(scale) * fp32(log2 e) rounded to fp32 - the B operand of every score MFMA."""
    c = torch.tensor(float(scale), dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    return (q.to(dtype).float() * c).to(dtype)


def att_heads(t, H):
    """(B, N, H*D) -> (B, H, N, D)"""
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H).transpose(1, 2)


def att_tokens(t):
    """(B, H, N, D) -> (B, N, H*D)"""
    B, H, N, D = t.shape
    return t.transpose(1, 2).reshape(B, N, H * D)


class AttentionRef:
    """The float64 reference of one attention problem in the (B, T, H*D) layout of the output, and what its budget needs."""

    def __init__(self, q, k, v, H, scale, dtype):
        qs = att_heads(attention_prescale(q, scale, dtype).double(), H)
        kd, vd = att_heads(r64(k, dtype), H), att_heads(r64(v, dtype), H)
        self.dtype, self.S, self.D = dtype, k.shape[1], q.shape[2] // H
        s = qs @ kd.transpose(-1, -2)
        m = s.max(-1, keepdim=True).values
        p = torch.exp2(s - m)
        p = p / p.sum(-1, keepdim=True)
        ref, mag = p @ vd, p @ vd.abs()
        sd = (p @ (vd * vd) - ref * ref).clamp_min(0.0).sqrt()
        self.p = p                                                   # (B, H, T, S): the spotlight condition reads it
        self.ref, self.mag = att_tokens(ref), att_tokens(mag)
        self.weight = torch.minimum(self.mag + self.ref.abs(), att_tokens(sd))                  # W
        qk = (qs.abs() @ kd.abs().transpose(-1, -2)).max(-1, keepdim=True).values           # (B, H, T, 1)
        self.qk = att_tokens(qk.expand(-1, -1, -1, self.D))
        self.smag = self.qk + att_tokens((m.abs() + ATT_LAG).expand(-1, -1, -1, self.D))
        self.vsum = att_tokens(vd.abs().sum(-2, keepdim=True).expand(-1, -1, q.shape[1], -1))

    def relative(self):
        """e: the bound on the relative error of a P_k, per output element."""
        f32 = self.dtype == torch.float32
        e = (SPLIT_OPERAND_U if f32 else U_OUT[self.dtype]) + ATT_EXP2_ULPS * 2.0 ** -23 + math.log(2.0) * acc_bound(self.D, self.smag)
        if f32:
            e = e + math.log(2.0) * ATT_SPLIT_MULT * split_term(self.qk)
        return e

    def extra(self):
        """Everything beyond U_OUT |ref| + acc_bound(S, mag + |ref|): the `extra64` of assert_elementwise."""
        e = self.relative()
        x = e / (1.0 - e) * self.weight + ATT_SUBNORMAL_P[self.dtype] * (self.vsum + self.S * self.ref.abs())
        if self.dtype == torch.float32:
            x = x + ATT_SPLIT_MULT * split_term(self.mag + self.ref.abs())
        return x

    def gate(self, out, what):
        """assert_elementwise on every element; returns the worst ratio to the budget."""
        return assert_elementwise(out, self.ref, self.mag + self.ref.abs(), self.S, self.dtype, what, self.extra())

    def ratio(self, out):
        return gate_ratio(out, self.ref, self.mag + self.ref.abs(), self.S, self.dtype, self.extra())[0]


# ---- input families ------------------------------------------------------------------------------------------------------------
def att_spot_keys(S):
    """The keys the spotlight family must light: every key of the last two key tiles, the first and the last key of every tile."""
    nkt = (S + 63) // 64
    keys = set(range(max(0, (nkt - 2) * 64), S))
    for t in range(nkt):
        keys |= {t * 64, min(S, t * 64 + 64) - 1}
    return sorted(keys)


def att_spot_pairs(B, T, S, H):
    """[(b, h, row, key, gain)]: the row's gain cycles through ATT_SPOT_GAINS.  The two upper gains give their key most of the
    row whatever S is; 0.35 (four base-2 units: under the lag, the reference maximum stays) gives it 2^4 / (1.6 S + 2^4), under
    ATT_SPOT_MIN_P from S = 200 on.  So every required key goes to a row of the upper gains - one row each while a head has
    rows enough, else some rows carry two keys at the same gain and share the row - and the 0.35 rows take the keys that are
    not required, or (short S, where every key is required and 0.35 suffices) required ones again in another head."""
    need = att_spot_keys(S)
    other = [c for c in range(S) if c not in set(need)]
    strong = [r for r in range(T) if r % 3 != 0]
    weak = [r for r in range(T) if r % 3 == 0]
    if not strong:                                   # T = 1
        strong, weak = weak, []
    heads = B * H
    per_head = min(len(need), max(len(strong), -(-len(need) // heads)))
    pairs = []
    for n in range(heads):
        b, h = divmod(n, H)
        mine = [need[(n * per_head + i) % len(need)] for i in range(per_head)]
        pairs += [(b, h, strong[i % len(strong)], c, ATT_SPOT_GAINS[strong[i % len(strong)] % 3]) for i, c in enumerate(mine)]
        pool = other if other else [c for c in need if c not in set(mine)]
        pairs += [(b, h, r, pool[(n * len(weak) + i) % len(pool)], ATT_SPOT_GAINS[0]) for i, r in enumerate(weak[:len(pool)])]
    return pairs


def attention_inputs(family, B, T, S, H, D):
    """(q, k, v) of a family, fp32 on the CPU, (B, T | S, H*D); and the spotlight pairs (None elsewhere)."""
    C = H * D
    q, k, v = normal(f"a.q{B}.{T}.{C}", (B, T, C)), normal(f"a.k{B}.{S}.{C}", (B, S, C)), normal(f"a.v{B}.{S}.{C}", (B, S, C))
    amp = (64.0 / D) ** 0.5                           # the same score scale at every head size (scale = D^-0.5)
    pairs = None
    if family == "spotlight":
        pairs = att_spot_pairs(B, T, S, H)
        b, h, row, key = (torch.tensor([p[i] for p in pairs]) for i in range(4))
        g = torch.tensor([p[4] for p in pairs], dtype=torch.float32)[:, None]
        k4, q4 = k.view(B, S, H, D), q.view(B, T, H, D)            # (a key is lit once per head: no index repeats)
        k4[b, key, h] = 0.3 * k4[b, key, h] + g * amp * q4[b, row, h]
    elif family == "negative":
        u = normal(f"a.u{C}", (C,)) * amp ** 0.5
        q, k = u + 0.5 * q, -0.6 * u + 0.5 * k
    else:
        assert family == "normal"
    return q, k, v, pairs


def assert_spotlight_condition(ref: AttentionRef, pairs, S, H):
    """From the reference: every required key holds at least ATT_SPOT_MIN_P of some row that lights it, in tile 0 and in the
    last tile among them; returns the smallest of those probabilities."""
    b, h, row, key = (torch.tensor([p[i] for p in pairs]) for i in range(4))
    best = {}
    for c, pr in zip(key.tolist(), ref.p[b, h, row, key].tolist()):
        best[c] = max(best.get(c, 0.0), pr)
    need = att_spot_keys(S)
    low = {c: best.get(c, 0.0) for c in need if best.get(c, 0.0) < ATT_SPOT_MIN_P}
    assert not low, f"spotlight keys under {ATT_SPOT_MIN_P} of every row that lights them: {low}"
    assert 0 in best and S - 1 in best
    return min(best[c] for c in need)


# ---- which kernel a shape takes (attention.hip: attention16_launch, st_attention; attention_f32.hip; attention_anyd.hip) ----------
def _cdiv(a, b):
    return -(-a // b)


def attention_kernel(dtype, B, T, S, H, D):
    """(kernel, template arguments after the element type, grid) st_attention launches - the host's selection rule restated."""
    if D != 64:
        return "attn_anyd_kernel", (D, 4), (_cdiv(T, 64), H, B)
    if dtype == torch.float32:
        return "attn_split_kernel", (4, False), (_cdiv(T, 64) * H * B, 1, 1)
    if S < 256:
        return "attn16v2_kernel", (4, 1), (_cdiv(T, 64), H, B)
    nw = 4 if _cdiv(T, 256) * H * B <= 128 else 7
    if nw == 4 and _cdiv(T, 128) * H * B <= 176 and _cdiv(T, 96) * H * B <= 256:
        nw = 3
    if nw == 7:
        r7, r8 = _cdiv(_cdiv(T, 224) * H * B, 256), _cdiv(_cdiv(T, 256) * H * B, 256)
        if 6 * r8 < 5 * r7:
            nw = 8
    return "attn32i_kernel", (nw, nw != 8), (_cdiv(T, 32 * nw) * H * B, 1, 1)


# ---- the cases: (kernel tag, (B, T, S, H, D), family) -------------------------------------------------------------------------------
ATT_FAMILIES = ("normal", "spotlight", "negative")
ATT_HALF = (torch.bfloat16, torch.float16)


def _att_cases(tag, B, T, H, D, sizes, all_families):
    return [(tag, (B, T, S, H, D), f) for S in sizes for f in ATT_FAMILIES if f == "normal" or S in all_families]


# 16-row kernel: a second block with one live row; 1, 2, 3 and 4 key tiles against the ring of three, tails of 1, 13, 17 and 63
ATT_16V2 = _att_cases("attn16v2", 1, 65, 2, 64, (1, 17, 64, 65, 77, 128, 129, 192, 255), (77, 255))
# 32-row kernel: 4 to 13 key tiles (the six-slot ring wraps once from 385, twice at 769), tails on both sides of 32
ATT_32I_3 = _att_cases("attn32i-3", 1, 97, 1, 64, (256, 257, 288, 289, 319, 320, 321, 384, 385, 449, 769), (257, 289, 449))
ATT_32I_4 = _att_cases("attn32i-4", 1, 193, 90, 64, (257, 321, 449), (321,))            # cdiv(193, 128) * 90 = 180 > 176
ATT_32I_7 = _att_cases("attn32i-7", 1, 257, 65, 64, (257, 321, 449), (449,))            # 130 blocks of 256 rows > 128; the second: 33 live rows
ATT_32I_8 = _att_cases("attn32i-8", 1, 255, 130, 64, (256, 257, 289, 385, 769), (769,))    # r7 = 2, r8 = 1
ATT_16BIT = ATT_16V2 + ATT_32I_3 + ATT_32I_4 + ATT_32I_7 + ATT_32I_8
ATT_EXPECTED = {"attn16v2": ("attn16v2_kernel", (4, 1)), "attn32i-3": ("attn32i_kernel", (3, True)), "attn32i-4": ("attn32i_kernel", (4, True)),
                "attn32i-7": ("attn32i_kernel", (7, True)), "attn32i-8": ("attn32i_kernel", (8, False)),
                "anyd16": ("attn_anyd_kernel", (16, 4)), "anyd32": ("attn_anyd_kernel", (32, 4)), "anyd128": ("attn_anyd_kernel", (128, 4)),
                "split": ("attn_split_kernel", (4, False))}
# other head sizes (bf16, fp16, fp32): one LDS buffer, 1, 2 and 3 key tiles, tails of 1 and 63; every family at 65 and 129
ATT_ANYD = [c for D in (16, 32, 128) for c in _att_cases(f"anyd{D}", 2, 33, 3, D, (1, 63, 64, 65, 129), (65, 129))]
# fp32 at head size 64: two LDS buffers, 1 to 4 key tiles; st_attention and, on split images of K and V, st_attention_split
ATT_F32 = _att_cases("split", 1, 65, 2, 64, (1, 63, 64, 65, 128, 129, 193), (65, 193))


def attention_cases(dtype):
    return ATT_ANYD + (ATT_F32 if dtype == torch.float32 else ATT_16BIT)


# ------------------------------------------------------------------------------------------------ the conv family: dispatch restated, cases, operands
# (tests/test_conv_gate_host.py proves the gate on a CPU emulation of both conv loops; tests/test_conv_edges_gpu.py applies it.)
# The label of every case below - kernel, tile, K split - is COMPUTED by the restatements of the host's selection rules that
# follow (csrc/conv_halo.h: conv_halo_applies, conv_halo_launch; csrc/dispatch.h: gemm_dispatch) and asserted against the
# lists on the CPU; on the GPU, ColStats.rows (the tile's BM) is the piece of it a test can observe.
CONV_WORKSPACE_BYTES = 192 << 20          # ops.GEMM_WORKSPACE_BYTES: what a K split may use (the GPU tests assert the two agree)


def conv_geometry(cfg):
    """(Ho, Wo, M, K) of a case (N, Cin, H, W, Cout, k, stride, pad, ups)."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    He, We = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = (He + 2 * pad - k) // stride + 1, (We + 2 * pad - k) // stride + 1
    return Ho, Wo, N * Ho * Wo, k * k * Cin


def conv_halo_applies(dtype, cfg):
    """csrc/conv_halo.h: conv_halo_applies (kb: 64 channels a slice in 16 bit, 32 as split fp32)."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    Ho, Wo, M, _ = conv_geometry(cfg)
    kb = 32 if dtype == torch.float32 else 64
    if k != 3 or stride != 1 or pad != 1 or Cin % kb or Cout % 4 or Cout < 64:
        return False
    if ups:
        return Wo in (64, 128) and Ho % (256 // Wo) == 0 and M % 256 == 0
    if W not in (32, 64, 128) and not (W == 16 and kb == 64):
        return False
    bm = 128 if W == 128 else 256
    return H % (bm // W) == 0 and M % bm == 0


def conv_halo_plan(dtype, cfg, workspace_bytes=CONV_WORKSPACE_BYTES):
    """conv_halo_launch restated: (label, BM, BN, sk, tiles).  The K split is the time model's choice:
        rounds of 256 blocks x (tap trips per slice x trip_us + fixed_us) + per slice 1.2 us and its fp32 slab at ~4 TB/s,
    a slice keeps at least two channel slices, at most 8 slices (16 where the launch has at most 16 tiles); a later candidate
    must win by more than 0.5 us."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    Ho, Wo, M, _ = conv_geometry(cfg)
    sp = dtype == torch.float32
    sp128 = sp and Cout % 128 == 0 and Wo <= 64
    bm = 128 if (not ups and W == 128) else 256
    bn = (128 if sp128 else 64) if sp else (160 if (ups or W == 128) else 128)
    if not sp and not ups and W == 128:
        cost = lambda w: _cdiv((M // bm) * _cdiv(Cout, w), 256) * w
        if cost(128) < cost(160):
            bn = 128
    tiles = (M // bm) * _cdiv(Cout, bn)
    ncs = Cin // (32 if sp else 64)
    sk = 1
    if tiles <= 16384:
        trip_us, fixed_us = (0.75 if sp else 0.77) * bn / 128.0, (10.0 if sp else 5.4)
        slab_us = 2.0 * tiles * bm * bn * 4.0 / 4.0e6
        trips, cap = ncs * 9, (16 if tiles <= 16 else 8)
        max_sk = min(ncs // 2, cap)
        best = 1e30
        for s in range(1, max(max_sk, 1) + 1):
            if s > 1 and s * tiles * bm * bn * 4 + 65536 > workspace_bytes:
                break
            rounds = (tiles * s + 255) // 256
            t = rounds * (trips / float(s) * trip_us + fixed_us) + (s * (1.2 + slab_us) if s > 1 else 0.0)
            if t < best - 0.5:
                best, sk = t, s
    wl2 = Wo.bit_length() - 1
    label = f"halo<{wl2},{bm // Wo},{bn}{',ups' if ups else ''}>/sk{sk}"
    return label, bm, bn, sk, tiles


# gemm_dispatch's candidate list (tile, BM, BN, microseconds per K trip); a conv prices every trip at 1.6 x
IGEMM_CANDS = [("128x128", 128, 128, 0.53), ("64x128", 64, 128, 0.34), ("128x64", 128, 64, 0.32), ("64x64", 64, 64, 0.19),
               ("128x320", 128, 320, 1.9), ("64x320", 64, 320, 1.1), ("256x128", 256, 128, 0.72), ("128x80", 128, 80, 0.37),
               ("128x160", 128, 160, 0.66)]
IGEMM_SKS = (1, 2, 3, 4, 6, 8)


def conv_igemm_plan(dtype, cfg, workspace_bytes=CONV_WORKSPACE_BYTES, plain_f32=False):
    """gemm_dispatch<T, CONV = true> restated: (label, BM, BN, sk, tiles).  plain_f32: fp32 operands that are not split images
    (one configuration: 64 x 64, no K split)."""
    _, _, M, K = conv_geometry(cfg)
    Nc = cfg[4]
    if plain_f32:
        return "igemm<64x64,f32>/sk1", 64, 64, 1, _cdiv(M, 64) * _cdiv(Nc, 64)
    sp = dtype == torch.float32
    nk = K // (32 if sp else 64)
    best, pick = 1e30, None
    for name, bm, bn, trip_us in IGEMM_CANDS:
        if sp and (bn == 320 or name == "256x128"):
            continue
        nt = _cdiv(M, bm) * _cdiv(Nc, bn)
        trip = (0.8 if (sp and name == "128x160") else trip_us) * 1.6
        for s in IGEMM_SKS:
            if s > 1 and (nk // s < 4 or nt > 16384):
                break
            slab_mb = float(s) * nt * bm * bn * 4.0 / 1e6
            if s > 1 and slab_mb * 1e6 + 65536 > workspace_bytes:
                break
            rounds = float((nt * s + 255) // 256)
            trip_bw = float(min(nt * s, 256)) * (bm + bn) * 128.0 / 14.0e6
            cost = rounds * (_cdiv(nk, s) * max(trip, trip_bw) + 3.0) * (1.3 if rounds > 1.0 else 1.0) + \
                (2.1 + 0.4 * slab_mb if s > 1 else 0.0)
            if cost < best:
                best, pick = cost, (name, bm, bn, s, nt)
    name, bm, bn, s, nt = pick
    return f"igemm<{name}>/sk{s}", bm, bn, s, nt


def conv_plan(dtype, cfg, plain_f32=False):
    """Where ops.conv2d sends a case: the thin kernel, the halo conv or the implicit GEMM - (label, BM, BN, sk, tiles)."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    if plain_f32:
        assert dtype == torch.float32 and Cin % 32 == 0
        return conv_igemm_plan(dtype, cfg, plain_f32=True)
    if Cin % (32 if dtype == torch.float32 else 64):
        return "thin", 0, 0, 1, 0
    if conv_halo_applies(dtype, cfg):
        return conv_halo_plan(dtype, cfg)
    return conv_igemm_plan(dtype, cfg)


# ---- the cases: (label in bf16 / fp16, label as split fp32 or None, (N, Cin, H, W, Cout, k, stride, pad, ups)) ------------------
# Cin is the 16-bit one; the fp32 case has the same number of channel slices (a slice is 64 channels in 16 bit, 32 as split
# fp32: half the Cin - conv_cases does that).  label = kernel<template arguments>/sk<K slices>:
#   halo<WL2,TH,BN[,ups]>  conv_halo_kernel<T, WL2, TH, BN, 4, 2, UPS>: rows of 2^WL2 pixels, TH rows and BN channels a tile
#   igemm<BMxBN>           gemm_dma_kernel<T, BM, BN, ..., CONV = true>
# Smallest shapes that reach the path, about 2048 output pixels at most - two exceptions, both forced by the selection rule:
# the 160-channel halo tile at W = 128 without upsampling is only taken where 128-channel tiles need a second round of 256
# blocks and 160-channel tiles do not (43 rows x 644 channels: 258 against 215 tiles), and an implicit-GEMM tile other than
# 64 x 64 wins only once the 64 x 64 tiles fill more than a round (a 1x1 conv with thousands of output channels: cheap).
def _c3(n, cin, h, w, co, ups=False):
    return (n, cin, h, w, co, 3, 1, 1, ups)


def _c1(n, cin, h, w, co):
    return (n, cin, h, w, co, 1, 1, 0, False)


# halo conv, 16 bit, Cin = 128 (two slices: the patch double buffer and the weight ring's wrap), H > TH (a tile with an image
# row above and below it), a ragged last channel tile; W = 64 also H = TH with two images; W = 128 also H = 3 and 2
CONV_HALO_16 = [("halo<4,16,128>/sk1", None, _c3(2, 128, 32, 16, 136)), ("halo<5,8,128>/sk1", None, _c3(2, 128, 16, 32, 136)),
                ("halo<6,4,128>/sk1", None, _c3(1, 128, 8, 64, 136)), ("halo<6,4,128>/sk1", None, _c3(2, 128, 4, 64, 72)),
                ("halo<7,1,128>/sk1", None, _c3(1, 128, 3, 128, 136)), ("halo<7,1,128>/sk1", None, _c3(1, 128, 2, 128, 64)),
                ("halo<7,1,160>/sk1", None, _c3(1, 128, 43, 128, 644)),
                ("halo<6,4,160,ups>/sk1", None, _c3(1, 128, 4, 32, 168, True)), ("halo<7,2,160,ups>/sk1", None, _c3(1, 128, 2, 64, 168, True))]
# halo conv, split fp32 (listed with the 16-bit Cin = 128: 64 channels, two slices): the 64-channel tile, the 128-channel one
# (Cout % 128 == 0, Wout <= 64), the W = 128 form (always 64 channels), both upsampling forms
CONV_HALO_32 = [(None, "halo<5,8,64>/sk1", _c3(1, 128, 16, 32, 72)), (None, "halo<5,8,128>/sk1", _c3(1, 128, 16, 32, 128)),
                (None, "halo<6,4,64>/sk1", _c3(1, 128, 8, 64, 72)), (None, "halo<6,4,128>/sk1", _c3(2, 128, 4, 64, 128)),
                (None, "halo<7,1,64>/sk1", _c3(1, 128, 3, 128, 72)), (None, "halo<7,1,64>/sk1", _c3(1, 128, 2, 128, 128)),
                (None, "halo<6,4,64,ups>/sk1", _c3(1, 128, 4, 32, 72, True)), (None, "halo<6,4,128,ups>/sk1", _c3(1, 128, 4, 32, 128, True)),
                (None, "halo<7,2,64,ups>/sk1", _c3(1, 128, 2, 64, 72, True))]
# halo K split over channel slices: 4 slices in 2, 6 in 3, 5 in 2 and 7 in 3 (ncs % sk != 0: the first slices are longer), 20 in 9
# (cap = 16 at no more than 16 tiles; 20 % 9 = 2).  The 16-pixel level exists in 16 bit only: split fp32 takes 8 x 32 there.
CONV_HALO_SPLITS = [("halo<5,8,128>/sk2", "halo<5,8,128>/sk2", _c3(1, 256, 16, 32, 128)), ("halo<5,8,128>/sk3", "halo<5,8,128>/sk3", _c3(1, 384, 16, 32, 128)),
                    ("halo<6,4,128>/sk2", "halo<6,4,64>/sk2", _c3(1, 320, 8, 64, 72)), ("halo<5,8,128>/sk3", "halo<5,8,128>/sk3", _c3(1, 448, 16, 32, 128)),
                    ("halo<4,16,128>/sk9", None, _c3(1, 1280, 16, 16, 128)), (None, "halo<5,8,128>/sk9", _c3(1, 1280, 8, 32, 128))]
# implicit GEMM, every tile of gemm_dispatch's candidate list by a 1x1 conv with ragged M and ragged N (one K tile).  Split fp32
# is offered neither BN = 320 nor 256 x 128 (dispatch.h): those shapes land on the tiles named.  Every candidate is reachable.
CONV_IGEMM_TILES = [("igemm<64x64>/sk1", "igemm<64x64>/sk1", _c1(1, 64, 1, 70, 200)), ("igemm<64x128>/sk1", "igemm<64x128>/sk1", _c1(1, 64, 1, 33, 16392)),
                    ("igemm<128x64>/sk1", "igemm<128x64>/sk1", _c1(1, 64, 1, 70, 8200)), ("igemm<128x80>/sk1", "igemm<128x80>/sk1", _c1(1, 64, 1, 70, 16392)),
                    ("igemm<128x128>/sk1", "igemm<128x128>/sk1", _c1(1, 64, 1, 70, 20488)), ("igemm<128x160>/sk1", "igemm<128x160>/sk1", _c1(1, 64, 1, 70, 32776)),
                    ("igemm<256x128>/sk1", "igemm<64x128>/sk1", _c1(1, 64, 1, 134, 20488)), ("igemm<128x320>/sk1", "igemm<128x160>/sk1", _c1(1, 64, 1, 134, 32776)),
                    ("igemm<64x320>/sk1", "igemm<64x128>/sk1", _c1(1, 64, 1, 33, 40968))]
# implicit GEMM geometry: 3x3 at W = 12 and 24 (the UNet's levels at latent 96 x 64), stride 2 at an even and an odd size, 1x1
# at stride 2, pad 0, upsampling at an odd size, two images of 63 pixels (one M tile holds both: the row bias and img = mm / hw)
# - on 64 x 64 tiles (two K tiles a tap; the model splits K in four: 18 K tiles as 5 + 5 + 4 + 4, every boundary inside a tap)
# and again, with one K tile a tap, on the 128- and 64-row tiles a wide Cout selects; two images of 195 pixels on 128 x 160
# (the second M tile straddles them); 128 and 64 pixels an image (whole tiles: the launches that can emit column partials)
CONV_IGEMM_GEOM = [("igemm<64x64>/sk4", "igemm<64x64>/sk4", _c3(1, 128, 12, 12, 72)), ("igemm<64x64>/sk4", "igemm<64x64>/sk4", _c3(1, 128, 24, 24, 72)),
                   ("igemm<64x64>/sk4", "igemm<64x64>/sk4", (1, 128, 16, 12, 72, 3, 2, 1, False)), ("igemm<64x64>/sk4", "igemm<64x64>/sk4", (1, 128, 15, 13, 72, 3, 2, 1, False)),
                   ("igemm<64x64>/sk1", "igemm<64x64>/sk1", (1, 128, 9, 7, 72, 1, 2, 0, False)), ("igemm<64x64>/sk4", "igemm<64x64>/sk4", (1, 128, 9, 7, 72, 3, 1, 0, False)),
                   ("igemm<64x64>/sk4", "igemm<64x64>/sk4", _c3(1, 128, 5, 7, 72, True)), ("igemm<64x64>/sk4", "igemm<64x64>/sk4", _c3(2, 128, 9, 7, 72)),
                   ("igemm<128x64>/sk1", "igemm<128x64>/sk1", _c3(2, 64, 9, 7, 8200)), ("igemm<128x160>/sk1", "igemm<128x160>/sk1", _c3(2, 64, 15, 13, 8200)),
                   ("igemm<128x128>/sk1", "igemm<128x128>/sk1", _c3(2, 64, 9, 7, 20488)), ("igemm<64x64>/sk1", "igemm<64x64>/sk1", (1, 64, 16, 12, 8200, 3, 2, 1, False)),
                   ("igemm<64x128>/sk1", "igemm<64x128>/sk1", (1, 64, 15, 13, 16392, 3, 2, 1, False)), ("igemm<64x128>/sk1", "igemm<64x128>/sk1", _c3(1, 64, 5, 7, 8200, True)),
                   ("igemm<128x64>/sk1", "igemm<128x64>/sk1", _c3(1, 64, 16, 8, 8200)), ("igemm<64x64>/sk1", "igemm<64x64>/sk1", _c3(2, 64, 8, 8, 200))]
# implicit GEMM K splits with nk % sk != 0: 2 (27 K tiles: 14 + 13, the boundary inside a tap), 3 (a 3x3 conv has nk % 9 == 0, so
# thirds are whole taps: the uneven split in three is a 1x1 conv's, 13 K tiles as 5 + 4 + 4), 4, 6 and 8 on 64 x 64 tiles (18, 27,
# 36 K tiles: boundaries inside taps); on the production tiles 128 x 80 in 8, 6 and 4 (45, 45, 54 K tiles) and 128 x 64 in 4
# (63 K tiles: 16 + 16 + 16 + 15, two images of 575 pixels: the fifth M tile straddles them); stride 2 in four slices.
# (The model splits 256 x 128 only from 2304 pixels x 1280 channels on, and 128 x 128 in 16 bit not below that either: left out.)
CONV_IGEMM_SPLITS = [("igemm<64x64>/sk2", "igemm<64x64>/sk2", _c3(1, 192, 48, 48, 136)), ("igemm<64x64>/sk3", "igemm<64x64>/sk3", _c1(1, 832, 9, 7, 8)),
                     ("igemm<64x64>/sk4", "igemm<64x64>/sk4", _c3(1, 128, 5, 7, 8)), ("igemm<64x64>/sk6", "igemm<64x64>/sk6", _c3(1, 192, 5, 7, 8)),
                     ("igemm<64x64>/sk8", "igemm<64x64>/sk8", _c3(1, 256, 5, 7, 8)), ("igemm<128x80>/sk8", "igemm<128x80>/sk8", _c3(1, 320, 48, 48, 72)),
                     ("igemm<128x80>/sk6", "igemm<128x80>/sk6", _c3(1, 320, 48, 48, 136)), ("igemm<128x80>/sk4", "igemm<128x80>/sk4", _c3(1, 384, 48, 48, 200)),
                     ("igemm<128x64>/sk4", "igemm<128x64>/sk4", _c3(2, 448, 25, 23, 328)), ("igemm<64x64>/sk4", "igemm<64x64>/sk4", (1, 128, 48, 24, 320, 3, 2, 1, False))]
# conv2d_cat (1x1 over [x0 | x1], never materialised): (label, label, cfg with Cin = C0 + C1, C0) - C0 != C1; Csplit inside the K
# range of one launch, inside the second slice of a split in three (13 K tiles as 5 + 4 + 4, Csplit after 6) and of a split in
# four (19 as 5 + 5 + 5 + 4, Csplit after 7); on a 128-row tile.  Bit-equal to conv2d(torch.cat(...)).
CONV_CAT = [("igemm<64x64>/sk1", "igemm<64x64>/sk1", _c1(2, 192, 9, 7, 72), 64), ("igemm<64x64>/sk3", "igemm<64x64>/sk3", _c1(2, 832, 9, 7, 8), 384),
            ("igemm<64x64>/sk4", "igemm<64x64>/sk4", _c1(2, 1216, 9, 7, 72), 448), ("igemm<128x64>/sk1", "igemm<128x64>/sk1", _c1(1, 192, 1, 70, 8200), 128)]
# plain fp32 operands on the exact fp32 MFMA (gemm_dma_kernel<float, 64, 64, ..., CONV>, the 64 x 64 path): ops.conv2d takes it
# for an fp32 weight that is NOT channels_last (its split image is not made).  A conv with Cin % 32 != 0 that is not thin
# (k * k * Cin > 64) reaches no kernel: st_conv2d rejects it.  (cfg with the fp32 Cin itself.)
CONV_PLAIN_F32 = [("igemm<64x64,f32>/sk1", _c3(2, 64, 9, 7, 72)), ("igemm<64x64,f32>/sk1", (1, 32, 15, 13, 72, 3, 2, 1, False)),
                  ("igemm<64x64,f32>/sk1", _c3(1, 32, 5, 7, 72, True)), ("igemm<64x64,f32>/sk1", _c3(1, 64, 8, 32, 64))]
CONV_GROUPS = {"halo": CONV_HALO_16 + CONV_HALO_32, "halo-k-split": CONV_HALO_SPLITS, "igemm-tiles": CONV_IGEMM_TILES,
               "igemm-geometry": CONV_IGEMM_GEOM, "igemm-k-split": CONV_IGEMM_SPLITS}


def conv_cfg_for(dtype, cfg):
    """The listed (16-bit) case with the same number of channel slices in `dtype`."""
    return cfg if dtype != torch.float32 else (cfg[0], cfg[1] // 2) + tuple(cfg[2:])


def conv_cases(dtype, group):
    """[(label, cfg)] of a group in `dtype`."""
    i = 1 if dtype == torch.float32 else 0
    return [(c[i], conv_cfg_for(dtype, c[2])) for c in CONV_GROUPS[group] if c[i] is not None]


def conv_cat_cases(dtype):
    """[(label, cfg, C0)]"""
    i, div = (1, 2) if dtype == torch.float32 else (0, 1)
    return [(c[i], conv_cfg_for(dtype, c[2]), c[3] // div) for c in CONV_CAT]


def label_bm(label):
    """Rows of a tile (ColStats.rows) from a label: halo<WL2,TH,..> is TH << WL2, igemm<BMxBN> is BM."""
    args = label[label.index("<") + 1:label.index(">")].split(",")
    return (int(args[1]) << int(args[0])) if label.startswith("halo") else int(args[0].split("x")[0])


def label_sk(label):
    return int(label.rsplit("/sk", 1)[1])


# ---- two operand families -------------------------------------------------------------------------------------------------------------
# "normal": seeded normal operands, gated with the constants above at n_terms = k * k * Cin + max(0, sk - 8) (EPI_OPS holds up to
#     seven slab adds); split fp32 adds split_term.
# "exact": activations from {-1, 0, 1}, weights / bias / row bias / residual multiples of 1/8 below 2.  Every product is a
#     multiple of 1/8 and every partial sum - in any order, every K-split slab - is exact in fp32 while sum |terms| < 2^24 / 8
#     (asserted on the reference); the split image of such a value has an empty low half.  The budget is the store rounding
#     alone, U_OUT |ref| (fp32: equality), so ONE dropped or doubled term (at least 1/8) shows wherever U_OUT |ref| < 1/16 -
#     asserted for 99 % of the elements.  bf16 needs |ref| < 16 there: weights have variance 1.25, so a sum of n terms (and bias,
#     row bias, residual) deviates by 1.12 sqrt(n + 3); CONV_EXACT_TERMS[bf16] = 16 non-zero terms an output - a density of
#     16 / K - puts 16 at 3.3 deviations (0.1 % of the elements beyond it, which leaves room for the neighbours of the spots
#     below).  fp16 (|ref| < 128) and fp32 (no store rounding) take 400: 22 a deviation - and the column partials stay exact
#     too (colstats_ratios: 256 squares of mean 1.25 * 403 sum to half of 2^18).
CONV_EXACT_TERMS = {torch.bfloat16: 16, torch.float16: 400, torch.float32: 400}
CONV_FAMILIES = ("normal", "exact")


def _eighths(name, shape):
    g = torch.Generator().manual_seed(int.from_bytes(name.encode(), "little") % (2 ** 63 - 1))
    return torch.randint(-15, 16, shape, generator=g).float() / 8


def conv_operands(cfg, family, dtype):
    """(x, w, bias, rowbias, residual) of a case on the CPU in fp32 (the exact family's density depends on the type)."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    Ho, Wo, M, K = conv_geometry(cfg)
    tag = "-".join(str(int(v)) for v in cfg)
    if family == "normal":
        return (normal(f"c.x{tag}", (N, Cin, H, W)), normal(f"c.w{tag}", (Cout, Cin, k, k), K ** -0.5), normal(f"c.b{tag}", (Cout,)),
                normal(f"c.rb{tag}", (N, Cout)), normal(f"c.r{tag}", (N, Cout, Ho, Wo)))
    assert family == "exact"
    density = min(1.0, CONV_EXACT_TERMS[dtype] / K)
    g = torch.Generator().manual_seed(int.from_bytes(f"c.e{tag}".encode(), "little") % (2 ** 63 - 1))
    x = (torch.rand(N, Cin, H, W, generator=g) < density).float() * (torch.randint(0, 2, (N, Cin, H, W), generator=g).float() * 2 - 1)
    w, b = _eighths(f"c.ew{tag}", (Cout, Cin, k, k)), _eighths(f"c.eb{tag}", (Cout,))
    _exact_spots(x, w, b, cfg, dtype)
    return x, w, b, _eighths(f"c.erb{tag}", (N, Cout)), _eighths(f"c.er{tag}", (N, Cout, Ho, Wo))


# Below 32 (bf16) / 256 (fp16) every multiple of 1/8 is a value of the type, and up to twice that the others are ties: the exact
# family alone never makes a store round, so a store that rounds WRONGLY (towards zero) would pass it.  Two "spots" per case
# give it values that do round: the activations under one output element (n, co, oy, ox) are cleared and then set, one by one,
# to the sign of the weight they meet, until conv + bias lands in [64, 96) / [512, 768) on a value 3/8 above a multiple of 1/2
# in magnitude - there the type's spacing is 1/2, rounding to nearest errs by 1/8 and truncation by 3/8 > U_OUT |ref|.  Only
# where the output has 256 pixels (512 with upsampling: a spot's neighbours - 9 or 16 pixels whose sums gain up to 680 terms -
# stay inside the 1 % that may exceed 1/16 of store rounding; ConvCase asserts it) and the element has terms enough; fp32
# has no store rounding.
CONV_SPOT_RANGE = {torch.bfloat16: (64.0, 96.0), torch.float16: (512.0, 768.0)}


def _exact_spots(x, w, b, cfg, dtype):
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    Ho, Wo, M, K = conv_geometry(cfg)
    if dtype not in CONV_SPOT_RANGE or M < (512 if ups else 256):
        return 0
    lo, hi = CONV_SPOT_RANGE[dtype]
    made = 0
    for j in range(1 if (ups or M < 512) else 2):          # (few pixels, or upsampling's wider footprint: one spot's neighbours are enough)
        n, oy, ox, co = (N - 1) * j, (Ho // 3 + 5 * j) % Ho, (Wo // 2 + 7 * j) % Wo, (3 + 11 * j) % Cout
        weff = {}                                             # input pixel -> the weights it meets (upsampling: several taps share a pixel)
        for r in range(k):
            for s in range(k):
                iy, ix = oy * stride - pad + r, ox * stride - pad + s
                if not (0 <= iy < (2 * H if ups else H) and 0 <= ix < (2 * W if ups else W)):
                    continue
                key = (iy >> 1, ix >> 1) if ups else (iy, ix)
                weff[key] = weff.get(key, 0) + w[co, :, r, s]
        for (iy, ix) in weff:
            x[n, :, iy, ix] = 0.0
        v, done = float(b[co]), False
        for (iy, ix), wv in weff.items():
            for c in range(Cin):
                if float(wv[c]) == 0.0:
                    continue
                x[n, c, iy, ix] = 1.0 if float(wv[c]) > 0 else -1.0
                v += abs(float(wv[c]))
                if lo <= v < hi and (v * 8) % 4 == 3:
                    done = True
                    break
            if done:
                break
        if done:
            made += 1
        else:                                                 # not enough terms under this element: leave no half-made spot
            for (iy, ix) in weff:
                x[n, :, iy, ix] = 0.0
    return made


class ConvCase:
    """Operands and float64 reference of one conv case, type and family: `expect(epi)` gives (ref64, mag64, n_terms) of the plain
    (+bias) launch ("bias") and of the one with row bias and residual ("full"; conv2d_cat has no row bias: "res")."""

    def __init__(self, cfg, dtype, family, sk=1, split_operands=None):
        self.cfg, self.dtype, self.family, self.sk = cfg, dtype, family, sk
        N, Cin, H, W, Cout, k, stride, pad, ups = cfg
        self.x, self.w, self.b, self.rb, self.res = conv_operands(cfg, family, dtype)
        self.K = k * k * Cin
        self.split = (dtype == torch.float32) if split_operands is None else split_operands
        self.prod, self.magprod = conv_ref64(self.x, self.w, None, dtype, stride, pad, ups)
        if family == "exact":
            full_mag = self.magprod + r64(self.b, dtype).abs()[None, :, None, None] + r64(self.rb, dtype).abs()[:, :, None, None] + r64(self.res, dtype).abs()
            assert float(full_mag.max()) < 2.0 ** 24 / 8, f"conv {cfg} {dtype}: exact-sum operands are not exact (sum |terms| {float(full_mag.max())})"
            for t in (self.x, self.w, self.b, self.rb, self.res):
                assert torch.equal(t.to(dtype).float(), t) and torch.equal(t * 8, (t * 8).round())

    def expect(self, epi):
        d = self.dtype
        ref, mag = self.prod + r64(self.b, d)[None, :, None, None], self.magprod + r64(self.b, d).abs()[None, :, None, None]
        if epi == "full":
            ref, mag = ref + r64(self.rb, d)[:, :, None, None], mag + r64(self.rb, d).abs()[:, :, None, None]
        if epi in ("full", "res"):
            ref, mag = ref + r64(self.res, d), mag + r64(self.res, d).abs()
        n_terms = self.K + max(0, self.sk - 8)
        if self.family == "exact":
            blind = float((U_OUT[d] * ref.abs() >= 1.0 / 16).double().mean())
            assert blind <= 0.01, f"conv {self.cfg} {d} {epi}: {blind:.3%} of the outputs could hide a one-term error (store rounding >= 1/16)"
            return ref, torch.zeros_like(ref), n_terms
        if self.split:
            mag = mag + as_magnitude(split_term(self.magprod), n_terms)
        return ref, mag, n_terms

    def gate(self, out, epi, what):
        ref, mag, n_terms = self.expect(epi)
        return assert_elementwise(out, ref, mag, n_terms, self.dtype, what)


def colstats_ratios(buf, rows, stored, bm, exact, what):
    """Column partials (tiles, C, 2) of a launch against float64 sums of the STORED output over each tile's `rows` rows: the sums
    inside 2 (BM + 8) 2^-24 sum |stored| (BM fp32 adds in two levels, each at most twice a rounding, the slot adds among the 8),
    the squares the same on sum stored^2 (the fma rounds once per term); exact operands: equality (squares of multiples of 1/8 are multiples
    of 1/64: their sums are exact in fp32 below 2^18, asserted; a 16-bit store keeps a multiple of 1/8 one).  Returns the two
    worst ratios."""
    assert rows == bm, f"{what}: column partials over {rows} rows a tile, the case is labelled {bm}"
    o = stored.detach().double().cpu().permute(0, 2, 3, 1)
    C = o.shape[-1]
    o = o.reshape(-1, C)
    M = o.shape[0]
    assert M % rows == 0
    o = o.view(M // rows, rows, C)
    s = buf.detach().double().cpu()[:M // rows]
    assert tuple(s.shape) == (M // rows, C, 2) and torch.isfinite(s).all(), f"{what}: a column partial is not finite"
    s1, s2 = o.sum(1), (o * o).sum(1)
    k = 2.0 * (rows + 8) * U_ACC
    b1, b2 = k * o.abs().sum(1), k * s2
    if exact:          # equality wherever the fp32 sums are exact: every column but the few that hold a spot, which keep the bound
        small = (s2 < 2.0 ** 18) & (o.abs().sum(1) < 2.0 ** 21)
        assert int((~small).sum()) <= 2, f"{what}: the partials of these operands are not exact in fp32"
        bad = ((s[..., 0] != s1) | (s[..., 1] != s2)) & small
        assert not bool(bad.any()), f"{what}: column partials of exact operands are not exact ({int(bad.sum())} of {bad.numel()})"
        assert bool(((s[..., 0] - s1).abs() <= b1).all()) and bool(((s[..., 1] - s2).abs() <= b2).all()), f"{what}: column partials over their budget"
        return 0.0, 0.0
    r1 = float(((s[..., 0] - s1).abs() / b1.clamp_min(1e-300)).max())
    r2 = float(((s[..., 1] - s2).abs() / b2.clamp_min(1e-300)).max())
    assert r1 <= 1.0 and r2 <= 1.0, f"{what}: column partials {r1:.3g} (sums) / {r2:.3g} (squares) x their budget"
    return r1, r2


# ------------------------------------------------------------------------------------------------ the fp8 GEMM family: dispatch restated, cases, operands
# (tests/test_fp8_gate_host.py proves the gate on a CPU emulation of the e4m3 path; tests/test_fp8_edges_gpu.py applies it.)
FP8_WORKSPACE_BYTES = 192 << 20           # ops.GEMM_WORKSPACE_BYTES: what a K split may use (the GPU tests assert the two agree)
FP8_KB = 128                              # k per K tile: 128 bytes of e4m3


def dense_plan(M, K, N, geglu=False, ln=False, *, kb=FP8_KB, f8=True, workspace_bytes=FP8_WORKSPACE_BYTES):
    """gemm_dispatch<T, CONV = false> restated for a K that is a whole number of K tiles: (tile, BM, BN, sk, tiles).
      small_model  the candidates of IGEMM_CANDS in their order, a later one must be strictly cheaper; no BN = 320 for 32-byte
                   fragments (e4m3), no BN = 80 under GEGLU; every ST_TW_* factor is 1.0; a K trip is 128 bytes whatever the
                   type (kb = 128 k in e4m3, 64 in 16 bit); no K split with a folded LayerNorm; a slice keeps nk / sk >= 4 K tiles;
      eight-phase  gemm8p_applies (whole 256-row tiles, whole BN columns over value + gate rows, K >= 2 K tiles, N % 8 == 0),
                   c256 / c160 = rounds x (nk x 1.65 | 1.52 + 4), taken where the cheaper one is under ST_TW_8P = 1.1 x the
                   small tiles' best (c256 wins a tie).
    The column split of a 256 x 256 launch needs a launch without row scales: an e4m3 launch always has them; the 16-bit
    restatement (f8 = False: the lists of the LDS-DMA gate, which the CPU test holds this function to) refuses a shape
    that could take it."""
    rows = 2 * N if geglu else N
    nk = K // kb
    assert K % kb == 0 and nk >= 1
    best, pick = 1e30, None
    for name, bm, bn, trip in IGEMM_CANDS:
        if (f8 and bn == 320) or (geglu and bn % 32 != 0):
            continue
        nt = _cdiv(M, bm) * _cdiv(rows, bn)
        for s in IGEMM_SKS:
            if s > 1 and (ln or nk // s < 4 or nt > 16384):
                break
            slab_mb = float(s) * nt * bm * bn * 4.0 / 1e6
            if s > 1 and slab_mb * 1e6 + 65536 > workspace_bytes:
                break
            rounds = float((nt * s + 255) // 256)
            trip_bw = float(min(nt * s, 256)) * (bm + bn) * 128.0 / 14.0e6
            cost = rounds * (_cdiv(nk, s) * max(trip, trip_bw) + 3.0) * (1.3 if rounds > 1.0 else 1.0) + \
                (2.1 + 0.4 * slab_mb if s > 1 else 0.0)
            if cost < best:
                best, pick = cost, (name, bm, bn, s, nt)
    c = {}
    for bn, per_trip in ((256, 1.65), (160, 1.52)):
        applies = M % 256 == 0 and rows % bn == 0 and K >= 2 * kb and N % 8 == 0
        nt = _cdiv(M, 256) * _cdiv(rows, bn)
        c[bn] = (float((nt + 255) // 256) * (nk * per_trip + 4.0), nt) if applies else (1e30, nt)
    if not f8 and c[256][0] < 1e29:
        total, tm = c[256][1], M // 256
        assert not (total > 256 and 0 < total % 256 <= 128 and 256 % tm == 0), "dense_plan: the column split is not restated"
    if c[256][0] < 1e29 and c[256][0] <= c[160][0] and c[256][0] < 1.1 * best:
        return "256x256", 256, 256, 1, c[256][1]
    if c[160][0] < 1e29 and c[160][0] < c[256][0] and c[160][0] < 1.1 * best:
        return "256x160", 256, 160, 1, c[160][1]
    return pick


def fp8_plan(M, K, N, geglu=False, ln=False):
    """(tile, BM, BN, sk, tiles) of gemm_dispatch<f8, false> (st_linear_fp8, st_linear_fp8x)."""
    return dense_plan(M, K, N, geglu, ln, kb=FP8_KB, f8=True)


# ---- the cases: (tile the dispatch takes, (M, K, N)); every label is asserted against fp8_plan on the CPU ---------------------------
# one K tile (K = 128), a partial last M tile and a partial last N tile on every tile the e4m3 GEMM is offered, N % 8 == 0
FP8_PLAIN = [("64x64", (1, 128, 8)), ("64x64", (70, 128, 200)), ("128x64", (197, 128, 4128)), ("64x128", (259, 128, 4128)),
             ("128x128", (400, 128, 5128)), ("128x80", (450, 128, 3368)), ("128x160", (771, 128, 4648)), ("256x128", (1027, 128, 4488))]
FP8_GEGLU = [("64x64", (1, 128, 8)), ("64x64", (100, 128, 40)), ("128x64", (71, 128, 4168)), ("64x128", (134, 128, 3088)),
             ("128x128", (197, 128, 4128)), ("128x160", (400, 128, 4128)), ("256x128", (400, 128, 5128))]      # (BN = 80 is not offered to GEGLU)
FP8_WIDE_TILES = ("128x160", "256x128")
# K tiles against ring stages (four; 256 x 128 three): 2, 3, 4, 5 K tiles - odd and even trip counts of a loop that runs two
# trips an iteration (one fragment set per stage)
FP8_RING_K = (256, 384, 512, 640)
# the uneven K splits of the 16-bit gate with K doubled: the same nk, the same tile, the same sk
FP8_UNEVEN_SPLITS = [(sk, t, (M, 2 * K, N)) for sk, t, (M, K, N) in DMA_UNEVEN_SPLITS]
FP8_LN_K = (256, 1280)
FP8_PER_TENSOR_TILES = ("64x64", "128x80", "256x128")
# row statistics: the buffer holds 64 N tiles (ops.STATS_MAX_CHUNKS): 128 x 64 at N = 4128 (65 tiles) cannot emit them and has a
# shape of its own, as in DMA_STATS
FP8_STATS = [(t, (257, 128, 3272) if t == "128x64" else s) for t, s in FP8_PLAIN]
# eight-phase kernel (whole tiles only), the smallest shapes the model gives it: (tile, (M, K, N), geglu, folded LayerNorm)
FP8_GEMM8P = [("256x256", (768, 256, 11008), False, False), ("256x256", (768, 640, 11008), False, False),
              ("256x160", (5632, 256, 1440), False, False), ("256x160", (5632, 640, 1440), False, False),
              ("256x256", (768, 256, 5504), True, False), ("256x160", (5632, 256, 720), True, False),
              ("256x256", (768, 640, 5504), True, True), ("256x160", (5632, 640, 720), True, True)]
FP8_FAMILIES = ("normal", "exact")


def fp8_ring():
    """The plain shape of every tile with M > 1 at 2, 3, 4 and 5 K tiles."""
    return [(t, (M, k, N)) for t, (M, _, N) in FP8_PLAIN if M > 1 for k in FP8_RING_K]


def fp8_wide():
    return [(t, s) for t, s in FP8_PLAIN if t in FP8_WIDE_TILES]


def fp8_ln():
    """(tile, shape, geglu): the plain and the GEGLU shape of every tile with M > 1 at K = 256 and 1280."""
    return [(t, (M, k, N), g) for g, lst in ((False, FP8_PLAIN), (True, FP8_GEGLU)) for t, (M, _, N) in lst if M > 1 for k in FP8_LN_K]


def fp8_per_tensor():
    return [(t, s) for t, s in FP8_PLAIN if t in FP8_PER_TENSOR_TILES and s[0] > 1]


# ---- operands: the bytes and the scales themselves ----------------------------------------------------------------------------------
# The GEMM's operands are e4m3 bytes and fp32 scales, made on the host: no test of the GEMM depends on a quantiser kernel.
# "normal": seeded normal values; activation row m carries the factor 1.7^-(m % 7), weight row n 1.7^-(n % 5) (at most 1: the
#     pre-activations keep about unit variance, under ACT_RANGE among millions).  7 and 5 are coprime to every tile dimension, and
#     neighbours in either cycle differ by 1.7 or more (the wrap by 1.7^6 / 1.7^4): quantised to amax / 448 per row, a scale
#     taken from ANY other row or column of a tile is off by far more than 2^-8.  Per tensor: one scale for the whole activation.
#     Budget: assert_elementwise at n_terms = K + what the launch form spends beyond EPI_OPS (fp8_n_terms).  A product of two
#     e4m3 values has 8 significand bits: exact in fp32.
# "exact": activation bytes from {-1, 0, 1} at density 16 / K, weight bytes, bias and residual multiples of 1/8 below 2 (each an e4m3
#     value: asserted), row scales 2^(m % 7), column scales 2^(n % 5) (per tensor: 4).  Every term is a multiple of rs cs / 8 >= 1/8, so
#     every partial sum, slab and scaled value is exact in fp32 while 8 sum |terms| < 2^24 (asserted on the reference): the
#     budget is the bf16 store alone, U_OUT |ref| with mag = 0.  ONE dropped or doubled term is at least rs cs / 8 and shows
#     wherever U_OUT |ref| < rs cs / 16 - asserted for 99 % of the elements (measured on the reference alone: 0.04 - 0.08 % are
#     blind).  No scale below 1: with 2^-j scales a bias of eighths would leave 59 % of the elements blind (measured).
# How v_mfma_scale_f32_16x16x128_f8f6f4 rounds inside its 128-term sum has not been measured on the instruction alone
# (profiles/r05_mfma_accumulation.txt covers the f16 and f32 instructions): ACC_FACTOR = 2 is the assumption here as elsewhere.
# The exact family does not depend on it (no sum of it rounds); the normal family's budget is led by the bf16 store except
# under cancellation.  Should the normal family ever exceed its budget on the device while the exact family holds bit for bit,
# the instruction's own summation is the suspect: measure it alone (tools/mfma_acc_probe.py is the style), never fit it here.
E4M3 = torch.float8_e4m3fn
FP8_MAX = 448.0


def e4m3_bytes(t):
    q = t.float().to(E4M3)
    assert bool(torch.isfinite(q.float()).all()), "a value beyond the e4m3 range"
    return q.view(torch.uint8)


def e4m3_f64(q):
    return q.view(E4M3).double()


def quantise_rows(t, per_tensor=False):
    """(bytes, fp32 scales): amax / 448 per row, or one scale for the whole tensor."""
    amax = t.abs().amax().reshape(1) if per_tensor else t.abs().amax(1)
    scale = amax.float().clamp_min(1e-12) / FP8_MAX
    return e4m3_bytes(t / scale[:, None]), scale.contiguous()


def _cycle(n, period):
    return torch.pow(torch.tensor(1.7), -(torch.arange(n) % period).float())


def _signs_at_density(name, shape, density):
    g = torch.Generator().manual_seed(int.from_bytes(name.encode(), "little") % (2 ** 63 - 1))
    return (torch.rand(*shape, generator=g) < density).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


class Fp8Problem:
    """Bytes, scales, bias and the float64 products of one (M, K, weight rows) problem in a family: shared between epilogues."""

    def __init__(self, M, K, rows, family, per_tensor=False):
        self.M, self.K, self.rows, self.family, self.per_tensor = M, K, rows, family, per_tensor
        if family == "normal":
            x = normal(f"8.x{M}.{K}", (M, K)) * _cycle(M, 7)[:, None]
            w = normal(f"8.w{rows}.{K}", (rows, K), K ** -0.5) * _cycle(rows, 5)[:, None]
            self.xq, self.rs = quantise_rows(x, per_tensor)
            self.wq, self.cs = quantise_rows(w)
            self.bias = normal(f"8.b{rows}", (rows,), 0.5)
        else:
            assert family == "exact"
            x, w = _signs_at_density(f"8.ex{M}.{K}", (M, K), min(1.0, 16.0 / K)), _eighths(f"8.ew{rows}.{K}", (rows, K))
            self.xq, self.wq = e4m3_bytes(x), e4m3_bytes(w)
            assert torch.equal(e4m3_f64(self.xq), x.double()) and torch.equal(e4m3_f64(self.wq), w.double())      # every value IS an e4m3 value
            self.rs = torch.full((1,), 4.0) if per_tensor else torch.pow(torch.tensor(2.0), (torch.arange(M) % 7).float())
            self.cs = torch.pow(torch.tensor(2.0), (torch.arange(rows) % 5).float())
            self.bias = _eighths(f"8.eb{rows}", (rows,))
        xd, wd = e4m3_f64(self.xq), e4m3_f64(self.wq)
        self.unit = self.rs.double()[:, None] * self.cs.double()[None, :]          # (M | 1, rows): what one unit of the byte product is worth
        self.prod, self.magprod = (xd @ wd.T) * self.unit, (xd.abs() @ wd.abs().T) * self.unit

    def residual(self, N):
        return normal(f"8.r{self.M}.{N}", (self.M, N)) if self.family == "normal" else _eighths(f"8.er{self.M}.{N}", (self.M, N))


def fp8_n_terms(K, *, sk=1, bias=False, residual=False, act=False, ln=False):
    """n_terms of the budget: K, plus the fp32 operations of the launch form beyond the EPI_OPS the budget has already: sk - 1
    slab adds, two multiplies for the scales (rs * cs, then the product with the sum), the two FMAs of a fold, bias, the two of
    a SiLU / GEGLU (the activation's product and the gate's bias), residual."""
    ops_ = (sk - 1) + 2 + (2 if ln else 0) + int(bias) + (2 if act else 0) + int(residual)
    return K + max(0, ops_ - EPI_OPS)


def fp8_expect(prob, *, bias=True, silu=False, geglu=False, residual=None, sk=1):
    """(ref64, mag64, extra64, n_terms) of st_linear_fp8 / st_linear_fp8x (no fold) on a problem's operands: the scaled product,
    then linear_ref64's epilogue.  Exact family: mag = 0, after the conditions of the family have been asserted on the reference."""
    dt = torch.bfloat16
    ref, mag, extra = linear_ref64(None, None, prob.bias if bias else None, dt, silu=silu, geglu=geglu, residual=residual,
                                   products=(prob.prod, prob.magprod), K=prob.K)
    n_terms = fp8_n_terms(prob.K, sk=sk, bias=bias, residual=residual is not None, act=silu or geglu)
    if prob.family == "exact":
        assert not silu and not geglu, "the exact family has plain, bias and residual epilogues only"
        assert 8.0 * float(mag.max()) < 2.0 ** 24, f"fp8 {(prob.M, prob.K, prob.rows)}: exact-sum operands are not exact in fp32"
        blind = float((U_OUT[dt] * ref.abs() >= prob.unit / 16.0).double().mean())
        assert blind <= 0.01, f"fp8 {(prob.M, prob.K, prob.rows)}: {blind:.3%} of the outputs could hide a one-term error"
        return ref, torch.zeros_like(ref), None, n_terms
    return ref, mag, extra, n_terms


# ---- the fold's activation: a bf16 tensor as its producer stored it, its row partials, its e4m3 copy under a delayed scale ----------
def fp8_ln_operands(M, K, rows):
    """(x, gamma, beta, w, bias) of a LayerNorm-fold case: rows with a non-zero mean whose size cycles with period 7 (rstd differs
    from row to row by 1.7 and more), weight rows that cycle with period 5."""
    x, g, be, w, b = dma_ln_operands(M, K, rows)
    return x * (_cycle(M, 7) * 1.7 ** 3)[:, None], g, be, w * _cycle(rows, 5)[:, None], b


def fp8_delayed_scale(amax):
    """(scale, 1 / scale) as st_fp8_update_scales leaves them for a tensor whose producer saw max |value| = amax: fp32 arithmetic,
    margin 2 (ops.FP8_MARGIN)."""
    s = torch.tensor(2.0, dtype=torch.float32) * torch.as_tensor(amax, dtype=torch.float32) / torch.tensor(FP8_MAX, dtype=torch.float32)
    return s, torch.tensor(1.0, dtype=torch.float32) / s


def e4m3_copy(stored, inv_scale):
    """The copy an epilogue leaves: e4m3(clamp(fp32(stored) * inv_scale)) - bytes."""
    return (stored.float() * inv_scale).clamp(-FP8_MAX, FP8_MAX).to(E4M3).view(torch.uint8)


def fp8_fold(gamma, beta, w, bias):
    """ops.fold_layer_norm_fp8 on the CPU (the same torch arithmetic on bf16-rounded parameters): (bytes, scales, c, d)."""
    g, be, wt, b = (t.to(torch.bfloat16).float() for t in (gamma, beta, w, bias))
    wq, ws = quantise_rows(wt * g[None, :])
    c = (wq.view(E4M3).float().sum(1) * ws).contiguous()
    return wq, ws, c, (wt @ be + b).contiguous()


def fp8_ln_reference(x_stored, q, scale, wq, ws, c, d, eps, geglu):
    """(ref64, mag64, extra64, n_terms) of st_linear_fp8x with a folded LayerNorm: the row statistics are those of the bf16
    tensor its producer stored, the product is that of the tensor's e4m3 copy q under its one scale and the folded weight's
    bytes under their per-row scales; c and d are fold_layer_norm_fp8's."""
    K = q.shape[1]
    unit = float(scale) * ws.double()[None, :]
    xd, wd = e4m3_f64(q), e4m3_f64(wq)
    ref, mag, extra = ln_linear_ref64(x_stored.float(), None, c, d, torch.bfloat16, eps, geglu=geglu,
                                      products=((xd @ wd.T) * unit, (xd.abs() @ wd.abs().T) * unit))
    return ref, mag, extra, fp8_n_terms(K, ln=True, act=geglu)
