"""CPU proof that the per-element gate of tests/edge_util.py bites: an emulation of the kernels' arithmetic (fp32 sum of the
rounded operands, fp32 epilogue, ONE rounding to the stored type) passes it at every shape the GPU tests use, and every
mutation a kernel bug would amount to fails it.  No GPU, no operator library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import edge_util as eu

HALF = [torch.bfloat16, torch.float16]


def _name(dtype):
    return str(dtype).split(".")[-1]


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
def _truncate(v32: torch.Tensor, dtype) -> torch.Tensor:
    """fp32 -> dtype rounding toward zero (what a store that drops the low bits does)."""
    if dtype == torch.bfloat16:
        return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(dtype)
    h = v32.to(dtype)
    over = h.float().abs() > v32.abs()                      # rounded away from zero: step back by one ulp
    bits = h.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dtype)      # (sign-magnitude: -1 on the bits is towards zero for both signs)


def emulate_linear(x, w, b, dtype, mutation=None):
    xr, wr = x.to(dtype).float(), w.to(dtype).float()
    br = None if b is None else b.to(dtype).float()
    if mutation == "drop_tail8":
        xr, wr = xr[:, :-8], wr[:, :-8]
    elif mutation == "drop_one_k":
        keep = [k for k in range(xr.shape[1]) if k != xr.shape[1] // 2]
        xr, wr = xr[:, keep], wr[:, keep]
    acc = F.linear(xr, wr)
    if mutation == "round_before_bias":
        acc = acc.to(dtype).float()
    if br is not None:
        if mutation == "bias_shift":
            br = br.clone()
            br[-1] = br[-2]
        acc = acc + br
    return _truncate(acc, dtype) if mutation == "truncate" else acc.to(dtype)


def emulate_conv(x, w, b, dtype, stride, pad, ups, mutation=None):
    xr, wr, br = x.to(dtype).float(), w.to(dtype).float(), b.to(dtype).float()
    if ups:
        xr = F.interpolate(xr, scale_factor=2.0, mode="nearest")
    if mutation == "pad_row_reads_neighbour":
        assert pad == 1
        xp = F.pad(xr, (1, 1, 1, 1))
        xp[:, :, 0, 1:-1] = xr[:, :, 0]                     # the zero row above the image holds the image's first row
        return F.conv2d(xp, wr, br, stride=stride).to(dtype)
    return F.conv2d(xr, wr, br, stride=stride, padding=pad).to(dtype)


def _linear_operands(M, K, N, rows=None):
    rows = N if rows is None else rows
    return (eu.normal(f"h.x{M}.{K}", (M, K)), eu.normal(f"h.w{rows}.{K}", (rows, K), K ** -0.5), eu.normal(f"h.b{rows}", (rows,)))


def _conv_operands(cfg):
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    return (eu.normal(f"h.cx{Cin}.{H}", (N, Cin, H, W)), eu.normal(f"h.cw{Cout}.{Cin}", (Cout, Cin, k, k), (Cin * k * k) ** -0.5),
            eu.normal(f"h.cb{Cout}", (Cout,)))


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_emulated_linear_passes_at_every_gpu_shape(dtype):
    """Measured: 0.93-0.99 of the budget for bf16 / fp16 (a correctly rounded store uses all of U_OUT * |ref| somewhere among
    tens of thousands of elements), under 0.15 for fp32."""
    worst = 0.0
    for (M, K, N) in eu.linear_cases(dtype):
        x, w, b = _linear_operands(M, K, N)
        ref, mag, _ = eu.linear_ref64(x, w, b, dtype)
        worst = max(worst, eu.assert_elementwise(emulate_linear(x, w, b, dtype), ref, mag, K, dtype, f"emulated linear {(M, K, N)}"))
    print(f"emulated linear {dtype}: worst ratio {worst:.3f}")
    assert worst > (0.5 if dtype != torch.float32 else 0.0)      # the gate is tight: the emulation uses most of it


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_emulated_activation_epilogues_pass(dtype):
    """SiLU and GEGLU epilogues: the activation as the exact function of the fp32 pre-activation, rounded to fp32."""
    M, K, N = 70, 72, 200
    x, w, b = _linear_operands(M, K, N)
    pre = F.linear(x.to(dtype).float(), w.to(dtype).float(), b.to(dtype).float())
    ref, mag, extra = eu.linear_ref64(x, w, b, dtype, silu=True)
    eu.assert_elementwise(eu.silu64(pre.double()).float().to(dtype), ref, mag, K, dtype, "emulated linear+silu", extra)
    for (M, K, Fh) in eu.LINEAR_GEGLU:
        x, w, b = _linear_operands(M, K, Fh, rows=2 * Fh)
        pre = F.linear(x.to(dtype).float(), w.to(dtype).float(), b.to(dtype).float())
        out = (pre[:, :Fh] * eu.gelu64(pre[:, Fh:].double()).float()).to(dtype)
        ref, mag, extra = eu.linear_ref64(x, w, b, dtype, geglu=True)
        eu.assert_elementwise(out, ref, mag, K, dtype, f"emulated linear+geglu {(M, K, Fh)}", extra)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_emulated_conv_passes_at_every_gpu_shape(dtype):
    halo = [(n, c, h, w, co, 3, 1, 1, False) for (n, c, h, w, co) in eu.HALO_CONVS] + \
           [(n, c, h, w, co, 3, 1, 1, True) for (n, c, h, w, co) in eu.HALO_CONVS_UPS]
    for cfg in eu.THIN_CONVS + halo + eu.IGEMM_CONVS:      # (Cin = 64: 576 terms, gated in every type)
        N, Cin, H, W, Cout, k, stride, pad, ups = cfg
        x, w, b = _conv_operands(cfg)
        ref, mag = eu.conv_ref64(x, w, b, dtype, stride, pad, ups)
        eu.assert_elementwise(emulate_conv(x, w, b, dtype, stride, pad, ups), ref, mag, k * k * Cin, dtype, f"emulated conv {cfg}")


# ------------------------------------------------------------------------------------------------ every mutation fails
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["drop_tail8", "drop_one_k", "bias_shift"])
@pytest.mark.parametrize("shape", [(70, 72, 200), (64, 136, 72)])
def test_linear_indexing_mutations_fail(dtype, mutation, shape):
    """A dropped K tail (the `k0 + c * VEC < K` mask off by one vector), one dropped k, the last output column with its
    neighbour's bias: hundreds to hundreds of thousands of times the budget."""
    M, K, N = shape
    x, w, b = _linear_operands(M, K, N)
    ref, mag, _ = eu.linear_ref64(x, w, b, dtype)
    with pytest.raises(AssertionError, match="x its budget"):
        eu.assert_elementwise(emulate_linear(x, w, b, dtype, mutation), ref, mag, K, dtype, mutation)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("mutation", ["truncate", "round_before_bias"])
@pytest.mark.parametrize("shape", [(70, 72, 200), (64, 136, 72), (130, 8, 64)])
def test_linear_rounding_mutations_fail_at_short_k(dtype, mutation, shape):
    """A truncating store (error up to 2 U_OUT |ref|) and a result rounded before the bias add (U_OUT |sum| + U_OUT |ref|) only
    exceed the budget while its accumulation term 2 (K + 8) 2^-24 mag stays below the store rounding U_OUT |ref|: mag / |ref| is
    typically 5-50, so at K = 136 the term is 1.7e-5 mag against 4.9e-4 |ref| (fp16) - well below - while at K = 1288 it is
    1.5e-4 mag, as large as the rounding itself, and a truncating fp16 store passes.  Hence K <= 136 in every case that uses
    the gate, and these two mutations are only asserted there.  (fp32 stores its accumulator as it is: there is no store
    rounding to get wrong.)"""
    M, K, N = shape
    assert K <= 136
    x, w, b = _linear_operands(M, K, N)
    ref, mag, _ = eu.linear_ref64(x, w, b, dtype)
    with pytest.raises(AssertionError, match="x its budget"):
        eu.assert_elementwise(emulate_linear(x, w, b, dtype, mutation), ref, mag, K, dtype, mutation)


_PAD_CASES = [(d, c) for d in eu.DTYPES for c in [(1, 3, 9, 7, 32, 3, 1, 1, False), (1, 7, 8, 8, 16, 3, 2, 1, False), (1, 4, 5, 7, 32, 3, 1, 1, True)]] + \
             [(d, (1, 64, 3, 128, 160, 3, 1, 1, False)) for d in eu.DTYPES]      # (Cin = 64: n_terms = 576)


@pytest.mark.parametrize("dtype,cfg", _PAD_CASES, ids=lambda v: _name(v) if isinstance(v, torch.dtype) else "-".join(str(int(e)) for e in v))
def test_conv_padding_mutation_fails(dtype, cfg):
    """One row of zero padding read as the neighbouring image row."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    x, w, b = _conv_operands(cfg)
    ref, mag = eu.conv_ref64(x, w, b, dtype, stride, pad, ups)
    with pytest.raises(AssertionError, match="x its budget"):
        eu.assert_elementwise(emulate_conv(x, w, b, dtype, stride, pad, ups, "pad_row_reads_neighbour"), ref, mag, k * k * Cin, dtype, "padding")


def test_failure_message_names_the_worst_element():
    ref = torch.zeros(3, 4, dtype=torch.float64) + 1.0
    out = ref.clone().float()
    out[2, 1] = 1.5
    with pytest.raises(AssertionError, match=r"element \(2, 1\) = 1\.5, float64 reference 1\.0"):
        eu.assert_elementwise(out, ref, ref.abs(), 8, torch.float32, "msg")
    out[0, 0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        eu.assert_elementwise(out, ref, ref.abs(), 8, torch.float32, "msg")


# ------------------------------------------------------------------------------------------------ the activations' own error
def _gelu_fast_f32(x):
    """csrc/common.h gelu_erf_fast_f in numpy float32 (division and exp2 correctly rounded where the device takes v_rcp / v_exp)."""
    f = np.float32
    x = x.astype(f)
    z = np.abs(x) * f(0.70710678118654752)
    t = f(1.0) / (f(0.3275911) * z + f(1.0))
    poly = f(1.061405429) * t + f(-1.453152027)
    poly = poly * t + f(1.421413741)
    poly = poly * t + f(-0.284496736)
    poly = poly * t + f(0.254829592)
    e = np.exp2(z * z * f(-1.4426950408889634)).astype(f)
    erf_abs = (-poly * t) * e + f(1.0)
    half_x = f(0.5) * x
    return np.abs(half_x) * erf_abs + half_x


def _silu_f32(x):
    f = np.float32
    x = x.astype(f)
    return x / (f(1.0) + np.exp(-x).astype(f))


def test_activation_error_constants():
    """The float32 restatements of the device activations against the exact functions in float64 over [-8, 8] (2^20 + 1 points):
    gelu_erf_fast_f deviates by 4.68e-7 at most, x / (1 + expf(-x)) by 7.03e-7 (asserted below with 7 % of margin: 5.0e-7 and
    7.5e-7).  edge_util's constants add the allowance for the device's one-ulp v_rcp_f32 /
    v_exp_f32 and two-ulp expf derived there: GELU_FAST_ABS_ERR = 1.5e-6 and SILU_ABS_ERR = 2.7e-6 must cover the measured
    figure plus that allowance.  The reference is the exact function, never the kernel."""
    x = np.linspace(-eu.ACT_RANGE, eu.ACT_RANGE, (1 << 20) + 1)
    x32 = x.astype(np.float32).astype(np.float64)
    xt = torch.from_numpy(x32)
    gelu_dev = float(np.abs(_gelu_fast_f32(x32).astype(np.float64) - eu.gelu64(xt).numpy()).max())
    silu_dev = float(np.abs(_silu_f32(x32).astype(np.float64) - eu.silu64(xt).numpy()).max())
    print(f"gelu_erf_fast_f restatement: max |error| {gelu_dev:.3e}; silu restatement: {silu_dev:.3e}")
    MEASURED_GELU, MEASURED_SILU = 5.0e-7, 7.5e-7      # measured 4.68e-7 and 7.03e-7
    assert gelu_dev <= MEASURED_GELU and silu_dev <= MEASURED_SILU
    ulp_allowance = 0.5 * eu.ACT_RANGE * 2.0 ** -23                  # one ulp of a factor of 0.5 |x| erf(...)
    assert MEASURED_GELU + 2 * ulp_allowance <= eu.GELU_FAST_ABS_ERR
    assert MEASURED_SILU + 2 * 2.0 ** -23 * eu.ACT_RANGE <= eu.SILU_ABS_ERR
    # both slopes stay under ACT_SLOPE
    h = 1e-6
    for fn in (eu.gelu64, eu.silu64):
        slope = ((fn(xt + h) - fn(xt - h)) / (2 * h)).abs().max()
        assert float(slope) <= eu.ACT_SLOPE
