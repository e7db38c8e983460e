"""Every attention kernel behind ops.attention gated per element against float64 (tests/edge_util.py: AttentionRef - the
reference on the values the kernels are documented to see, a derived budget): the 16-row kernel's three-slot ring at 1 to 4 key
tiles, attn32i_kernel in its 3, 4 and 7 compute-wave forms with a loader wave and its 8-wave self-loading form (the six-slot
ring before and after it wraps, both halves of mask_tail, the dummy DMAs past the last tile), attn_anyd_kernel at head sizes 16,
32 and 128, attn_split_kernel on fp32 tensors and on split images of K and V - on unit-normal inputs, on "spotlight" inputs that
give single keys of the last two key tiles (and the first and last key of every tile) a visible share of a row while moving
the lazy reference maximum, and on "negative" inputs whose true scores all sit far below that of a zero-filled key.  The CPU
proof that this gate catches a dropped key, an admitted key S, exchanged V rows, a stale ring slot, a skipped rescale, a row sum
short of a tile, a truncating store and a clamped row: tests/test_attention_gate_host.py.

Every case: operands in NaN-poisoned memory with NaN between the token rows (negative-family cases: q and k | v as column slices
of fused, NaN-separated buffers), the output between guard margins, every element gated, bit-equal to ops.attention; the kernel
and grid the host's selection rule gives for the shape are asserted, so a shape that moves to another kernel fails.

Worst ratio to the budget on the MI355X beside the CPU emulation's (equal to three digits in every 16-bit group, bf16 / fp16):
    attn16v2    normal 0.554 / 0.459   spotlight 0.880 / 0.905   negative 0.283 / 0.228
    attn32i-3   normal 0.294 / 0.258   spotlight 0.894 / 0.789   negative 0.229 / 0.185
    attn32i-4   normal 0.378 / 0.321   spotlight 0.891 / 0.797   negative 0.223 / 0.206
    attn32i-7   normal 0.383 / 0.291   spotlight 0.893 / 0.765   negative 0.186 / 0.144
    attn32i-8   normal 0.376 / 0.339   spotlight 0.875 / 0.665   negative 0.157 / 0.116
    anyd 16 / 32 / 128: normal 0.39 / 0.43 / 0.40 (bf16), 0.36 / 0.34 / 0.33 (fp16); spotlight 0.85 - 0.89; negative 0.22 - 0.35
    fp32 (split operands, attn_split_kernel and attn_anyd_kernel): 0.03 and under, emulation 0.04 and under - the budget's fp32
    sums take their worst case S * 2^-24 where rounding errors of both signs add like sqrt(S)."""
import functools

import pytest
import torch

from stabletriton_amd import ops
from tests import edge_util as eu
from tests.test_edges_gpu import _dev, _name, _report

pytestmark = pytest.mark.gpu


def _id(v):
    if isinstance(v, tuple) and len(v) == 3 and isinstance(v[0], str):
        return f"{v[0]}-{_name(v[1])}-{v[2]}"
    return _name(v)


@functools.lru_cache(maxsize=2)
def _problem(family, shape, dtype):
    B, T, S, H, D = shape
    q, k, v, pairs = eu.attention_inputs(family, B, T, S, H, D)
    ref = eu.AttentionRef(q, k, v, H, D ** -0.5, dtype)
    spot = eu.assert_spotlight_condition(ref, pairs, S, H) if pairs is not None else None
    ref.p = None                                      # (B, H, T, S) float64: read above, not kept
    return q, k, v, ref, spot


def _fused(tensors, gpu, dtype):
    """Column slices of one NaN-filled (B, N, gap + C + gap + C ... + gap) buffer: strided rows, NaN columns on both sides."""
    B, N, C = tensors[0].shape
    gap = eu.ROW_GAP
    buf = torch.full((B, N, gap + len(tensors) * (C + gap)), float("nan"), dtype=dtype, device=gpu)
    views = []
    for i, t in enumerate(tensors):
        view = buf[..., gap + i * (C + gap):gap + i * (C + gap) + C]
        view.copy_(t.to(gpu, dtype))
        views.append(view)
    return views


def _operands(q, k, v, gpu, dtype, strided):
    if strided:
        return (*_fused((q,), gpu, dtype), *_fused((k, v), gpu, dtype))
    return tuple(_dev(t, gpu, dtype, row_gap=eu.ROW_GAP) for t in (q, k, v))


def _launch_and_gate(gpu, dtype, case):
    tag, shape, family = case
    B, T, S, H, D = shape
    kernel, targs, grid = eu.attention_kernel(dtype, B, T, S, H, D)
    assert (kernel, targs) == eu.ATT_EXPECTED[tag], f"{shape} takes {kernel}{targs}, the case is meant for {eu.ATT_EXPECTED[tag]}"
    q, k, v, ref, spot = _problem(family, shape, dtype)
    qg, kg, vg = _operands(q, k, v, gpu, dtype, strided=family == "negative")
    scale = D ** -0.5
    what = f"attention {tag} {shape} {family}"
    out, buf = eu.guarded((B, T, H * D), dtype, gpu)
    eu.attention_into(out, qg, kg, vg, H, scale)
    eu.assert_margins_intact(buf, what)
    ratio = ref.gate(out, what)
    _report(f"attention-{tag}-{family}", dtype, what + (f" (grid {grid}" + (f", lit keys hold >= {spot:.3f}" if spot is not None else "") + ")"), ratio)
    assert torch.equal(out, ops.attention(qg, kg, vg, H, scale)), f"{what}: ops.attention gives other bits"
    return out, ref, (qg, kg, vg), what


_HALF = [(d, c) for d in eu.ATT_HALF for c in eu.ATT_16BIT]
_ANYD = [(d, c) for d in eu.DTYPES for c in eu.ATT_ANYD]


@pytest.mark.parametrize("dtype,case", _HALF, ids=_id)
def test_head_size_64(gpu, dtype, case):
    """attn16v2_kernel (S < 256) and the four forms of attn32i_kernel, each at a ragged T (a last block with 1, 1, 65, 33 and
    255 live rows) and at key counts on both sides of every tile and ring boundary."""
    _launch_and_gate(gpu, dtype, case)


@pytest.mark.parametrize("dtype,case", _ANYD, ids=_id)
def test_other_head_sizes(gpu, dtype, case):
    """attn_anyd_kernel: one LDS buffer and two barriers per tile, head sizes 16 (half a contraction step), 32 and 128, in
    bf16, fp16 and on split fp32 operands; two batches, three heads, 33 rows (a third wave with one live row)."""
    _launch_and_gate(gpu, dtype, case)


@pytest.mark.parametrize("case", eu.ATT_F32, ids=_id)
def test_fp32_and_presplit(gpu, case):
    """attn_split_kernel<4, false> through st_attention, and <4, true> through st_attention_split on the split images of K and
    V that the project's own split op makes: the header of st_attention_split promises the same bits."""
    out, ref, (qg, kg, vg), what = _launch_and_gate(gpu, torch.float32, case)
    B, T, S, H, D = case[1]
    C = H * D
    images = [ops.split_rows(t.as_strided((B * S, C), (t.stride(1), 1))).s for t in (kg, vg)]
    pre, buf = eu.guarded((B, T, C), torch.float32, gpu)
    eu.attention_split_into(pre, qg, images[0], images[1], H, D ** -0.5)
    eu.assert_margins_intact(buf, what + " (pre-split)")
    _report(f"attention-presplit-{case[2]}", torch.float32, what + " (pre-split)", ref.gate(pre, what + " (pre-split)"))
    assert torch.equal(pre, out), f"{what}: st_attention_split and st_attention give different bits"
