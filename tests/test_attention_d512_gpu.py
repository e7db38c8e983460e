"""attn_d512_kernel (csrc/attention_d512.hip: head_dim 512, bf16 and fp16) behind ops.attention, gated per element against
float64 with tests/edge_util.py's AttentionRef - the reference on the values the kernels are documented to see and its derived
budget, as tests/test_attention_edges_gpu.py does for the other head sizes.

The kernel's constants: 64 query rows a block (two row halves of 32), 64 keys a tile, one K and one V buffer that every tile
reuses, channels split 256 | 256 between wave pairs.  The shapes (B, T, S, H):
    (2, 1, 9, 2)      T = 1 (one live row, the second row half all clamped), one tile with a short tail, head and batch offsets
    (1, 65, 65, 1)    exactly one tile and one key past it; a last block with one live row
    (1, 130, 200, 1)  four tiles (both buffers overwritten three times), a ragged last tile, T != S, three blocks
    (2, 33, 320, 2)   five whole tiles, two batches of two heads: offsets at a 1024-channel row, one live row in the second half
Every case: operands in NaN-poisoned memory with NaN between the token rows ("negative": q and k | v as column slices of fused,
NaN-separated buffers), the output between guard margins, every element gated, bit-equal to ops.attention.

Worst ratio to the budget on the MI355X (bf16 / fp16):
    normal 0.557 / 0.389   spotlight 0.929 / 0.808   negative 0.494 / 0.288
(the worst normal and negative figures are the T = 1, S = 9 case; the worst spotlight figure is (1, 65, 65, 1))."""
import functools

import pytest
import torch

from stabletriton_amd import ops
from tests import edge_util as eu

pytestmark = pytest.mark.gpu

D = 512
SHAPES = [(2, 1, 9, 2), (1, 65, 65, 1), (1, 130, 200, 1), (2, 33, 320, 2)]


@functools.lru_cache(maxsize=2)
def _problem(family, shape, dtype):
    B, T, S, H = shape
    q, k, v, pairs = eu.attention_inputs(family, B, T, S, H, D)
    ref = eu.AttentionRef(q, k, v, H, D ** -0.5, dtype)
    if pairs is not None:
        eu.assert_spotlight_condition(ref, pairs, S, H)
    ref.p = None                                      # (B, H, T, S) float64: read above, not kept
    return q, k, v, ref


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


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("family", eu.ATT_FAMILIES)
@pytest.mark.parametrize("dtype", eu.ATT_HALF, ids=lambda d: str(d).split(".")[-1])
def test_head_size_512(gpu, dtype, family, shape):
    B, T, S, H = shape
    q, k, v, ref = _problem(family, shape, dtype)
    if family == "negative":
        qg, kg, vg = (*_fused((q,), gpu, dtype), *_fused((k, v), gpu, dtype))
    else:
        qg, kg, vg = (eu.poisoned(t.to(gpu, dtype), row_gap=eu.ROW_GAP) for t in (q, k, v))
    what = f"attention d512 {shape} {family}"
    out, buf = eu.guarded((B, T, H * D), dtype, gpu)
    eu.attention_into(out, qg, kg, vg, H, D ** -0.5)
    eu.assert_margins_intact(buf, what)
    ratio = ref.gate(out, what)
    print(f"RATIO attention-d512-{family} {str(dtype).split('.')[-1]} {what}: {ratio:.3f} of the budget")
    assert torch.equal(out, ops.attention(qg, kg, vg, H, D ** -0.5)), f"{what}: ops.attention gives other bits"
