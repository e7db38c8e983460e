"""GroupNorm, LayerNorm and the stand-alone GEGLU (csrc/norms.hip) gated per element against float64 (tests/edge_util.py:
group_norm_ref64, group_norm_from_stats_ref64, layer_norm_ref64, geglu_ref64 - the reference on the rounded operands, a budget
derived from the kernels' documented arithmetic): the three-launch GroupNorm in both layouts at one block and many, ragged
blocks, the block cap with more partials than gn_finalize has lanes, idle threads, cpg = 3 and 15, G = 1, G = C and one pixel;
GroupNorm from producer statistics the test writes itself (straddling groups, two sources of different tile heights, more
(channel, tile) pairs than threads) in its concatenated and its never-concatenated form; LayerNorm at every vector count; GEGLU
on strided halves, dense and mixed operands and just over the grid cap.  The CPU proof that this gate catches a neighbour's
rstd, dropped pixels, miscounted blocks, a Chan merge without its cross term, wrong channels, strides and tiles, a skipped
activation and a truncating store: tests/test_norm_gate_host.py.

Every case: operands (and partial buffers) in NaN-poisoned memory, the output between guard margins, every element gated, a
second launch bit-equal.

Worst ratio to the budget on the MI355X beside the CPU emulation's.  In bf16 and fp16 the two agree to three digits in every
group (the store's rounding uses nearly all of U_OUT |ref| at some element), bf16 / fp16:
    gn-nhwc     normal 0.996 / 0.996   offset 0.975 / 0.893   gradient 0.987 / 0.990   quiet 0.987 / 0.971
    gn-nchw     normal 0.987 / 0.991   offset 0.954 / 0.876   gradient 0.983 / 0.979   quiet 0.983 / 0.981
    from-stats  normal 0.996 / 0.995   quiet 0.975 / 0.981    (the cat form: the same figures, and the same bits)
    ln          normal 0.995 / 0.990   offset 0.991 / 0.972
    geglu       0.995 / 0.995
fp32, device / emulation (sums and merges round in another order on the device, and it contracts multiply-adds; both stay
under a third of the budget, whose statistics terms are worst cases):
    gn-nhwc     normal 0.134 / 0.167   offset 0.276 / 0.256   gradient 0.140 / 0.153   quiet 0.154 / 0.110
    gn-nchw     normal 0.118 / 0.118   offset 0.065 / 0.076   gradient 0.093 / 0.130   quiet 0.086 / 0.096
    from-stats  normal 0.149 / 0.168   quiet 0.106 / 0.131
    ln          normal 0.113 / 0.153   offset 0.067 / 0.081
    geglu       0.123 / 0.095   (gelu_erf_f's own 6.8e-7 against the emulation's exact function rounded to fp32)"""
import functools

import pytest
import torch

from stabletriton_amd import ops
from tests import edge_util as eu
from tests.test_edges_gpu import _dev, _name, _report

pytestmark = pytest.mark.gpu
EPS = eu.NORM_EPS
CL = torch.channels_last


def _id(v):
    if isinstance(v, tuple) and len(v) == 3 and isinstance(v[0], bool):
        return f"{'nhwc' if v[0] else 'nchw'}-{_name(v[1])}-{v[2]}"
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], str):
        return f"{_name(v[0])}-{v[1]}"
    return _name(v)


def _gate(out, ref, dtype, what, group):
    ratio = eu.assert_elementwise(out, ref[0], ref[1], 0, dtype, what, ref[2])
    _report(group, dtype, what, ratio)


def _twice(launch, shape, dtype, gpu, what, channels_last=False):
    """Two launches into guarded outputs: margins intact, bit-equal; returns the first output."""
    outs = []
    for _ in range(2):
        out, buf = eu.guarded(shape, dtype, gpu, channels_last=channels_last)
        launch(out)
        eu.assert_margins_intact(buf, what)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), f"{what}: two launches of the same problem differ"
    return outs[0]


# ================================================================================================ GroupNorm, three launches
_GN = [(d, c) for d in eu.DTYPES for c in eu.gn_cases(d)]


@pytest.mark.parametrize("dtype,case", _GN, ids=_id)
def test_group_norm(gpu, dtype, case):
    """st_group_norm with SiLU off and on; what each shape reaches is listed beside eu.GN_NHWC / eu.GN_NCHW and asserted by
    tests/test_norm_gate_host.py::test_case_labels."""
    nhwc, shape, family = case
    N, C, H, W, G = shape
    x, gamma, beta = eu.gn_operands(shape, family)
    xg, wg, bg = _dev(x, gpu, dtype, cl=nhwc), _dev(gamma, gpu, dtype), _dev(beta, gpu, dtype)
    for silu in (False, True):
        what = f"group_norm {'nhwc' if nhwc else 'nchw'} {shape} {family} silu={silu}"
        out = _twice(lambda o: eu.group_norm_into(o, xg, G, wg, bg, EPS, silu, nhwc), (N, C, H, W), dtype, gpu, what, channels_last=nhwc)
        _gate(out, eu.group_norm_ref64(x, gamma, beta, G, EPS, dtype, silu), dtype, what, f"gn-{'nhwc' if nhwc else 'nchw'}-{family}")


# ================================================================================================ GroupNorm from producer statistics
_GN_STATS = [(d, c) for d in eu.DTYPES for c in eu.GN_STATS]


@pytest.mark.parametrize("dtype,case", _GN_STATS, ids=lambda v: _name(v) if isinstance(v, torch.dtype) else f"{_name(v[0])}-{v[1]}")
def test_group_norm_from_stats(gpu, dtype, case):
    """gn_cols_finalize and the apply pass, isolated from any producer: the partials are the float64 sums of the stored values
    per tile row, rounded once to fp32 (eu.gn_partials), in poisoned buffers.  Two-source cases run on the concatenated tensor,
    on the two tensors (each poisoned on its own: a read past C0 in the first shows), and the two outputs are bit-equal."""
    (N, C0, C1, HW, G, rows0, rows1), family = case
    shape = eu.gn_stats_shape(case[0])
    C, H, W = shape[1], shape[2], shape[3]
    x, gamma, beta = eu.gn_operands(shape, family)
    xg, wg, bg = _dev(x, gpu, dtype, cl=True), _dev(gamma, gpu, dtype), _dev(beta, gpu, dtype)
    p0 = eu.poisoned(eu.gn_partials(xg[:, :C0], rows0).to(gpu))
    p1 = eu.poisoned(eu.gn_partials(xg[:, C0:], rows1).to(gpu)) if C1 else None
    halves = (_dev(x[:, :C0], gpu, dtype, cl=True), _dev(x[:, C0:], gpu, dtype, cl=True)) if C1 else None
    for silu in (False, True):
        what = f"group_norm_from_stats {case[0]} {family} silu={silu}"
        ref = eu.group_norm_from_stats_ref64(x, gamma, beta, G, EPS, dtype, silu)
        out = _twice(lambda o: eu.group_norm_from_stats_into(o, xg, G, wg, bg, EPS, silu, p0, C0, rows0, p1, C1, rows1),
                     (N, C, H, W), dtype, gpu, what, channels_last=True)
        _gate(out, ref, dtype, what, f"gn-from-stats-{family}")
        if C1:
            cat = _twice(lambda o: eu.group_norm_from_stats_cat_into(o, halves[0], halves[1], G, wg, bg, EPS, silu, p0, C0, rows0, p1, C1, rows1),
                         (N, C, H, W), dtype, gpu, what + " (cat)", channels_last=True)
            _gate(cat, ref, dtype, what + " (cat)", f"gn-from-stats-cat-{family}")
            assert torch.equal(cat, out), f"{what}: the two-tensor form and the concatenated form give different bits"


# ================================================================================================ LayerNorm
_LN = [(d, s, f) for d in eu.DTYPES for s in eu.ln_cases(d) for f in eu.LN_FAMILIES]


@pytest.mark.parametrize("dtype,shape,family", _LN, ids=_name)
def test_layer_norm(gpu, dtype, shape, family):
    """ln_kernel<T, 1> .. <T, 8> in every type, ragged and full last vector rows, row counts that leave idle waves."""
    x, gamma, beta = eu.ln_operands(shape, family)
    xg, wg, bg = _dev(x, gpu, dtype), _dev(gamma, gpu, dtype), _dev(beta, gpu, dtype)
    what = f"layer_norm {shape} {family} (NV = {eu.ln_vectors(dtype, shape[1])})"
    out = _twice(lambda o: eu.layer_norm_into(o, xg, wg, bg, EPS), shape, dtype, gpu, what)
    _gate(out, eu.layer_norm_ref64(x, gamma, beta, EPS, dtype), dtype, what, f"ln-{family}")


# ================================================================================================ GEGLU
@functools.lru_cache(maxsize=1)
def _geglu_problem(shape, dtype):
    s, g = eu.geglu_operands(shape)
    return s, g, eu.geglu_ref64(s, g, dtype)


def _geglu_views(s, g, gpu, dtype, layout):
    if layout == "dense":
        return _dev(s, gpu, dtype), _dev(g, gpu, dtype)
    Fh = s.shape[1]
    both = _dev(torch.cat([s, g], 1), gpu, dtype, row_gap=eu.ROW_GAP)
    return (_dev(s, gpu, dtype) if layout == "mixed" else both[:, :Fh]), both[:, Fh:]


_GEGLU = [(d, s, l) for d in eu.DTYPES for s, l in eu.geglu_cases(d)]


@pytest.mark.parametrize("dtype,shape,layout", _GEGLU, ids=_name)
def test_geglu(gpu, dtype, shape, layout):
    """st_geglu with gate arguments spanning [-7.5, 7.5]: the halves of one NaN-separated buffer, dense operands, a dense state
    beside a strided gate; the large shape has just over 4096 * 256 vectors, so some threads take a second grid-stride pass."""
    s, g, ref = _geglu_problem(shape, dtype)
    sg, gg = _geglu_views(s, g, gpu, dtype, layout)
    nvec, grid = eu.geglu_grid(dtype, *shape)
    what = f"geglu {shape} {layout} ({nvec} vectors, grid {grid})"
    out = _twice(lambda o: eu.geglu_into(o, sg, gg), shape, dtype, gpu, what)
    _gate(out, ref, dtype, what, "geglu")


# ================================================================================================ rejections
def test_rejections(gpu):
    """Shapes the entry points refuse: each comes back as a BackendError through _C.check, nothing is launched (the guarded
    outputs keep their fill)."""
    dtype = torch.bfloat16
    mk = lambda *shape, cl=False: _dev(eu.normal("n.rej", shape), gpu, dtype, cl=cl)

    def refused(match, shape, launch, channels_last=True):
        out, buf = eu.guarded(shape, dtype, gpu, channels_last=channels_last)
        with pytest.raises(ops.BackendError, match=match):
            launch(out)
        assert bool(torch.isnan(buf).all()), f"{match}: the refused call wrote to its output"

    w12, w16, w24 = mk(12), mk(16), mk(24)
    x12, x16, x24 = mk(1, 12, 2, 2, cl=True), mk(1, 16, 2, 3, cl=True), mk(1, 24, 2, 2, cl=True)
    part = lambda tiles, C: eu.poisoned(torch.zeros(tiles, C, 2, device=gpu))
    refused("multiple of 8", (1, 12, 2, 2), lambda o: eu.group_norm_into(o, x12, 3, w12, w12, EPS, False, True))            # NHWC, C % VEC != 0
    refused("rows per partial", (1, 16, 2, 3), lambda o: eu.group_norm_from_stats_into(o, x16, 2, w16, w16, EPS, False, part(2, 16), 16, 4))   # HW % rows != 0
    refused("sources cover", (1, 24, 2, 2), lambda o: eu.group_norm_from_stats_into(o, x24, 3, w24, w24, EPS, False, part(1, 8), 8, 4, part(1, 8), 8, 4))   # C0 + C1 != C
    xa, xb = mk(1, 12, 2, 2, cl=True), mk(1, 12, 2, 2, cl=True)
    refused("multiples of 8", (1, 24, 2, 2), lambda o: eu.group_norm_from_stats_cat_into(o, xa, xb, 3, w24, w24, EPS, False, part(1, 12), 12, 4, part(1, 12), 12, 4))   # C0 % VEC != 0
    wide = 8192                                                                                                   # nine vectors a lane and more
    refused("too wide", (2, wide), lambda o: eu.layer_norm_into(o, mk(2, wide), mk(wide), mk(wide), EPS), channels_last=False)
