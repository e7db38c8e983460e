"""st_attention_joint / ops.attention_joint (csrc/attention_joint.hip): self-attention over two key/value sources under one softmax.

The kernel is attn32i_kernel with another address rule, so its contracts are bit contracts, checked with torch.equal:
  (a) gate on, b < lead: the bits of ops.attention on the contiguous concatenation of the two sources;
  (b) gate off, or b >= lead: the bits of ops.attention(q, k, v); k2 / v2 are never read (NaN-filled here).
Each source sits in its own NaN-poisoned buffer with NaN between the token rows, so a read of key S1 from the first source, or in
front of / behind the second, shows; the output sits between guard margins.  (B, T, H) are the smallest the lists of
tests/edge_util.py use for each of the four kernel forms; (S1, S2) put the source boundary on a tile edge, inside the low half and
inside the high half of a 64-key tile, with a one-key second source, and with the six-slot ring wrapping once and twice.
The float64 gate of tests/edge_util.py (AttentionRef) runs once per form on the concatenation, for the record."""
import functools

import pytest
import torch

from stabletriton_amd import _C, ops
from tests import edge_util as eu

pytestmark = pytest.mark.gpu


def _name(v):
    return str(v).split(".")[-1] if isinstance(v, torch.dtype) else None


def _report(group, dtype, what, ratio):
    print(f"RATIO {group} {_name(dtype)} {what}: {ratio:.3f} of the budget")


def _dev(t, gpu, dtype, row_gap=0):
    return eu.poisoned(t.to(gpu, dtype), row_gap=row_gap)


D = 64
FORMS = {"attn32i-3": (1, 97, 1), "attn32i-4": (1, 193, 90), "attn32i-7": (1, 257, 65), "attn32i-8": (1, 255, 130)}
SPLITS_3 = ((256, 1), (256, 64), (257, 63), (289, 32), (300, 21), (320, 65), (289, 160), (448, 1), (256, 513), (385, 384))
SPLITS_OTHER = ((257, 64), (289, 160), (385, 384))
ALL_FAMILIES_AT = (449, 769)
RECORD = {"attn32i-3": (289, 160), "attn32i-4": (257, 64), "attn32i-7": (257, 64), "attn32i-8": (257, 64)}      # the float64 gate runs here


def _cases():
    out = []
    for tag, splits in (("attn32i-3", SPLITS_3), ("attn32i-4", SPLITS_OTHER), ("attn32i-7", SPLITS_OTHER), ("attn32i-8", SPLITS_OTHER)):
        for s1, s2 in splits:
            for fam in eu.ATT_FAMILIES:
                if fam == "normal" or s1 + s2 in ALL_FAMILIES_AT:
                    out.append((tag, (s1, s2), fam))
    return out


def _id(v):
    if isinstance(v, tuple) and len(v) == 3 and isinstance(v[0], str):
        return f"{v[0]}-{v[1][0]}+{v[1][1]}-{v[2]}"
    return _name(v)


@functools.lru_cache(maxsize=4)
def _inputs(family, B, T, S, H):
    q, k, v, _ = eu.attention_inputs(family, B, T, S, H, D)
    return q, k, v


def joint_into(out, q, k, v, k2, v2, H, scale, lead, gate=None):
    """st_attention_joint into the caller's dense `out` (ops.attention_joint's argument plumbing)."""
    B, T, C = q.shape
    for t in (q, k, v):
        assert t.stride(2) == 1 and t.stride(0) == t.stride(1) * t.shape[1]
    B2 = k2.shape[0]
    step, table = gate if gate is not None else (None, None)
    _C.check(_C.load().st_attention_joint(q.data_ptr(), k.data_ptr(), v.data_ptr(), k2.data_ptr(), v2.data_ptr(), out.data_ptr(), B, T, k.shape[1],
                                          k2.shape[1], B2, lead, H, C // H, q.stride(1), k.stride(1), v.stride(1), k2.stride(1), v2.stride(1),
                                          k2.stride(0) if B2 > 1 else 0, v2.stride(0) if B2 > 1 else 0, C, float(scale),
                                          None if table is None else table.data_ptr(), None if step is None else step.data_ptr(),
                                          0 if table is None else table.numel(), _C.dtype_code(q.dtype), _C.stream_ptr()), "attention_joint")
    return out


def _sources(k, v, s1, gpu, dtype):
    """(k, v) of the concatenation, of the first and of the second source: every one in a NaN-poisoned buffer of its own."""
    dev = lambda t: _dev(t.contiguous(), gpu, dtype, row_gap=eu.ROW_GAP)
    return (dev(k), dev(v)), (dev(k[:, :s1]), dev(v[:, :s1])), (dev(k[:, s1:]), dev(v[:, s1:]))


@pytest.mark.parametrize("dtype", eu.ATT_HALF, ids=_name)
@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_joint_equals_attention_on_the_concatenation(gpu, dtype, case):
    tag, (s1, s2), family = case
    B, T, H = FORMS[tag]
    kernel, targs, grid = eu.attention_kernel(dtype, B, T, s1 + s2, H, D)
    assert (kernel, targs) == eu.ATT_EXPECTED[tag], f"{(B, T, H)} takes {kernel}{targs}, the case is meant for {eu.ATT_EXPECTED[tag]}"
    assert eu.attention_kernel(dtype, B, T, s1, H, D)[:2] == (kernel, targs)      # the gated-off launch: the same form
    q, k, v = _inputs(family, B, T, s1 + s2, H)
    scale = D ** -0.5
    qg = _dev(q, gpu, dtype, row_gap=eu.ROW_GAP)
    (kc, vc), (k1, v1), (k2, v2) = _sources(k, v, s1, gpu, dtype)
    what = f"attention_joint {tag} {(B, T, H)} {s1}+{s2} {family}"
    expect = ops.attention(qg, kc, vc, H, scale)
    assert bool(torch.isfinite(expect).all())
    out, buf = eu.guarded((B, T, H * D), dtype, gpu)
    joint_into(out, qg, k1, v1, k2, v2, H, scale, B)
    eu.assert_margins_intact(buf, what)
    assert torch.equal(out, expect), f"{what}: not the bits of ops.attention on the concatenation"
    assert torch.equal(ops.attention_joint(qg, k1, v1, k2, v2, H, scale), expect), f"{what}: ops.attention_joint gives other bits"
    assert torch.equal(ops.attention_joint(qg, k1, v1, k2, v2, H, scale, fused=False), expect), f"{what}: the slow path gives other bits"
    if family == "normal" and RECORD[tag] == (s1, s2):
        ref = eu.AttentionRef(q, k, v, H, scale, dtype)
        ref.p = None
        _report(f"attention-joint-{tag}", dtype, what + f" (grid {grid})", ref.gate(out, what))


def _batched(gpu, dtype, B, T, s1, s2, H, views):
    q, k, v = _inputs("normal", B, T, s1 + s2, H)
    qg = _dev(q, gpu, dtype, row_gap=eu.ROW_GAP)
    if views:      # self-attention layout: one buffer of B entries with s1 keys, the second source = its last entries
        assert s1 == s2
        k1, v1 = (_dev(t[:, :s1].contiguous(), gpu, dtype, row_gap=eu.ROW_GAP) for t in (k, v))
        return qg, k1, v1, None, None
    dev = lambda t: _dev(t.contiguous(), gpu, dtype, row_gap=eu.ROW_GAP)
    return qg, dev(k[:, :s1]), dev(v[:, :s1]), dev(k[:1, s1:]), dev(v[:1, s1:])


@pytest.mark.parametrize("dtype", eu.ATT_HALF, ids=_name)
@pytest.mark.parametrize("B,lead,B2", [(3, 2, 1), (6, 4, 2)])
def test_batch_mapping(gpu, dtype, B, lead, B2):
    """Entry b < lead attends to [k[b] ; k2[b % B2]], entries >= lead to k[b] alone (contract b); B2 = 2: k2 = k[lead:], views of the
    one buffer the UNet's fused projection leaves."""
    T, H, s1 = 97, 1, 289
    s2 = s1 if B2 == 2 else 160
    scale = D ** -0.5
    qg, k1, v1, k2, v2 = _batched(gpu, dtype, B, T, s1, s2, H, views=B2 == 2)
    if k2 is None:
        k2, v2 = k1[lead:], v1[lead:]
    assert k2.shape[0] == B2
    out, buf = eu.guarded((B, T, H * D), dtype, gpu)
    joint_into(out, qg, k1, v1, k2, v2, H, scale, lead)
    eu.assert_margins_intact(buf, f"attention_joint batch {B}/{lead}/{B2}")
    for b in range(B):
        if b < lead:
            r = b % B2
            kc = torch.cat([k1[b:b + 1], k2[r:r + 1]], dim=1)
            vc = torch.cat([v1[b:b + 1], v2[r:r + 1]], dim=1)
            want = ops.attention(qg[b:b + 1].contiguous(), kc, vc, H, scale)
        else:
            want = ops.attention(qg[b:b + 1].contiguous(), k1[b:b + 1].contiguous(), v1[b:b + 1].contiguous(), H, scale)
        assert torch.equal(out[b:b + 1], want), f"batch entry {b} of {B} (lead {lead}, B2 {B2})"
    assert torch.equal(out[lead:], ops.attention(qg, k1, v1, H, scale)[lead:])
    assert torch.equal(ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead), out)
    assert torch.equal(ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead, fused=False), out)


def _gate_problem(gpu, dtype, nan_second=False):
    B, T, H, s1, s2 = 3, 97, 1, 300, 21
    q, k, v = _inputs("normal", B, T, s1 + s2, H)
    dev = lambda t: _dev(t.contiguous(), gpu, dtype, row_gap=eu.ROW_GAP)
    qg, k1, v1, k2, v2 = dev(q), dev(k[:, :s1]), dev(v[:, :s1]), dev(k[:1, s1:]), dev(v[:1, s1:])
    if nan_second:
        k2.fill_(float("nan"))
        v2.fill_(float("nan"))
    return qg, k1, v1, k2, v2, H, D ** -0.5


@pytest.mark.parametrize("dtype", eu.ATT_HALF, ids=_name)
def test_gate_off_never_reads_the_second_source(gpu, dtype):
    qg, k1, v1, k2, v2, H, scale = _gate_problem(gpu, dtype, nan_second=True)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    table = torch.zeros(1, dtype=torch.float32, device=gpu)
    out, buf = eu.guarded(tuple(qg.shape), dtype, gpu)
    joint_into(out, qg, k1, v1, k2, v2, H, scale, 2, gate=(step, table))
    eu.assert_margins_intact(buf, "attention_joint gate off")
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, ops.attention(qg, k1, v1, H, scale))
    assert torch.equal(ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=2, gate=(step, table)), out)


@pytest.mark.parametrize("dtype", eu.ATT_HALF, ids=_name)
def test_gate_is_read_at_every_replay_and_clamps(gpu, dtype):
    qg, k1, v1, k2, v2, H, scale = _gate_problem(gpu, dtype)
    lead = 2
    off = ops.attention(qg, k1, v1, H, scale)
    on = ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead)
    assert not torch.equal(on[:lead], off[:lead]) and torch.equal(on[lead:], off[lead:])
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    table = torch.zeros(2, dtype=torch.float32, device=gpu)
    ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead, gate=(step, table))      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead, gate=(step, table))
    graph.replay()
    assert torch.equal(out, off)
    table[0] = 1.0
    graph.replay()
    assert torch.equal(out, on), "the captured launch did not follow the table"
    step.fill_(1)                    # entry 1 is 0
    graph.replay()
    assert torch.equal(out, off), "the captured launch did not follow the step counter"
    table[1] = 1.0
    table[0] = 0.0
    step.fill_(7)                    # beyond the table: clamps to the last entry (1)
    graph.replay()
    assert torch.equal(out, on)
    step.fill_(-3)                   # clamps to entry 0 (0)
    graph.replay()
    assert torch.equal(out, off)


SLOW = [("fp32", torch.float32, 2, 64, 300), ("d32", torch.bfloat16, 4, 32, 300), ("short", torch.bfloat16, 2, 64, 64), ("short-f16", torch.float16, 2, 64, 64)]


@pytest.mark.parametrize("tag,dtype,H,Dh,s1", SLOW, ids=[c[0] for c in SLOW])
def test_slow_path(gpu, tag, dtype, H, Dh, s1):
    """fp32 (strict mode), another head size and a short first source: torch.cat + ops.attention, within AttentionRef's per-dtype
    budget of the float64 statement on the concatenation; the device gate is honoured by a torch.where."""
    B, T, s2, lead = 3, 33, 21, 2
    q, k, v, _ = eu.attention_inputs("normal", B, T, s1 + s2, H, Dh)
    scale = Dh ** -0.5
    dev = lambda t: t.to(gpu, dtype).contiguous()
    qg, k1, v1, k2, v2 = dev(q), dev(k[:, :s1]), dev(v[:, :s1]), dev(k[:1, s1:]), dev(v[:1, s1:])
    with pytest.raises(ops.BackendError, match="attention_joint"):
        ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead, fused=True)
    out = ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead)
    kc = torch.cat([k[:lead, :s1], k[:1, s1:].expand(lead, -1, -1)], dim=1)
    vc = torch.cat([v[:lead, :s1], v[:1, s1:].expand(lead, -1, -1)], dim=1)
    what = f"attention_joint slow path {tag}"
    _report(f"attention-joint-slow-{tag}", dtype, what + " (lead)", eu.AttentionRef(q[:lead], kc, vc, H, scale, dtype).gate(out[:lead], what))
    _report(f"attention-joint-slow-{tag}", dtype, what + " (rest)",
            eu.AttentionRef(q[lead:], k[lead:, :s1], v[lead:, :s1], H, scale, dtype).gate(out[lead:], what))
    plain = ops.attention(qg, k1, v1, H, scale)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    table = torch.tensor([0.0, 1.0], dtype=torch.float32, device=gpu)
    assert torch.equal(ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead, gate=(step, table)), plain)
    step.fill_(1)
    assert torch.equal(ops.attention_joint(qg, k1, v1, k2, v2, H, scale, lead=lead, gate=(step, table)), out)


def test_kernel_refuses_what_the_slow_path_takes(gpu):
    lib = _C.load()
    x = torch.zeros(1, 256, 64, dtype=torch.bfloat16, device=gpu)
    p = x.data_ptr()
    args = lambda S1, Dh, dt: (p, p, p, p, p, p, 1, 256, S1, 256, 1, 1, 1, Dh, 64, 64, 64, 64, 64, 0, 0, 64, 0.125, None, None, 0, dt, None)
    for S1, Dh, dt, word in ((255, 64, _C.ST_BF16, b"S1"), (256, 32, _C.ST_BF16, b"head_dim"), (256, 64, _C.ST_F32, b"16-bit")):
        assert lib.st_attention_joint(*args(S1, Dh, dt)) != 0 and word in lib.st_last_error()
