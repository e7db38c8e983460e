"""CPU proof that the per-element gate of tests/edge_util.py on GroupNorm, LayerNorm and GEGLU (group_norm_ref64,
group_norm_from_stats_ref64, layer_norm_ref64, geglu_ref64) bites: a torch fp32 emulation of csrc/norms.hip in the kernels'
own order -
  gn_stats_nhwc    per-thread sums over pixels p0 + rp, p0 + rp + RP, ..., then over rp in order, then over the cpg channels,
                   mean = S / cnt and m2 = max(SS - S * mean, 0) with cnt = (p1 - p0) * cpg;
  gn_stats_nchw    256 strided partial sums per chunk, the wave tree, the four-wave add;
  gn_finalize      each lane folds partials lane, lane + 64, ... with chan_merge, then the ordered butterfly, rsqrt;
  gn_cols_finalize float64 sums of fp32 partials, one rounding of (mean, rstd);
  the apply pass   a = rstd * gamma, (x - mean) * a + beta, SiLU, one rounding to the stored type;
  ln_kernel        per-lane sums over its vectors, the wave tree, the two-pass variance; geglu_kernel with the float32
                   restatement of the 16-bit GELU (tests/test_edge_gate_host.py) / the exact function rounded to fp32 -
passes the gate at every case, type and family tests/test_norm_edges_gpu.py launches, and every mutation a kernel bug would
amount to fails it.  The four measured constants of the budget are measured here.  (The emulation multiplies and adds
separately where the compiler may contract to an FMA: one rounding fewer on the device, inside the same bounds.)
No GPU, no operator library."""
import functools

import numpy as np
import pytest
import torch

from tests import edge_util as eu
from tests.test_edge_gate_host import _gelu_fast_f32, _truncate

HALF = [torch.bfloat16, torch.float16]
EPS = eu.NORM_EPS
EPS32 = torch.tensor(EPS, dtype=torch.float32)


def _name(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, (tuple, list)):
        return "-".join(_name(e) or str(e) for e in v)
    return None


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
def _seq_sum(t, dim):
    """fp32 sum along `dim` in index order, from 0.f."""
    acc = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        acc = acc + t.select(dim, i)
    return acc


def _wave_tree(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1 over the last axis of 64 lanes."""
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    return v[..., 0]


def emu_stats_nhwc(xr, G, dtype, mutation=None):
    """gn_stats_nhwc on the fp32 values xr (N, C, H, W): partials (N, NB, G, 3) = (mean, m2, cnt)."""
    N, C = xr.shape[:2]
    v = xr.reshape(N, C, -1).transpose(1, 2)                      # (N, HW, C)
    HW = v.shape[1]
    VC, RP, NB, P = eu.gn_geometry_nhwc(dtype, C, HW)
    K = -(-P // RP)
    blk = torch.zeros(N, NB, K * RP, C)                            # pixels a block does not have add 0.f: exact
    cnt = torch.zeros(NB)
    for b in range(NB):
        p0, p1 = b * P, min(b * P + P, HW)
        live = p1 - p0 - (1 if mutation == "drop_last_pixel" else 0)
        blk[:, b, :live] = v[:, p0:p0 + live]
        cnt[b] = (P if mutation == "count_P" else p1 - p0) * (C // G)
    blk = blk.view(N, NB, K, RP, C)
    s, ss = _seq_sum(blk, 2), _seq_sum(blk * blk, 2)              # a thread's passes
    s, ss = _seq_sum(s, 2), _seq_sum(ss, 2)                       # over rp, in order
    S, SS = _seq_sum(s.view(N, NB, G, C // G), 3), _seq_sum(ss.view(N, NB, G, C // G), 3)
    cnt = cnt.view(1, NB, 1).expand(N, NB, G)
    mean = S / cnt
    return torch.stack([mean, (SS - S * mean).clamp_min(0.0), cnt], -1)


def emu_stats_nchw(xr, G, mutation=None):
    N, C = xr.shape[:2]
    HW = xr[0, 0].numel()
    NB, chunk, _ = eu.gn_geometry_nchw(N, C, HW, G)
    total = (C // G) * HW
    runs = xr.reshape(N, G, total)
    parts = []
    for b in range(NB):
        i0, i1 = b * chunk, min(b * chunk + chunk, total)
        if mutation == "chunk_short":
            i1 -= 1
        n = i1 - i0
        seg = torch.zeros(N, G, -(-n // 256) * 256)
        seg[..., :n] = runs[..., i0:i1]
        seg = seg.view(N, G, -1, 256)
        s, ss = _seq_sum(seg, 2), _seq_sum(seg * seg, 2)
        s, ss = _wave_tree(s.view(N, G, 4, 64)), _wave_tree(ss.view(N, G, 4, 64))
        S, SS = _seq_sum(s, 2), _seq_sum(ss, 2)
        mean = S / n
        parts.append(torch.stack([mean, (SS - S * mean).clamp_min(0.0), torch.full_like(S, float(n))], -1))
    return torch.stack(parts, 1)


def _merge(a, b, mutation=None):
    """chan_merge(a <- b) on tuples (mean, m2, cnt)."""
    (mean, m2, cnt), (pm, p2, pc) = a, b
    live = pc > 0
    tot = cnt + pc
    d = pm - mean
    w = pc / torch.where(live, tot, torch.ones_like(tot))
    cross = torch.zeros_like(d) if mutation == "no_cross_term" else d * d * (cnt * w)
    return torch.where(live, mean + d * w, mean), torch.where(live, m2 + (p2 + cross), m2), torch.where(live, tot, cnt)


def emu_finalize(part, mutation=None):
    """gn_finalize on partials (N, NB, G, 3): (mean, rstd) as (N, G) fp32."""
    N, NB, G, _ = part.shape
    rounds = 1 if mutation == "first_64_partials" else -(-NB // 64)
    lanes = torch.zeros(N, rounds * 64, G, 3)
    lanes[:, :min(NB, rounds * 64)] = part[:, :rounds * 64]
    lanes = lanes.view(N, rounds, 64, G, 3)
    acc = tuple(torch.zeros(N, 64, G) for _ in range(3))
    for r in range(rounds):
        acc = _merge(acc, tuple(lanes[:, r, :, :, i] for i in range(3)), mutation)
    while acc[0].shape[1] > 1:                                     # lanes l and l ^ o, the lower one first
        acc = _merge(tuple(t[:, 0::2] for t in acc), tuple(t[:, 1::2] for t in acc), mutation)
    mean, m2, cnt = (t[:, 0] for t in acc)
    var = m2 / (cnt - 1.0 if mutation == "n_minus_1" else cnt)
    return mean, torch.rsqrt(var if mutation == "no_eps" else var + EPS32)


def emu_cols_finalize(p0, C0, tiles0, p1, C1, tiles1, N, G, cpg, HW, mutation=None):
    """gn_cols_finalize: p0 / p1 the partials as flat (pairs, 2) fp32 tensors (p1 None: one source).  An index a mutation
    sends past a buffer wraps round (the GPU test would read poison there)."""
    if mutation == "tiles0_for_source1":
        tiles1 = tiles0

    def sweep(flat, Cs, tiles, n, lo, hi):
        w = hi - lo
        if w <= 0 or flat is None:
            return 0.0, 0.0
        base = (0 if mutation == "no_image_offset" else n * tiles * Cs) + lo
        k = torch.arange(w * tiles)
        idx = (base + (k // w) * Cs + k % w) % flat.shape[0]
        return float(flat[idx, 0].double().sum()), float(flat[idx, 1].double().sum())

    mean, rstd = torch.zeros(N, G), torch.zeros(N, G)
    for n in range(N):
        for g in range(G):
            c_lo, c_hi = g * cpg, g * cpg + cpg
            S, Q = sweep(p0, C0, tiles0, n, min(c_lo, C0), min(c_hi, C0))
            off = 0 if mutation == "no_c0_subtract" else C0
            if not (mutation == "skip_straddle" and c_lo < C0 < c_hi):
                S1, Q1 = sweep(p1, C1, tiles1, n, max(c_lo, C0) - off, max(c_hi, C0) - off)
                S, Q = S + S1, Q + Q1
            m = S / (cpg * HW)
            var = max(Q / (cpg * HW) - m * m, 0.0)
            mean[n, g], rstd[n, g] = m, 1.0 / (var + float(EPS32)) ** 0.5         # stored as fp32: one rounding each
    return mean, rstd


def _silu32(f):
    return f / (1.0 + torch.exp(-f))


def emu_apply(xr, gr, br, mean, rstd, G, dtype, silu, mutation=None):
    """gn_apply_nhwc / gn_apply_nchw: the same arithmetic per element."""
    N, C = xr.shape[:2]
    ch = torch.arange(C)
    if mutation == "vector_group":                                  # every channel of a 16-byte vector takes its first channel's group
        ch = ch // eu.vec_of(dtype) * eu.vec_of(dtype)
    grp = ch // (C // G)
    if mutation == "neighbour_rstd":
        rstd = rstd.roll(1, 1)
    if mutation == "gamma_shift":
        gr = gr.roll(1)
    if mutation == "beta_shift":
        br = br.roll(1)
    a = rstd[:, grp].view(N, C, 1, 1) * gr.view(1, C, 1, 1)
    f = (xr - mean[:, grp].view(N, C, 1, 1)) * a + br.view(1, C, 1, 1)
    if silu and mutation != "no_silu":
        f = _silu32(f)
    return _truncate(f, dtype) if mutation == "truncate" else f.to(dtype)


def _rounded(dtype, *ts):
    return tuple(t.to(dtype).float() for t in ts)


def emu_group_norm(x, gamma, beta, G, dtype, nhwc, silu, mutation=None, stats=False):
    xr, gr, br = _rounded(dtype, x, gamma, beta)
    part = emu_stats_nhwc(xr, G, dtype, mutation) if nhwc else emu_stats_nchw(xr, G, mutation)
    mean, rstd = emu_finalize(part, mutation)
    if stats:
        return mean, rstd, part
    return emu_apply(xr, gr, br, mean, rstd, G, dtype, silu, mutation)


def _sources(x, case, dtype):
    """The stored halves of a from-statistics case and their partials as flat (pairs, 2) tensors."""
    N, C0, C1, HW, G, rows0, rows1 = case
    st = x.to(dtype)
    p0 = eu.gn_partials(st[:, :C0], rows0).view(-1, 2)
    p1 = eu.gn_partials(st[:, C0:], rows1).view(-1, 2) if C1 else None
    return p0, p1


def emu_group_norm_from_stats(x, gamma, beta, case, dtype, silu, mutation=None, cat=False):
    N, C0, C1, HW, G, rows0, rows1 = case
    C = C0 + C1
    xr, gr, br = _rounded(dtype, x, gamma, beta)
    p0, p1 = _sources(x, case, dtype)
    mean, rstd = emu_cols_finalize(p0, C0, HW // rows0, p1, C1, HW // rows1 if C1 else 0, N, G, C // G, HW, mutation)
    if cat and mutation == "cat_stride_C":                         # source 1 read with the pixel stride of the whole tensor
        flat = xr[:, C0:].reshape(N, C1, HW).transpose(1, 2).reshape(-1)         # x1 as it lies in memory: (n, p, c)
        n, p, c = torch.meshgrid(torch.arange(N), torch.arange(HW), torch.arange(C1), indexing="ij")
        x1 = flat[(n * HW * C + p * C + c) % flat.numel()]                             # (N, HW, C1)
        xr = torch.cat([xr[:, :C0], x1.transpose(1, 2).reshape(N, C1, *xr.shape[2:])], 1)
    return emu_apply(xr, gr, br, mean, rstd, G, dtype, silu, mutation)


def emu_layer_norm(x, gamma, beta, dtype, mutation=None, stats=False):
    xr, gr, br = _rounded(dtype, x, gamma, beta)
    rows, C = xr.shape
    vec, NV = eu.vec_of(dtype), eu.ln_vectors(dtype, C)
    VC = C // vec
    live_vc = VC - 1 if mutation == "drop_last_vector" else VC
    pad = torch.zeros(rows, 64 * NV * vec)
    pad[:, :live_vc * vec] = xr[:, :live_vc * vec]
    live = torch.zeros(64 * NV * vec, dtype=torch.bool)
    live[:live_vc * vec] = True
    lanes = lambda t: t.view(-1, NV, 64, vec).permute(0, 2, 1, 3).reshape(-1, 64, NV * vec)   # a lane's values in its own order
    denom = float(64 * NV * vec) if mutation == "mean_over_padded" else float(C)
    mean = _wave_tree(_seq_sum(lanes(pad), 2)) / denom
    if mutation == "one_pass":
        var = _wave_tree(_seq_sum(lanes(pad * pad), 2)) / denom - mean * mean
    else:
        d = torch.where(live, pad - mean[:, None], torch.zeros(()))
        var = _wave_tree(_seq_sum(lanes(d * d), 2)) / denom
    rstd = torch.rsqrt(var + EPS32)
    if stats:
        return mean, var
    return ((xr - mean[:, None]) * rstd[:, None] * gr + br).to(dtype)


def _gelu32(g32, dtype, tanh=False):
    if tanh:
        return (0.5 * g32 * (1.0 + torch.tanh(0.7978845608028654 * (g32 + 0.044715 * g32 * g32 * g32)))).float()
    if dtype == torch.float32:
        return eu.gelu64(g32.double()).float()                     # gelu_erf_f: within 6.8e-7 of the exact function
    return torch.from_numpy(_gelu_fast_f32(g32.numpy().astype(np.float64)))


def _geglu_buffers(state, gate, dtype, layout):
    """(state view, gate view) in the layout's memory, on the CPU: the gaps hold 1.0 where the GPU test holds NaN."""
    rows, Fh = state.shape
    s, g = state.to(dtype), gate.to(dtype)
    if layout == "dense":
        return s, g
    buf = torch.ones(rows, 2 * Fh + eu.ROW_GAP, dtype=dtype)
    buf[:, :Fh], buf[:, Fh:2 * Fh] = s, g
    return (s if layout == "mixed" else buf[:, :Fh]), buf[:, Fh:2 * Fh]


def emu_geglu(state, gate, dtype, layout="dense", mutation=None):
    rows, Fh = state.shape
    sv, gv = _geglu_buffers(state, gate, dtype, layout)
    if mutation == "swap":
        sv, gv = gv, sv
    if mutation == "gate_at_state_stride":
        flat = gv.as_strided((gv.untyped_storage().nbytes() // gv.element_size() - gv.storage_offset(),), (1,), gv.storage_offset())
        r, c = torch.meshgrid(torch.arange(rows), torch.arange(Fh), indexing="ij")
        gv = flat[(r * sv.stride(0) + c) % flat.numel()]
    out = (sv.float() * _gelu32(gv.float().contiguous(), dtype, tanh=mutation == "tanh_gelu")).to(dtype)
    if mutation == "no_second_pass":                                # vectors 4096 * 256 .. are never stored
        nvec, grid = eu.geglu_grid(dtype, rows, Fh)
        out.view(-1)[grid * 256 * eu.vec_of(dtype):] = 0
    return out


# ------------------------------------------------------------------------------------------------ cached problems
@functools.lru_cache(maxsize=4)
def _gn_problem(shape, family, dtype, silu, from_stats=False):
    x, gamma, beta = eu.gn_operands(shape, family)
    ref = (eu.group_norm_from_stats_ref64 if from_stats else eu.group_norm_ref64)(x, gamma, beta, shape[4], EPS, dtype, silu)
    return (x, gamma, beta), ref


def _gate(out, ref, dtype, what):
    return eu.assert_elementwise(out, ref[0], ref[1], 0, dtype, what, ref[2])


def _fails(out, ref, dtype, what):
    with pytest.raises(AssertionError, match="x its budget"):
        _gate(out, ref, dtype, what)


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_emulation_passes_at_every_gpu_case(dtype):
    """Every case of tests/test_norm_edges_gpu.py in this type: the emulation is inside the budget; the worst ratio per group is
    printed (the GPU file's docstring records them beside the device's)."""
    worst = {}

    def note(group, ratio):
        worst[group] = max(worst.get(group, 0.0), ratio)

    for nhwc, shape, family in eu.gn_cases(dtype):
        for silu in (False, True):
            (x, gamma, beta), ref = _gn_problem(shape, family, dtype, silu)
            out = emu_group_norm(x, gamma, beta, shape[4], dtype, nhwc, silu)
            note(f"gn-{'nhwc' if nhwc else 'nchw'}-{family}", _gate(out, ref, dtype, f"emulated group_norm {shape} {family} nhwc={nhwc} silu={silu}"))
    for case, family in eu.GN_STATS:
        shape = eu.gn_stats_shape(case)
        for silu in (False, True):
            (x, gamma, beta), ref = _gn_problem(shape, family, dtype, silu, True)
            out = emu_group_norm_from_stats(x, gamma, beta, case, dtype, silu)
            note(f"gn-from-stats-{family}", _gate(out, ref, dtype, f"emulated group_norm_from_stats {case} {family} silu={silu}"))
    for shape in eu.ln_cases(dtype):
        for family in eu.LN_FAMILIES:
            x, gamma, beta = eu.ln_operands(shape, family)
            note(f"ln-{family}", _gate(emu_layer_norm(x, gamma, beta, dtype), eu.layer_norm_ref64(x, gamma, beta, EPS, dtype), dtype,
                                       f"emulated layer_norm {shape} {family}"))
    for shape, layout in eu.geglu_cases(dtype):
        s, g = eu.geglu_operands(shape)
        note("geglu", _gate(emu_geglu(s, g, dtype, layout), eu.geglu_ref64(s, g, dtype), dtype, f"emulated geglu {shape} {layout}"))
    for group, ratio in worst.items():
        print(f"EMULATION RATIO {group} {_name(dtype)}: {ratio:.3f} of the budget")


def test_measured_constants():
    """The four measured constants.  Over every three-launch GroupNorm case, layout, family and type: |mean - mu| in units of
    U_ACC * mean|x|, and what the variance m2 / cnt is off by beyond the mean's share 2 |mu| |mean - mu|, in units of
    U_ACC * q.  Over every LayerNorm case: the same for the mean, the variance in units of U_ACC * var.  edge_util's constants
    cover what is measured and are at most twice it."""
    gm = gv = lm = lv = 0.0
    for dtype in eu.DTYPES:
        for nhwc, shape, family in eu.gn_cases(dtype):
            x, gamma, beta = eu.gn_operands(shape, family)
            N, G = shape[0], shape[4]
            mean, _, part = emu_group_norm(x, gamma, beta, G, dtype, nhwc, False, stats=True)
            m2, cnt = emu_finalize_m2(part)
            xg = eu.r64(x, dtype).reshape(N, G, -1)
            mu, q, m1 = xg.mean(-1), (xg * xg).mean(-1), xg.abs().mean(-1)
            var = ((xg - mu[..., None]) ** 2).mean(-1)
            e_mean = (mean.double() - mu).abs()
            e_var = (((m2 / cnt).double() - var).abs() - 2.0 * mu.abs() * e_mean).clamp_min(0.0)
            gm, gv = max(gm, float((e_mean / (eu.U_ACC * m1)).max())), max(gv, float((e_var / (eu.U_ACC * q)).max()))
        for shape in eu.ln_cases(dtype):
            for family in eu.LN_FAMILIES:
                x, gamma, beta = eu.ln_operands(shape, family)
                mean, var32 = emu_layer_norm(x, gamma, beta, dtype, stats=True)
                xd = eu.r64(x, dtype)
                mu, m1 = xd.mean(-1), xd.abs().mean(-1)
                var = ((xd - mu[:, None]) ** 2).mean(-1)
                e_mean = (mean.double() - mu).abs()
                e_var = ((var32.double() - var).abs() - e_mean * e_mean).clamp_min(0.0)
                lm, lv = max(lm, float((e_mean / (eu.U_ACC * m1)).max())), max(lv, float((e_var / (eu.U_ACC * var)).max()))
    print(f"EMULATION statistics: GroupNorm mean off by {gm:.2f} U_ACC mean|x| at most, variance by {gv:.2f} U_ACC q beyond the "
          f"mean's share; LayerNorm mean {lm:.2f} U_ACC mean|x|, variance {lv:.2f} U_ACC var")
    assert gm <= eu.GN_MEAN_ULPS <= 2.0 * gm
    assert gv <= eu.GN_VAR_ULPS <= 2.0 * gv
    assert lm <= eu.LNK_MEAN_ULPS <= 2.0 * lm
    assert lv <= eu.LNK_VAR_ULPS <= 2.0 * lv


def emu_finalize_m2(part):
    """(m2, cnt) of the merged partials, as gn_finalize has them in front of the rsqrt."""
    N, NB, G, _ = part.shape
    rounds = -(-NB // 64)
    lanes = torch.zeros(N, rounds * 64, G, 3)
    lanes[:, :NB] = part
    lanes = lanes.view(N, rounds, 64, G, 3)
    acc = tuple(torch.zeros(N, 64, G) for _ in range(3))
    for r in range(rounds):
        acc = _merge(acc, tuple(lanes[:, r, :, :, i] for i in range(3)))
    while acc[0].shape[1] > 1:
        acc = _merge(tuple(t[:, 0::2] for t in acc), tuple(t[:, 1::2] for t in acc))
    return acc[1][:, 0], acc[2][:, 0]


def test_case_labels():
    """The restated geometry of every case has the property the case is listed for."""
    for dtype in eu.DTYPES:
        vec = eu.vec_of(dtype)
        geo = [eu.gn_geometry_nhwc(dtype, s[1], s[2] * s[3]) for s in eu.gn_nhwc_shapes(dtype)]
        shapes = eu.gn_nhwc_shapes(dtype)
        assert all(s[1] % vec == 0 and s[1] % s[4] == 0 for s in shapes)
        VC, RP, NB, P = geo[0]                                      # cpg = 3, idle threads, one block
        assert shapes[0][1] // shapes[0][4] == 3 and RP * VC < eu.GN_THREADS and NB == 1
        assert shapes[1][0] * shapes[1][4] == 9                      # gn_finalize: 4 + 4 + 1 waves
        VC, RP, NB, P = geo[2]                                      # several blocks; 16 bits: the last one ragged
        assert (NB, P) == ((7, 11) if dtype == torch.float32 else (4, 20)) and (dtype == torch.float32 or 77 % P != 0)
        assert shapes[3][1] // shapes[3][4] == 15
        VC, RP, NB, P = geo[4]                                      # the block cap
        HW = shapes[4][2] * shapes[4][3]
        assert (VC, RP, NB, P) == (320, 3, 225, 4) and P > RP and NB > 64 and HW % P != 0 and RP * VC < eu.GN_THREADS
        assert -(-HW // RP) > eu.GN_MAX_BLOCKS and 3 <= NB // 64 and -(-NB // 64) == 4
        assert shapes[5][4] == 1 and shapes[6][2] * shapes[6][3] == 1 and shapes[7][4] == shapes[7][1]
    (N, C, H, W, G) = eu.GN_NCHW[0]
    NB, chunk, bx = eu.gn_geometry_nchw(N, C, H * W, G)
    assert NB == 2 and chunk % 256 != 0 and bx == 3
    (N, C, H, W, G) = eu.GN_NCHW[1]
    assert eu.gn_geometry_nchw(N, C, H * W, G)[0] == 1
    assert eu.GN_NCHW[2][0] * eu.GN_NCHW[2][4] == 9 and eu.GN_NCHW[3][2] * eu.GN_NCHW[3][3] == 1
    # from statistics: straddling groups, pairs per group against the 256 threads, tile heights
    (N, C0, C1, HW, G, r0, r1), _ = eu.GN_STATS[0]
    cpg = (C0 + C1) // G
    assert cpg == 15 and C0 % cpg != 0 and (HW // r0, HW // r1) == (3, 2) and N == 2
    (N, C0, C1, HW, G, r0, r1), _ = eu.GN_STATS[1]
    cpg = (C0 + C1) // G
    assert cpg == 60 and C0 // cpg == 21 and C0 % cpg != 0 and cpg * (HW // r0) == 480 > 256 and cpg * (HW // r1) == 240 and r0 != r1
    assert cpg % 8 != 0 and cpg % 4 == 0                            # a 16-bit vector straddles two groups, an fp32 one does not
    (N, C0, C1, HW, G, r0, r1), _ = eu.GN_STATS[2]
    assert C1 == 0 and HW // r0 == 1
    assert eu.GN_STATS[3][1] == "quiet" and all(c[1] % 8 == 0 and c[2] % 8 == 0 for c, _ in eu.GN_STATS)
    for dtype in eu.DTYPES:
        cases = eu.ln_cases(dtype)
        assert {eu.ln_vectors(dtype, C) for _, C in cases} == set(range(1, 9))
        assert all(C % eu.vec_of(dtype) == 0 for _, C in cases) and any(r % 4 for r, _ in cases)
        assert any(64 * eu.ln_vectors(dtype, C) * eu.vec_of(dtype) != C for _, C in cases)
        assert eu.ln_vectors(dtype, 4096 if dtype == torch.float32 else 8192) > 8            # what the rejection test sends
        rows, Fh = eu.GEGLU_STRIDE2[dtype]
        nvec, grid = eu.geglu_grid(dtype, rows, Fh)
        assert nvec > 4096 * 256 and grid == 4096 and nvec < 2 * 4096 * 256
        assert all(eu.geglu_grid(dtype, r, f)[0] <= 4096 * 256 for r, f in eu.GEGLU_SMALL) and any(r % 4 for r, _ in eu.GEGLU_SMALL)
    assert eu.GEGLU_GATE_SPAN < eu.ACT_RANGE


# ------------------------------------------------------------------------------------------------ every mutation fails
def _gn_mutation(dtype, nhwc, shape, family, mutation, silu=True):
    (x, gamma, beta), ref = _gn_problem(shape, family, dtype, silu)
    _fails(emu_group_norm(x, gamma, beta, shape[4], dtype, nhwc, silu, mutation), ref, dtype, f"{mutation} {shape} {family}")


def _ragged_nhwc(dtype):
    """The smallest NHWC case whose last block is ragged in this type."""
    for s in sorted(eu.gn_nhwc_shapes(dtype), key=lambda s: s[1] * s[2] * s[3]):
        _, _, NB, P = eu.gn_geometry_nhwc(dtype, s[1], s[2] * s[3])
        if NB > 1 and (s[2] * s[3]) % P:
            return s
    raise AssertionError("no ragged NHWC case")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_neighbour_rstd_fails(dtype):
    """A group takes its neighbour's rstd: at groups of 105 values (rstd differs by several percent between neighbours) and
    at the block-cap case's groups of 35,960 / 71,920 values, where neighbours differ by a few tenths of a percent - less than
    a bf16 store rounds away at most elements, so only the elements whose reference is near zero give it away."""
    _gn_mutation(dtype, True, eu.gn_nhwc_shapes(dtype)[0], "normal", "neighbour_rstd")
    _gn_mutation(dtype, True, eu.gn_nhwc_shapes(dtype)[4], "normal", "neighbour_rstd")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_block_drops_its_last_pixel_fails(dtype):
    for shape in (eu.gn_nhwc_shapes(dtype)[0], eu.gn_nhwc_shapes(dtype)[2]):
        _gn_mutation(dtype, True, shape, "normal", "drop_last_pixel")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_ragged_block_counting_P_fails(dtype):
    """cnt = P * cpg in the last block, not (p1 - p0) * cpg: at the smallest case whose last block is ragged in this type (fp32
    has seven whole blocks at 320 channels: the block-cap case there)."""
    _gn_mutation(dtype, True, _ragged_nhwc(dtype), "normal", "count_P")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_chan_merge_without_cross_term_fails(dtype):
    """m2 without d * d * cnt * w, on the gradient family (block means differ): NHWC with several blocks, NCHW with two."""
    _gn_mutation(dtype, True, eu.gn_nhwc_shapes(dtype)[2], "gradient", "no_cross_term")
    _gn_mutation(dtype, False, eu.GN_NCHW[0], "gradient", "no_cross_term")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_finalize_reading_64_partials_fails(dtype):
    _gn_mutation(dtype, True, eu.gn_nhwc_shapes(dtype)[4], "normal", "first_64_partials")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation,family", [("n_minus_1", "normal"), ("no_eps", "quiet")])
def test_variance_mutations_fail(dtype, mutation, family):
    """Variance over n - 1 (n = 105 in the first NHWC case); eps dropped where it is a tenth of a group's variance."""
    _gn_mutation(dtype, True, eu.gn_nhwc_shapes(dtype)[0], family, mutation)
    _gn_mutation(dtype, False, eu.GN_NCHW[0], family, mutation, silu=False)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_nchw_chunk_one_short_fails(dtype):
    _gn_mutation(dtype, False, eu.GN_NCHW[0], "normal", "chunk_short")
    _gn_mutation(dtype, False, eu.GN_NCHW[2], "normal", "chunk_short")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["vector_group", "gamma_shift", "beta_shift", "no_silu"])
def test_apply_mutations_fail(dtype, mutation):
    """At cpg = 3 and cpg = 15 (a 16-byte vector straddles groups in every type)."""
    for shape in (eu.gn_nhwc_shapes(dtype)[0], eu.gn_nhwc_shapes(dtype)[3]):
        _gn_mutation(dtype, True, shape, "normal", mutation)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_truncating_store_fails(dtype):
    """16-bit types only: fp32 stores its registers as they are, there is no store rounding to get wrong."""
    _gn_mutation(dtype, True, eu.gn_nhwc_shapes(dtype)[0], "normal", "truncate")
    _gn_mutation(dtype, True, eu.gn_nhwc_shapes(dtype)[0], "normal", "truncate", silu=False)


def _stats_mutation(dtype, index, mutation, cat=False):
    case, family = eu.GN_STATS[index]
    shape = eu.gn_stats_shape(case)
    (x, gamma, beta), ref = _gn_problem(shape, family, dtype, True, True)
    _fails(emu_group_norm_from_stats(x, gamma, beta, case, dtype, True, mutation, cat), ref, dtype, f"{mutation} {case}")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["no_c0_subtract", "tiles0_for_source1", "no_image_offset", "skip_straddle"])
@pytest.mark.parametrize("index", [0, 1])
def test_from_stats_mutations_fail(dtype, mutation, index):
    _stats_mutation(dtype, index, mutation)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("index", [0, 1])
def test_cat_second_source_at_the_wrong_stride_fails(dtype, index):
    _stats_mutation(dtype, index, "cat_stride_C", cat=True)


@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_vector_group_fails_at_cpg_60(dtype):
    """cpg = 60 is a whole number of fp32 vectors (4 values) and not of 16-bit ones (8): the mutation exists in 16 bits only."""
    _stats_mutation(dtype, 1, "vector_group")


def _ln_mutation(dtype, shape, family, mutation):
    x, gamma, beta = eu.ln_operands(shape, family)
    _fails(emu_layer_norm(x, gamma, beta, dtype, mutation), eu.layer_norm_ref64(x, gamma, beta, EPS, dtype), dtype, f"{mutation} {shape}")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["drop_last_vector", "mean_over_padded"])
def test_layer_norm_indexing_mutations_fail(dtype, mutation):
    for shape in ((5, 1432), (9, 640) if mutation == "drop_last_vector" else eu.ln_cases(dtype)[2]):
        _ln_mutation(dtype, shape, "normal", mutation)


@pytest.mark.parametrize("shape", [(7, 2048), (5, 1372)], ids=_name)
def test_layer_norm_one_pass_variance_fails_in_fp32(shape):
    """var = q - mean^2 on the offset family (q / var = 65).  The cancellation moves rstd by about 65 * 4 U_ACC = 1.5e-5 of
    itself: 1.6 to 2.6 times the fp32 budget at these two widths, and 4e-3 of what a 16-bit store rounds away - in bf16 and
    fp16 the emulation's ratio does not move in the third digit (0.99 and 0.97 with either variance), so the mutation is
    asserted in fp32 only."""
    _ln_mutation(torch.float32, shape, "offset", "one_pass")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("mutation", ["swap", "gate_at_state_stride", "tanh_gelu"])
def test_geglu_mutations_fail(dtype, mutation):
    shape = (5, 40)
    s, g = eu.geglu_operands(shape)
    _fails(emu_geglu(s, g, dtype, "mixed", mutation), eu.geglu_ref64(s, g, dtype), dtype, f"geglu {mutation}")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_geglu_without_second_pass_fails(dtype):
    shape = eu.GEGLU_STRIDE2[dtype]
    s, g = eu.geglu_operands(shape)
    _fails(emu_geglu(s, g, dtype, "dense", "no_second_pass"), eu.geglu_ref64(s, g, dtype), dtype, "geglu without the second pass")
