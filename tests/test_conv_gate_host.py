"""CPU proof that the per-element gate bites on the conv family, as tests/test_dma_gate_host.py proves it for the LDS-DMA GEMM:
an fp32 emulation of both conv loops' arithmetic -
  * the halo conv (csrc/conv_halo.h): channel-slice-major, nine tap trips a slice, the slabs of its K split over channel slices
    added in slice order;
  * the implicit GEMM (csrc/gemm_dma.h, CONV = true): tap-major K tiles, a K split whose slices may begin inside a filter tap,
    the two-source 1x1 form;
the three-product image arithmetic of split fp32 operands, bias / row bias / residual in fp32, ONE rounding to the stored type,
column partials of the stored values - passes the gate at every case tests/test_conv_edges_gpu.py launches, in every type and
both operand families, and every mutation a kernel bug would amount to fails it.  The case labels (kernel, tile, K split) are
held against the restated selection rules here.  No GPU, no operator library."""
import functools

import pytest
import torch

from tests import edge_util as eu
from tests.test_dma_gate_host import _fma, _images
from tests.test_edge_gate_host import _truncate

HALF = [torch.bfloat16, torch.float16]
F32 = torch.float32


def _name(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, (tuple, list)):
        return "-".join(_name(e) or str(e) for e in v)
    return None


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
def gather_index(cfg, mutation=None, th=None):
    """(M, taps): the flat input pixel (n * H + iy) * W + ix that output pixel m reads at tap (r, s), -1 = zero."""
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    Ho, Wo, M, _ = eu.conv_geometry(cfg)
    m = torch.arange(M)
    img, rem = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    cols = []
    for r in range(k):
        for s in range(k):
            iy, ix = oy * stride - pad + r, ox * stride - pad + s
            if mutation == "stride_origin" and stride == 2:
                iy = iy + 1                                               # iy = oy * stride - pad off by one
            if ups and mutation == "ups_shift":
                iy, ix = (oy >> 1) + r - 1, (ox >> 1) + s - 1            # instead of (oy + r - 1) >> 1
                ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            elif ups:
                ok = (iy >= 0) & (iy < 2 * H) & (ix >= 0) & (ix < 2 * W)
                iy, ix = iy >> 1, ix >> 1
            else:
                ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            idx = torch.where(ok, (img * H + iy) * W + ix, torch.full_like(m, -1))
            if mutation == "pad_left" and not ups:                        # the left padding column: the last pixel of the row above
                hit = (ix == -1) & (iy >= 1) & (iy < H)
                idx = torch.where(hit, (img * H + iy) * W - 1, idx)
            elif mutation == "halo_zero" and r == 0:                      # a tile's top halo row inside the image read as zero
                idx = torch.where((oy % th == 0) & (oy > 0), torch.full_like(m, -1), idx)
            elif mutation == "halo_other_image" and r == 0 and not ups:  # the second image's first tile: its halo row from the first image
                hit = (img >= 1) & (oy == 0) & (ix >= 0) & (ix < W)
                idx = torch.where(hit, img * H * W - W + ix, idx)
            cols.append(idx)
    return torch.stack(cols, 1)


def _gather(x, idx):
    """x (N, Cin, H, W) -> (M, taps, Cin) by `idx`."""
    flat = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
    flat = torch.cat([flat, torch.zeros(1, x.shape[1])])
    return flat[idx]                                                      # (-1 indexes the zero row)


def _units(kind, cfg, kb):
    """The K loop's units in order: halo - channel slices (nine positions each); implicit GEMM - K tiles (one position each)."""
    Cin, taps = cfg[1], cfg[5] * cfg[5]
    if kind == "halo":
        return [[(tap, cs * kb) for tap in range(9)] for cs in range(Cin // kb)]
    return [[divmod(kt * kb, Cin)] for kt in range(taps * Cin // kb)]


def emulate_acc(case, kind, sk, mutation=None, th=None, x_override=None):
    """fp32 accumulators (M, Cout) behind the K loop and the slab sum, as the kernel named by `kind` forms them."""
    cfg, dtype = case.cfg, case.dtype
    N, Cin, H, W, Cout, k, stride, pad, ups = cfg
    split, plain32 = case.split, dtype == F32 and not case.split
    kb = 32 if dtype == F32 else 64
    x = case.x if x_override is None else x_override
    idx = gather_index(cfg, mutation, th)
    xi = (x,) if plain32 else _images(x, dtype)
    wi = (case.w,) if plain32 else _images(case.w, dtype)
    A = [_gather(t, idx) for t in xi]
    Wt = [t.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin) for t in wi]
    if mutation == "drop_one_term":                                       # one (tap, channel) term, where an activation is not zero
        nz = A[0].abs().sum(0).nonzero()
        tap, c = (int(v) for v in nz[len(nz) // 2])
        A = [a.clone() for a in A]
        for a in A:
            a[:, tap, c] = 0.0
    units = _units(kind, cfg, kb)
    base, rem = divmod(len(units), sk)
    slabs, lo = [], 0
    for sl in range(sk):
        n = base + (1 if sl < rem else 0)
        if mutation == "drop_uneven_tail":                                 # the `split < nk_rem` term lost: every slice takes nk_base units
            lo, n = sl * base, base
        mine = list(range(lo, lo + n))
        if mutation == "shift_boundary" and sl == 1:                       # one unit summed twice, one never
            mine = list(range(lo - 1, lo + n - 1))
        pos = [p for u in mine for p in units[u]]
        if mutation == "midtap_start" and kind == "igemm" and pos[0][1] != 0:      # a slice that starts inside a tap begins at the tap's first channel
            k0 = pos[0][0] * Cin
            pos = [divmod(k0 + j * kb, Cin) for j in range(len(pos))]
        acc = torch.zeros(A[0].shape[0], Cout)
        corr = torch.zeros_like(acc) if len(A) == 2 else None
        for j, (tap, c0) in enumerate(pos):
            ac0 = wc0 = c0
            if kind == "halo" and j >= 9:
                if mutation == "stale_patch":                              # the slice reads the previous slice's patch (cs & 1 stuck)
                    ac0 = c0 - kb
                elif mutation == "ring_wrap" and tap < 2:                  # the two weight tiles issued at taps 7 and 8 come from the old slice
                    wc0 = c0 - kb
            a_, w_ = slice(ac0, ac0 + kb), slice(wc0, wc0 + kb)
            acc = acc + A[0][:, tap, a_] @ Wt[0][:, tap, w_].T
            if corr is not None:
                corr = corr + A[0][:, tap, a_] @ Wt[1][:, tap, w_].T
                corr = corr + A[1][:, tap, a_] @ Wt[0][:, tap, w_].T
        slabs.append(acc if corr is None else _fma(corr, torch.tensor(2.0 ** -11), acc))
        lo += n
    return slabs[0] if sk == 1 else functools.reduce(lambda a, s: a + s, slabs, torch.zeros_like(slabs[0]))


def emulate_store(case, acc, epi, bm=64, mutation=None):
    """+bias, +row bias, +residual in fp32 (the staged epilogue's order), one rounding: (N, Cout, Ho, Wo) in the stored type."""
    cfg, dtype = case.cfg, case.dtype
    N, Cout = cfg[0], cfg[4]
    Ho, Wo, M, _ = eu.conv_geometry(cfg)
    v = acc + case.b.to(dtype).float()
    if epi == "full":
        img = torch.arange(M) // (Ho * Wo)
        if mutation == "rowbias_first_image":                             # a tile that straddles two images: the row bias of its first image
            img = (torch.arange(M) // bm * bm) // (Ho * Wo)
        v = v + case.rb.to(dtype).float()[img]
    if epi in ("full", "res"):
        v = v + case.res.to(dtype).float().permute(0, 2, 3, 1).reshape(M, Cout)
    out = _truncate(v, dtype) if mutation == "truncate" else v.to(dtype)
    return out.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2)


def emulate_colstats(stored, bm, mutation=None):
    """(tiles, C, 2) fp32: per tile of bm rows the sums of the stored values and of their squares, 16 rows at a time, the partial
    sums added in order."""
    C = stored.shape[1]
    o = stored.float().permute(0, 2, 3, 1).reshape(-1, bm // 16, 16, C)
    if mutation == "colstats_short":                                       # one wave row (16 tile rows) too few
        o = o[:, :-1]
    s1, s2 = torch.zeros(o.shape[0], C), torch.zeros(o.shape[0], C)
    for g in range(o.shape[1]):
        s1, s2 = s1 + o[:, g].sum(1), s2 + (o[:, g] * o[:, g]).sum(1)
    return torch.stack([s1, s2], -1)


def _kind(label):
    return "halo" if label.startswith("halo") else "igemm"


def _run(case, label, epi, mutation=None, acc=None, x_override=None):
    bm, sk = eu.label_bm(label), eu.label_sk(label)
    th = bm // eu.conv_geometry(case.cfg)[1] if _kind(label) == "halo" else None
    if acc is None:
        acc = emulate_acc(case, _kind(label), sk, mutation, th, x_override)
    return emulate_store(case, acc, epi, bm, mutation)


def _case(dtype, label, cfg, family, plain=False):
    return eu.ConvCase(cfg, dtype, family, sk=eu.label_sk(label), split_operands=False if plain else None)


def _all_cases(dtype):
    """[(group, label, cfg, C0 or None, plain fp32)] - everything tests/test_conv_edges_gpu.py launches in `dtype`."""
    out = [(g, lab, cfg, None, False) for g in eu.CONV_GROUPS for lab, cfg in eu.conv_cases(dtype, g)]
    out += [("cat", lab, cfg, c0, False) for lab, cfg, c0 in eu.conv_cat_cases(dtype)]
    if dtype == F32:
        out += [("plain-fp32", lab, cfg, None, True) for lab, cfg in eu.CONV_PLAIN_F32]
    return out


# ------------------------------------------------------------------------------------------------ the labels are computed
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_labels_follow_the_restated_selection_rules(dtype):
    """conv_halo_applies, the halo time model and gemm_dispatch's cost model, restated in tests/edge_util.py, give every label of
    the case lists; uneven splits are uneven, and the implicit-GEMM splits (3x3) have a slice boundary inside a tap."""
    for group, label, cfg, c0, plain in _all_cases(dtype):
        got = eu.conv_plan(dtype, cfg, plain_f32=plain)
        assert got[0] == label, f"{group} {cfg} {dtype}: the rules give {got[0]}, the list says {label}"
        assert eu.label_bm(label) == got[1] and eu.label_sk(label) == got[3]
        assert group.startswith("halo") == eu.conv_halo_applies(dtype, cfg) or plain
    kb = 32 if dtype == F32 else 64
    for label, cfg in eu.conv_cases(dtype, "halo-k-split"):
        assert eu.label_sk(label) >= 2
    uneven = [(cfg[1] // kb) % eu.label_sk(label) != 0 for label, cfg in eu.conv_cases(dtype, "halo-k-split")]
    assert sum(uneven) >= 3 and max(eu.label_sk(label) for label, _ in eu.conv_cases(dtype, "halo-k-split")) > 8
    for label, cfg in eu.conv_cases(dtype, "igemm-k-split"):
        sk, nk = eu.label_sk(label), cfg[5] * cfg[5] * cfg[1] // kb
        base, rem = divmod(nk, sk)
        bounds = [s * base + min(s, rem) for s in range(1, sk)]
        assert sk >= 2 and ((rem != 0 and any(b * kb % cfg[1] for b in bounds)) or (cfg[5] == 1 and rem != 0) or cfg[6] == 2)
    assert {eu.label_sk(label) for label, _ in eu.conv_cases(dtype, "igemm-k-split")} == {2, 3, 4, 6, 8}
    for label, cfg, c0 in eu.conv_cat_cases(dtype):
        assert c0 != cfg[1] - c0 and c0 % kb == 0


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("family", eu.CONV_FAMILIES)
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_emulation_passes_at_every_gpu_case(dtype, family):
    """Worst ratios to the budget per group (printed).  Normal operands: the 16-bit types use most of the budget (the store's own
    rounding somewhere among thousands of elements), fp32 little (rounding errors of both signs add like sqrt(K), the budget
    takes K).  Exact-sum operands: the 16-bit types again the store's rounding, fp32 exactly 0 - and the two conditions that
    make that family see a one-term error hold for every case (ConvCase asserts them on the float64 reference)."""
    worst = {}
    for group, label, cfg, c0, plain in _all_cases(dtype):
        case = _case(dtype, label, cfg, family, plain)
        acc = emulate_acc(case, _kind(label), eu.label_sk(label))
        for epi in (("bias", "res") if c0 is not None else ("bias", "full")):
            out = _run(case, label, epi, acc=acc)
            r = case.gate(out, epi, f"emulated conv {cfg} {label} {epi}")
            worst[group] = max(worst.get(group, 0.0), r)
            bm, hw = eu.label_bm(label), eu.conv_geometry(cfg)[2] // cfg[0]
            if epi == "bias" and hw % bm == 0 and cfg[4] <= 1024:
                r1, r2 = eu.colstats_ratios(emulate_colstats(out, bm), bm, out, bm, family == "exact", f"emulated colstats {cfg}")
                worst["column-partials"] = max(worst.get("column-partials", 0.0), r1, r2)
    for group, r in worst.items():
        print(f"EMULATION conv {family} {group} {_name(dtype)}: worst ratio {r:.3g}")
    if family == "exact" and dtype == F32:
        assert max(worst.values()) == 0.0
    if dtype != F32 and family == "normal":
        assert worst["igemm-tiles"] > 0.5       # the gate is tight where the store's rounding leads (one K tile)


# ------------------------------------------------------------------------------------------------ every mutation fails
def _fails(case, out, epi, what):
    with pytest.raises(AssertionError, match="x its budget"):
        case.gate(out, epi, what)


def _pick(dtype, group, want):
    """The first case of a group whose label contains `want` (a case that exists in every type)."""
    for label, cfg in eu.conv_cases(dtype, group):
        if want in label:
            return label, cfg
    raise AssertionError(f"no {want} in {group} for {dtype}")


def _mutation_case(dtype, mutation):
    """(group, label fragment, epilogue) a mutation is shown on: the smallest listed case that exercises the mutated step."""
    return {
        "stale_patch": ("halo", "halo<5,8", "bias"), "ring_wrap": ("halo", "halo<5,8", "bias"),
        "drop_uneven_tail": ("halo-k-split", "halo<6,4", "bias"), "shift_boundary": ("igemm-k-split", "igemm<64x64>/sk4", "bias"),
        "pad_left": ("igemm-geometry", "igemm<64x64>/sk4", "bias"), "halo_zero": ("halo", "halo<5,8", "bias"),
        "halo_other_image": ("halo", "halo<6,4,128>", "bias"), "ups_shift": ("halo", "ups", "bias"),
        "stride_origin": ("igemm-k-split", "igemm<64x64>/sk4", "bias"), "midtap_start": ("igemm-k-split", "igemm<64x64>/sk6", "bias"),
        "rowbias_first_image": ("igemm-k-split", "igemm<128x64>/sk4", "full"),
    }[mutation]


_INDEX_MUTATIONS = ["stale_patch", "ring_wrap", "drop_uneven_tail", "shift_boundary", "pad_left", "halo_zero", "halo_other_image",
                    "ups_shift", "stride_origin", "midtap_start", "rowbias_first_image"]


@pytest.mark.parametrize("family", eu.CONV_FAMILIES)
@pytest.mark.parametrize("mutation", _INDEX_MUTATIONS)
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_indexing_mutations_fail(dtype, mutation, family):
    """A stale patch buffer, the weight ring's wrap taking the old slice, the tail of an uneven split dropped, a slice boundary
    one unit off, the left padding column read from the row above, a tile's top halo row read as zero, the halo row of another
    image, the upsampling shift applied before the tap offset, the stride-2 origin off by one, a mid-tap slice started at the
    tap's first channel, a straddling tile's row bias from its first image: each fails the gate in every type and on both
    operand families (the unmutated emulation of the same case passes)."""
    group, want, epi = _mutation_case(dtype, mutation)
    if mutation == "stride_origin":
        label, cfg = next((l, c) for l, c in eu.conv_cases(dtype, group) if c[6] == 2)
    elif mutation == "halo_other_image":
        label, cfg = next((l, c) for l, c in eu.conv_cases(dtype, group) if c[0] == 2 and not c[8])
    elif mutation == "pad_left":
        label, cfg = next((l, c) for l, c in eu.conv_cases(dtype, group) if c[5] == 3 and c[6] == 1 and c[7] == 1 and not c[8])
    else:
        label, cfg = _pick(dtype, group, want)
    case = _case(dtype, label, cfg, family)
    case.gate(_run(case, label, epi), epi, "unmutated")
    _fails(case, _run(case, label, epi, mutation), epi, mutation)


@pytest.mark.parametrize("family", eu.CONV_FAMILIES)
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_swapped_cat_sources_fail(dtype, family):
    label, cfg, c0 = eu.conv_cat_cases(dtype)[0]
    case = _case(dtype, label, cfg, family)
    swapped = torch.cat([case.x[:, c0:], case.x[:, :c0]], 1)
    case.gate(_run(case, label, "res"), "res", "unmutated")
    _fails(case, _run(case, label, "res", x_override=swapped), "res", "cat sources swapped")


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_one_dropped_term_at_the_longest_k_fails_on_exact_operands(dtype):
    """One (tap, channel) term of 11520 (16 bit; 5760 as split fp32) dropped, at the longest K of the lists.  The exact-sum
    family sees it: the budget is the store rounding alone and the term is at least 1/8.  The normal family CANNOT see it there,
    and the test says so by asserting that the mutated emulation passes its gate: a term is about |x w| ~ K^-1/2 mag / K, while
    the accumulation term of the budget is 2 (K + 8) 2^-24 mag: at K = 11520 a term is ten times smaller than what rounding alone may
    cost, and the 16-bit types add their store rounding to that."""
    longest = max((c for g in eu.CONV_GROUPS for c in eu.conv_cases(dtype, g)), key=lambda c: c[1][5] * c[1][5] * c[1][1])
    label, cfg = longest
    assert cfg[1] == (640 if dtype == F32 else 1280) and cfg[5] == 3
    exact = _case(dtype, label, cfg, "exact")
    exact.gate(_run(exact, label, "bias"), "bias", "unmutated")
    _fails(exact, _run(exact, label, "bias", "drop_one_term"), "bias", "one dropped term")
    if dtype == F32:
        return              # (K = 5760, no store rounding: the largest single terms still show, a typical one does not)
    normal = _case(dtype, label, cfg, "normal")
    normal.gate(_run(normal, label, "bias", "drop_one_term"), "bias", "one dropped term (masked on normal operands)")


@pytest.mark.parametrize("family", eu.CONV_FAMILIES)
@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_truncating_store_fails(dtype, family):
    """On normal operands while 2 (K + 8) 2^-24 mag stays under U_OUT |ref|: Cin <= 128, and in fp16 K <= 136 as well
    (tests/test_edge_gate_host.py: a 3x3 conv at Cin = 128 sums 1152 terms, whose accumulation term hides fp16's 2^-11).  On
    exact-sum operands at any K, through the family's spots (tests/edge_util.py: _exact_spots) - everywhere else its stored
    values are values of the type, and truncation gives the same bits as rounding.  fp32 stores its accumulator as it is."""
    long3x3 = [_pick(dtype, "halo", "halo<5,8"), next(c for c in eu.conv_cases(dtype, "igemm-geometry") if c[1][2:4] == (24, 24))]
    if family == "exact":
        cases = long3x3 + [_pick(dtype, "halo-k-split", "sk9")]
    else:              # K <= 128: the 1x1 convs; bf16, whose store rounding is eight times fp16's, also the 3x3 at Cin = 128
        cases = [eu.conv_cases(dtype, "igemm-tiles")[0], next(c for c in eu.conv_cases(dtype, "igemm-geometry") if c[1][5] == 1)]
        cases += long3x3 if dtype == torch.bfloat16 else []
        assert all(cfg[1] <= 128 for _, cfg in cases)
    for label, cfg in cases:
        case = _case(dtype, label, cfg, family)
        epi = "bias" if family == "exact" else "full"
        case.gate(_run(case, label, epi), epi, "unmutated")
        _fails(case, _run(case, label, epi, "truncate"), epi, f"truncate {cfg}")


@pytest.mark.parametrize("family", eu.CONV_FAMILIES)
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_short_column_partials_fail(dtype, family):
    """Column partials summed over one wave row (16 of the tile's rows) too few: over the derived bound on normal operands, not
    equal on exact ones."""
    for group, want in (("halo", "halo<5,8"), ("igemm-geometry", "igemm<128x64>")):
        label, cfg = next((l, c) for l, c in eu.conv_cases(dtype, group) if want in l and (eu.conv_geometry(c)[2] // c[0]) % eu.label_bm(l) == 0)
        case = _case(dtype, label, cfg, family)
        bm = eu.label_bm(label)
        out = _run(case, label, "bias")
        eu.colstats_ratios(emulate_colstats(out, bm), bm, out, bm, family == "exact", "unmutated")
        with pytest.raises(AssertionError, match="x their budget|are not exact|over their budget"):
            eu.colstats_ratios(emulate_colstats(out, bm, "colstats_short"), bm, out, bm, family == "exact", "short")
        with pytest.raises(AssertionError, match="the case is labelled"):
            eu.colstats_ratios(emulate_colstats(out, bm), bm // 2, out, bm, family == "exact", "rows")
