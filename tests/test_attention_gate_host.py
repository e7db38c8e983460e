"""CPU proof that the per-element attention gate of tests/edge_util.py (AttentionRef) bites: a torch fp32 / 16-bit emulation of
the attention kernels' arithmetic (csrc/attention_core.h, attention.hip, attention_anyd.hip, attention_f32.hip) -
  tiles of 64 keys, zero-filled and masked past S; q' = round_E(fp32(q) * c) once; scores accumulated in fp32 from -m_ref;
  the exact path on tile 0 and on a tile that outruns m_ref by more than the lag, O and the row sum rescaled by alpha there;
  P = 2^s rounded to the element type, the row sum taken from the ROUNDED P; one division and one rounding at the store;
  fp32 tensors as split images (hi + lo * 2^-11, three products, a main and a correction accumulator) -
passes the gate at every shape, type and family tests/test_attention_edges_gpu.py launches, and every mutation a kernel bug
would amount to fails it in both 16-bit types (and on split fp32 operands).  The two constants of the budget that cannot be derived are measured here.

Known undetectable (inside the rounding budget by construction, not bugs of the kind the gate is for, not asserted): a row sum
taken from the UNROUNDED p (the error of P then no longer cancels between numerator and denominator, but stays within u_E),
and a pre-scaled Q that is not rounded to the element type (the reference rounds it as the design states; leaving the
rounding out moves outputs by about half the budget at most).  No GPU, no operator library."""
import functools
import math

import pytest
import torch

from tests import edge_util as eu
from tests.test_edge_gate_host import _truncate

HALF = list(eu.ATT_HALF)
KV = 64


def _name(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, (tuple, list)):
        return "-".join(_name(e) or str(e) for e in v)
    return None


# ------------------------------------------------------------------------------------------------ the emulation and its mutations
def _fma(a, b, c):
    """fp32 fma(a, b, c) with a power-of-two b: the product is exact, the sum rounds at 53 bits and again at 24."""
    return (a.double() * b + c.double()).float()


def _images(t, dtype):
    """What the matrix pipe multiplies: the value rounded to the 16-bit type, or (hi, lo) of the split fp32 image (csrc/split.h)."""
    if dtype != torch.float32:
        return (t.to(dtype).float(),)
    hi = t.half().float()
    return hi, ((t - hi) * 2048.0).half().float()


def _product(a, b):
    """sum over the images: main accumulator a0 b0, correction a0 b1 + a1 b0 (in the kernels' order); None for 16-bit types"""
    main = a[0] @ b[0]
    return (main, None) if len(a) == 1 else (main, a[0] @ b[1] + a[1] @ b[0])


MUTATIONS = ("drop_last_key", "admit_key_S", "swap_v_rows", "stale_slot", "no_rescale", "sum_skips_tile", "truncate", "clamped_row")


def emulate(q, k, v, H, scale, dtype, mutation=None, split=True):
    """ops.attention as the kernels compute it; q (B, T, H*D), k / v (B, S, H*D) fp32.  split=False (fp32 tensors only): the
    same arithmetic on the fp32 values themselves - what test_measured_constants compares the split images with."""
    f32 = dtype == torch.float32
    idt = dtype if (not f32 or split) else None                        # None: one image, the fp32 value
    img = (lambda t: _images(t, idt)) if idt is not None else (lambda t: (t,))
    B, T, _ = q.shape
    S = k.shape[1]
    qi = img(eu.att_heads(eu.attention_prescale(q, scale, dtype).float(), H))
    kh, vh = eu.att_heads(k.to(dtype).float(), H), eu.att_heads(v.to(dtype).float(), H)
    D = kh.shape[-1]
    nkt = (S + KV - 1) // KV
    pad = nkt * KV + KV - S                                             # keys S .. are a zero line (one whole tile more: admit_key_S at S % 64 == 0 has no place)
    kh = torch.cat([kh, torch.zeros(B, H, pad, D)], 2)
    vh = torch.cat([vh, torch.zeros(B, H, pad, D)], 2)
    m = torch.zeros(B, H, T)
    om, oc = torch.zeros(B, H, T, D), torch.zeros(B, H, T, D)
    lm, lc = torch.zeros(B, H, T), torch.zeros(B, H, T)
    for kt in range(nkt):
        src = kt - 6 if (mutation == "stale_slot" and kt >= 6) else kt       # the ring slot still holds the tile of six trips ago
        ks = slice(src * KV, src * KV + KV)
        ki, vt = img(kh[:, :, ks].transpose(-1, -2)), vh[:, :, ks]
        live = min(KV, S - kt * KV)
        if kt == nkt - 1:
            if mutation == "drop_last_key":
                live -= 1
            elif mutation == "admit_key_S" and live < KV:
                live += 1
            elif mutation == "swap_v_rows" and live >= 2:
                vt = vt.clone()
                vt[:, :, [0, 1]] = vt[:, :, [1, 0]]
        vi = img(vt)
        mn, cr = _product(qi, ki)
        mn = mn - m[..., None]                                           # (the MFMA chain starts at -m_ref)
        s = mn if cr is None else _fma(cr, 2.0 ** -11, mn)
        s[..., live:] = -math.inf
        mx = s.max(-1).values
        if kt == 0:
            delta = torch.where(mx > -math.inf, mx, torch.zeros(()))
            alpha = torch.ones_like(mx)
        else:
            delta = torch.where(mx > eu.ATT_LAG, mx, torch.zeros(()))
            alpha = torch.ones_like(mx) if mutation == "no_rescale" else torch.exp2(-delta)
        s = s - delta[..., None]
        m = m + delta
        om, lm = om * alpha[..., None], lm * alpha
        if cr is not None:
            oc, lc = oc * alpha[..., None], lc * alpha
        pi = img(torch.exp2(s))
        a, c = _product(pi, vi)
        om = om + a
        if not (mutation == "sum_skips_tile" and kt == nkt - 1):
            lm = lm + pi[0].sum(-1)
        if c is not None:
            oc = oc + c
            if not (mutation == "sum_skips_tile" and kt == nkt - 1):
                lc = lc + pi[1].sum(-1)
    if len(qi) == 2:
        om, lm = _fma(oc, 2.0 ** -11, om), _fma(lc, 2.0 ** -11, lm)
    o = eu.att_tokens(om * (1.0 / lm)[..., None])
    if mutation == "clamped_row" and T >= 2:
        o = o.clone()
        o[:, T - 2] = o[:, T - 1]
    return _truncate(o, dtype) if mutation == "truncate" else o.to(dtype)


@functools.lru_cache(maxsize=4)
def _problem(family, shape, dtype):
    B, T, S, H, D = shape
    q, k, v, pairs = eu.attention_inputs(family, B, T, S, H, D)
    return q, k, v, pairs, eu.AttentionRef(q, k, v, H, D ** -0.5, dtype)


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
def test_emulation_passes_at_every_gpu_case(dtype):
    """Worst ratio to the budget per group (type x kernel x family), printed; the spotlight condition holds at every
    spotlight case."""
    worst = {}
    for tag, shape, family in eu.attention_cases(dtype):
        B, T, S, H, D = shape
        q, k, v, pairs, ref = _problem(family, shape, dtype)
        if pairs is not None:
            eu.assert_spotlight_condition(ref, pairs, S, H)
        r = ref.gate(emulate(q, k, v, H, D ** -0.5, dtype), f"emulated attention {tag} {shape} {family}")
        worst[(tag, family)] = max(worst.get((tag, family), 0.0), r)
    for (tag, family), r in worst.items():
        print(f"EMULATION attention {_name(dtype)} {tag} {family}: worst ratio {r:.3g}")
    # the gate is tight where the roundings to the element type lead: the emulation uses a good part of it
    assert dtype == torch.float32 or max(worst.values()) > 0.3


def test_measured_constants():
    """ATT_EXP2_ULPS: the fp32 exp2 against float64 at exponents of the kernels' range [-40, ATT_LAG], in ulp.  ATT_SPLIT_MULT:
    the split emulation against the same emulation on the fp32 values, in units of the worst-case split terms of the budget.
    edge_util's constants cover what is measured and are at most twice it."""
    x = torch.linspace(-40.0, eu.ATT_LAG, 400001)
    e, e64 = torch.exp2(x).double(), torch.exp2(x.double())
    ulps = float(((e - e64).abs() / e64).max()) / 2.0 ** -23
    mult = 0.0
    for tag, shape, family in eu.ATT_F32 + [c for c in eu.ATT_ANYD if c[1][1] == 129]:
        B, T, S, H, D = shape
        q, k, v, pairs, ref = _problem(family, shape, torch.float32)
        a = emulate(q, k, v, H, D ** -0.5, torch.float32).double()
        b = emulate(q, k, v, H, D ** -0.5, torch.float32, split=False).double()
        worst_case = (math.log(2.0) * eu.split_term(ref.qk) + eu.SPLIT_OPERAND_U) * ref.weight + eu.split_term(ref.mag + ref.ref.abs())
        mult = max(mult, float(((a - b).abs() / worst_case.clamp_min(1e-300)).max()))
    print(f"MEASURED exp2: {ulps:.3f} ulp; split images: {mult:.3f} of their worst-case terms")
    assert ulps <= eu.ATT_EXP2_ULPS <= 2.0 * ulps
    assert mult <= eu.ATT_SPLIT_MULT <= 2.0 * mult


# ------------------------------------------------------------------------------------------------ every mutation fails
# (T, S) of the GPU cases on one head (two for the 16-row kernel's), so that a mutation is tried where it can occur:
# one to thirteen key tiles, tails of 1, 13, 33 and 63 keys, a whole last tile, the ring wrap (S > 384)
MUTATION_SHAPES = [(1, 65, 77, 2, 64), (1, 65, 255, 2, 64), (1, 97, 257, 1, 64), (1, 97, 289, 1, 64), (1, 97, 320, 1, 64),
                   (1, 97, 449, 1, 64), (1, 97, 769, 1, 64), (2, 33, 129, 3, 32)]
# the families in which a mutation must fail the gate at every shape where it can occur (the others are tried and printed):
#  drop_last_key   spotlight: key S - 1 holds >= ATT_SPOT_MIN_P of a row.  (normal: 1 / S of a row - inside the budget of bf16.)
#  admit_key_S     negative only: every true score is far below 0, the zero key's 2^0 takes the row; elsewhere one key more
#                  among S of the same weight, with v = 0.
#  swap_v_rows     spotlight: both rows belong to the last tile, whose every key is lit.
#  stale_slot      every family (a whole tile of wrong keys and values).
#  no_rescale      spotlight only: rows whose maximum moves by 11 or 23 units; normal and negative rows seldom outrun the lag.
#  sum_skips_tile  spotlight (the last tile holds a lit key of some row); normal as well when the tile is not nearly empty.
#  truncate        spotlight only: rows that one key owns have W << |ref|, so the budget there is the store's own U_OUT |ref|.
#  clamped_row     every family.
MUST_FAIL = {"drop_last_key": ("spotlight",), "admit_key_S": ("negative",), "swap_v_rows": ("spotlight",),
             "stale_slot": eu.ATT_FAMILIES, "no_rescale": ("spotlight",), "sum_skips_tile": ("spotlight",),
             "truncate": ("spotlight",), "clamped_row": eu.ATT_FAMILIES}


def _can_occur(mutation, shape):
    B, T, S, H, D = shape
    tail = S - (S - 1) // KV * KV
    return {"admit_key_S": tail < KV, "swap_v_rows": tail >= 2, "stale_slot": S > 384, "no_rescale": S > KV}.get(mutation, True)


@pytest.mark.parametrize("dtype", eu.DTYPES, ids=_name)
@pytest.mark.parametrize("shape", MUTATION_SHAPES, ids=_name)
def test_every_mutation_fails(dtype, shape):
    """Both 16-bit types, and fp32 tensors on split operands as well (without `truncate`: an fp32 store drops nothing)."""
    B, T, S, H, D = shape
    for family in eu.ATT_FAMILIES:
        q, k, v, pairs, ref = _problem(family, shape, dtype)
        base = ref.gate(emulate(q, k, v, H, D ** -0.5, dtype), "unmutated")
        line = f"MUTATIONS {_name(dtype)} {_name(shape)} {family}: unmutated {base:.2f}"
        for mutation in MUTATIONS:
            if not _can_occur(mutation, shape) or (mutation == "truncate" and dtype not in HALF):
                continue
            out = emulate(q, k, v, H, D ** -0.5, dtype, mutation=mutation)
            r = ref.ratio(out)
            line += f" {mutation} {r:.3g}"
            if family in MUST_FAIL[mutation]:
                assert r > 1.0, f"{mutation} passes the gate ({r:.3g} of the budget) at {shape} {family} {_name(dtype)}"
                with pytest.raises(AssertionError, match="x its budget|non-finite"):
                    ref.gate(out, mutation)
        print(line)
