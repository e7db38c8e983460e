"""LoCon conv adapters and DoRA without a GPU: the parser's new spellings and refusals, and LoraSet on a CPU fp32 TINY module
in channels_last (torch merge, the kernel's formula) against the float64 formula computed on the 4-D weights:

    V_j = B + s_j (alpha_j / r_j) up_j down_j,   g_j[n] = m_j[n] / ||V_j[n]||  (1 for a plain adapter),   W = B + sum_j (g_j V_j - B)."""
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from stabletriton_amd import _C, lora, synth
from stabletriton_amd.build import lib_path
from stabletriton_amd.unet import TINY, UNet2DConditionModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_TOL = 1e-5


def _model():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m.to(memory_format=torch.channels_last)


def _shapes(m, kinds=(nn.Linear, nn.Conv2d)):
    return {n: tuple(l.weight.shape) for n, l in m.named_modules() if isinstance(l, kinds)}


def _adapter(m, rank, seed, dora, names=None, form="kohya", alpha=None):
    """A seeded adapter on the Linear and Conv2d modules of `m`: (state dict, {module: (down, up, magnitude or None)}).
    Conv factors are down (r, I, R, S) and up (O, r, 1, 1); a magnitude is ||B[n]|| * U(0.5, 1.5) per output row."""
    g = torch.Generator().manual_seed(seed)
    sd, facs = {}, {}
    for n, shape in _shapes(m).items():
        if names is not None and not names(n):
            continue
        w = dict(m.named_modules())[n].weight
        if len(shape) == 4:
            down, up = torch.randn(rank, *shape[1:], generator=g) * 0.1, torch.randn(shape[0], rank, 1, 1, generator=g) * 0.1
        else:
            down, up = torch.randn(rank, shape[1], generator=g) * 0.1, torch.randn(shape[0], rank, generator=g) * 0.1
        mag = w.detach().reshape(shape[0], -1).norm(dim=1) * (0.5 + torch.rand(shape[0], generator=g)) if dora else None
        facs[n] = (down, up, mag)
        if form == "kohya":
            stem = "lora_unet_" + n.replace(".", "_")
            sd[stem + ".lora_down.weight"], sd[stem + ".lora_up.weight"] = down, up
            if alpha is not None:
                sd[stem + ".alpha"] = torch.tensor(float(alpha))
            if dora:
                sd[stem + ".dora_scale"] = mag.reshape(-1, *([1] * (len(shape) - 1)))        # (N, 1) / (O, 1, 1, 1)
        else:
            sd[f"unet.{n}.lora_A.weight"], sd[f"unet.{n}.lora_B.weight"] = down, up
            if alpha is not None:
                sd[f"unet.{n}.alpha"] = torch.tensor(float(alpha))
            if dora:
                sd[f"unet.{n}.lora_magnitude_vector"] = mag
    return sd, facs


def _formula64(base, adapters):
    """adapters: [(facs, alpha or None, scale)] -> {module: W64 in the weight's own 4-D / 2-D shape}."""
    out = {}
    for n in {n for facs, _, _ in adapters for n in facs}:
        b = base[n + ".weight"].double()
        rows = b.reshape(b.shape[0], -1)                              # K in (I, R, S) order, like the 4-D factors
        w = rows.clone()
        for facs, alpha, s in adapters:
            if n not in facs or s == 0.0:
                continue
            down, up, mag = facs[n]
            r = down.shape[0]
            v = rows + s * ((alpha if alpha is not None else r) / r) * (up.double().reshape(-1, r) @ down.double().reshape(r, -1))
            gain = (mag.double() / v.norm(dim=1))[:, None] if mag is not None else 1.0
            w = w + gain * v - rows
        out[n] = w.reshape(b.shape)
    return out


def _assert_formula(m, base, adapters):
    worst = 0.0
    mods = dict(m.named_modules())
    for n, w64 in _formula64(base, adapters).items():
        err = float((mods[n].weight.double() - w64).abs().max() / w64.abs().max())
        worst = max(worst, err)
        assert err <= REL_TOL, f"{n}: {err:.3e} relative to the largest element"
    print(f"worst relative error {worst:.3e}")


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_places_conv_factors_and_magnitudes_in_every_spelling():
    m = _model()
    shapes = _shapes(m)
    convs = [n for n, s in shapes.items() if len(s) == 4]
    for want in ("conv_in", "conv_out", "down_blocks.0.resnets.0.conv1", "down_blocks.0.downsamplers.0.conv", "up_blocks.0.upsamplers.0.conv"):
        assert want in convs
    assert any(n.endswith("conv_shortcut") for n in convs) and any(n.endswith("conv2") for n in convs)
    for form in ("kohya", "peft"):
        sd, facs = _adapter(m, 4, 1, dora=True, form=form, alpha=2)
        for names in (shapes.keys(), shapes):                          # names alone, or names with shapes (checked while parsing)
            placed, unplaced = lora.parse_adapter(sd, names)
            triples, _ = lora.parse_lora_state_dict(sd, names)           # the historical form: the same triples, no magnitude
            assert unplaced == [] and sorted(placed) == sorted(shapes) == sorted(triples), form
            for n, p in placed.items():
                down, up, alpha = triples[n]
                assert torch.equal(down, p.down) and torch.equal(up, p.up) and alpha == p.alpha
                assert alpha == 2.0 and torch.equal(down.reshape(-1), facs[n][0].reshape(-1)) and torch.equal(up.reshape(-1), facs[n][1].reshape(-1))
                assert torch.equal(p.magnitude.reshape(-1), facs[n][2]), f"{form}: {n}"
        # the Linear names alone leave every conv key - factors and magnitude - unplaced, as before
        lin = _shapes(m, nn.Linear)
        placed, unplaced = lora.parse_lora_state_dict(sd, lin.keys())
        assert sorted(placed) == sorted(lin) and len(unplaced) == 4 * len(convs)
    # PEFT's magnitude spellings: bare, with an adapter name, with .weight, with both; any shape of N elements
    name = "mid_block.attentions.0.proj_in"
    n_rows, k = shapes[name]
    ab = {f"{name}.lora_A.weight": torch.zeros(4, k), f"{name}.lora_B.weight": torch.zeros(n_rows, 4)}
    mag = torch.arange(n_rows, dtype=torch.float32)
    for key, val in ((f"{name}.lora_magnitude_vector", mag), (f"unet.{name}.lora_magnitude_vector.default", mag[None, :]),
                     (f"{name}.lora_magnitude_vector.weight", mag[:, None]), (f"unet.{name}.lora_magnitude_vector.default_0.weight", mag)):
        placed, unplaced = lora.parse_adapter(dict(ab, **{key: val}), shapes)
        assert unplaced == [] and torch.equal(placed[name].magnitude.reshape(-1), mag), key
    placed, _ = lora.parse_adapter(ab, shapes)
    assert placed[name].magnitude is None
    # kohya's dora_scale: N as its first dimension, whatever follows; the same N elements folded differently are refused
    stem = "lora_unet_" + name.replace(".", "_")
    ko = {stem + ".lora_down.weight": torch.zeros(4, k), stem + ".lora_up.weight": torch.zeros(n_rows, 4)}
    for val in (mag, mag[:, None]):
        placed, _ = lora.parse_adapter(dict(ko, **{stem + ".dora_scale": val}), shapes.keys())
        assert torch.equal(placed[name].magnitude.reshape(-1), mag)
    for names in (shapes.keys(), shapes):
        with pytest.raises(ValueError, match="first dimension"):
            lora.parse_adapter(dict(ko, **{stem + ".dora_scale": mag.reshape(2, n_rows // 2)}), names)
    with pytest.raises(ValueError, match="magnitude"):
        lora.parse_lora_state_dict(dict(ab, **{f"{name}.lora_magnitude_vector": mag[:-1]}), shapes)


def test_parser_refuses_what_it_cannot_apply():
    m = _model()
    shapes = _shapes(m)
    conv, lin = "down_blocks.0.resnets.0.conv1", "mid_block.attentions.0.proj_in"
    o, i, r_, s_ = shapes[conv]
    n, k = shapes[lin]
    stem_c, stem_l = "lora_unet_" + conv.replace(".", "_"), "lora_unet_" + lin.replace(".", "_")
    good_c = {stem_c + ".lora_down.weight": torch.zeros(4, i, r_, s_), stem_c + ".lora_up.weight": torch.zeros(o, 4, 1, 1)}
    good_l = {stem_l + ".lora_down.weight": torch.zeros(4, k), stem_l + ".lora_up.weight": torch.zeros(n, 4)}
    lora.parse_lora_state_dict(dict(good_c, **good_l), shapes)
    # LyCORIS's input-axis decomposition: dora_scale (1, K) / (1, I, R, S)
    with pytest.raises(ValueError, match="input axis"):
        lora.parse_lora_state_dict(dict(good_l, **{stem_l + ".dora_scale": torch.ones(1, k)}), shapes.keys())
    with pytest.raises(ValueError, match="input axis"):
        lora.parse_lora_state_dict(dict(good_c, **{stem_c + ".dora_scale": torch.ones(1, i, r_, s_)}), shapes.keys())
    # Tucker's core, LoHa, LoKr
    with pytest.raises(ValueError, match="Tucker"):
        lora.parse_lora_state_dict(dict(good_c, **{stem_c + ".lora_mid.weight": torch.zeros(4, 4, r_, s_)}), shapes.keys())
    with pytest.raises(ValueError, match="LoHa"):
        lora.parse_lora_state_dict({stem_l + ".hada_w1_a": torch.zeros(n, 4), stem_l + ".hada_w1_b": torch.zeros(4, k)}, shapes.keys())
    with pytest.raises(ValueError, match="LoKr"):
        lora.parse_lora_state_dict({stem_l + ".lokr_w1": torch.zeros(4, 4), stem_l + ".lokr_w2": torch.zeros(n // 4, k // 4)}, shapes.keys())
    # a 1x1 down factor on a 3x3 convolution (with and without shapes at parse time: LoraSet.load checks too)
    bad = {stem_c + ".lora_down.weight": torch.zeros(4, i, 1, 1), stem_c + ".lora_up.weight": torch.zeros(o, 4, 1, 1)}
    with pytest.raises(ValueError, match="kernel"):
        lora.parse_lora_state_dict(bad, shapes)
    with pytest.raises(ValueError, match="kernel"):
        lora.LoraSet(m).load("a", bad, convs=True)
    with pytest.raises(ValueError, match=re.escape(conv)):
        lora.parse_lora_state_dict({stem_c + ".lora_down.weight": torch.zeros(4, i + 1, r_, s_), stem_c + ".lora_up.weight": torch.zeros(o, 4, 1, 1)}, shapes)
    # an incomplete pair; a magnitude without factors
    with pytest.raises(ValueError, match="incomplete"):
        lora.parse_lora_state_dict({stem_c + ".lora_down.weight": torch.zeros(4, i, r_, s_)}, shapes.keys())
    with pytest.raises(ValueError, match="incomplete"):
        lora.parse_lora_state_dict({stem_c + ".dora_scale": torch.ones(o, 1, 1, 1)}, shapes.keys())
    # grouped / dilated targets
    net = nn.Sequential(nn.Conv2d(8, 8, 3, groups=2), nn.Conv2d(8, 8, 3, dilation=2), nn.Linear(4, 4)).requires_grad_(False)
    ls = lora.LoraSet(net)
    for idx, shape in ((0, (2, 4, 3, 3)), (1, (2, 8, 3, 3))):
        with pytest.raises(ValueError, match="grouped or dilated"):
            ls.load("a", {f"{idx}.lora_A.weight": torch.zeros(shape), f"{idx}.lora_B.weight": torch.zeros(8, 2, 1, 1)}, convs=True)


# ------------------------------------------------------------------------------------------------ LoraSet on the CPU
def test_dora_on_every_linear_and_conv_matches_float64_and_round_trips():
    m = _model()
    shapes = _shapes(m)
    base = {k: v.clone() for k, v in m.state_dict().items()}
    strides = {k: v.stride() for k, v in m.state_dict().items()}
    ls = lora.attach(m)
    sd, facs = _adapter(m, 8, 2, dora=True, alpha=4)
    versions = {n: l.weight._version for n, l in m.named_modules() if n in shapes}
    assert ls.load("d", sd, scale=0.8, convs=True) == []
    assert sorted(ls.adapted_modules()) == sorted(shapes)
    assert all(l.weight._version > versions[n] for n, l in m.named_modules() if n in shapes), "version counters must move"
    assert not any(torch.equal(m.state_dict()[n + ".weight"], base[n + ".weight"]) for n in shapes)
    assert all(v.stride() == strides[k] for k, v in m.state_dict().items()), "a merge keeps every weight's layout"
    _assert_formula(m, base, [(facs, 4.0, 0.8)])
    at_08 = {k: v.clone() for k, v in m.state_dict().items()}
    ls.set_scale("d", -1.3)
    _assert_formula(m, base, [(facs, 4.0, -1.3)])
    ls.set_scale("d", 0.8)
    assert all(torch.equal(v, at_08[k]) for k, v in m.state_dict().items()), "returning to a scale must return the bits"
    ls.set_scale("d", 0.0)
    assert all(torch.equal(v, base[k]) for k, v in m.state_dict().items()), "scale 0 is the base, magnitude included"
    ls.set_scale("d", 0.8)
    ls.unload("d")
    assert ls.names() == [] and ls.adapted_modules() == []
    assert all(torch.equal(v, base[k]) for k, v in m.state_dict().items()), "unload restores every parameter bit for bit"
    # the PEFT spelling of the same adapter gives the same weights
    sd_p, _ = _adapter(m, 8, 2, dora=True, alpha=4, form="peft")
    ls.load("p", sd_p, scale=0.8, convs=True)
    assert all(torch.equal(v, at_08[k]) for k, v in m.state_dict().items())


def test_a_contiguous_model_takes_the_same_adapter():
    """Conv weights that are not channels_last are merged through their (O, I R S) view: the same weights, up to summation order."""
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    assert m.conv_in.weight.is_contiguous()
    base = {k: v.clone() for k, v in m.state_dict().items()}
    sd, facs = _adapter(m, 8, 2, dora=True)
    lora.LoraSet(m).load("d", sd, scale=0.8, convs=True)
    _assert_formula(m, base, [(facs, None, 0.8)])


def test_a_dora_and_a_plain_adapter_on_one_weight_match_the_formula():
    m = _model()
    base = {k: v.clone() for k, v in m.state_dict().items()}
    ls = lora.LoraSet(m)
    sd_d, facs_d = _adapter(m, 8, 3, dora=True)
    sd_p, facs_p = _adapter(m, 4, 4, dora=False, names=lambda n: "conv" in n or "attn1" in n, form="peft")
    ls.load("d", sd_d, 0.7, convs=True)
    ls.load("p", sd_p, -0.9, convs=True)
    _assert_formula(m, base, [(facs_d, None, 0.7), (facs_p, None, -0.9)])
    both = {k: v.clone() for k, v in m.state_dict().items()}
    ls.set_scale("d", 0.0)                                             # the DoRA adapter is skipped whole: today's plain formula
    _assert_formula(m, base, [(facs_p, None, -0.9)])
    ls.set_scales({"d": 0.7, "p": 0.0})
    _assert_formula(m, base, [(facs_d, None, 0.7)])
    ls.set_scale("p", -0.9)
    assert all(torch.equal(v, both[k]) for k, v in m.state_dict().items())
    ls.unload("d")
    _assert_formula(m, base, [(facs_p, None, -0.9)])
    ls.unload_all()
    assert all(torch.equal(v, base[k]) for k, v in m.state_dict().items())


def test_conv_targets_are_opt_in_and_dora_on_linears_applies_by_default():
    m = _model()
    base = {k: v.clone() for k, v in m.state_dict().items()}
    lin = _shapes(m, nn.Linear)
    ls = lora.LoraSet(m)
    sd, facs = _adapter(m, 4, 5, dora=True)
    conv_keys = [k for k in sd if any(("lora_unet_" + n.replace(".", "_") + ".") in k for n, s in _shapes(m).items() if len(s) == 4)]
    with pytest.raises(ValueError, match="conv_in") as exc:
        ls.load("a", sd)                                               # strict, convs=False: refused, and the error says how
    assert "pass convs=True" in str(exc.value)
    assert ls.names() == [] and all(torch.equal(v, base[k]) for k, v in m.state_dict().items())
    left = ls.load("a", sd, strict=False)
    assert sorted(left) == sorted(conv_keys) and sorted(ls.adapted_modules()) == sorted(lin)
    _assert_formula(m, base, [({n: f for n, f in facs.items() if n in lin}, None, 1.0)])
    assert all(torch.equal(v, base[k]) for k, v in m.state_dict().items() if base[k].dim() == 4), "no conv weight moved"
    ls.unload("a")
    sd_lin = {k: v for k, v in sd.items() if k not in conv_keys}
    assert ls.load("b", sd_lin) == []                                  # DoRA keys on Linear targets no longer fail a strict load
    assert lora.target_linears(m).keys() == lin.keys()
    assert list(lora.target_modules(m, convs=False)) == list(lin) and sorted(lora.target_modules(m, convs=True)) == sorted(_shapes(m))


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_dora_merge(lib):
    """The DoRA merge is st_lora_merge with a norm pass: its own entry point is gone."""
    assert lib.st_abi_version() == 18 == _C.ABI_VERSION
    assert hasattr(lib, "st_lora_merge") and "st_lora_merge" in _C.SIGNATURES
    assert not hasattr(lib, "st_lora_merge_dora") and "st_lora_merge_dora" not in _C.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stabletriton_amd.h")).read()
    assert re.search(r"\bint st_lora_merge\(", header) and not re.search(r"\bint st_lora_merge_dora\(", header)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path()], capture_output=True, text=True).stdout
    assert re.search(r" T st_lora_merge\b", out) and not re.search(r" T st_lora_merge_dora\b", out)
    # argument validation happens on the host, before any launch
    bf = _C.ST_BF16
    assert lib.st_lora_merge(None, 1, None, 1, 32, None, 1, None, 0, None, 8, None, 0, bf, 0, None) != 0 and b"null" in lib.st_last_error()
    assert lib.st_lora_merge(8, 1, 8, 1, 32, 8, 1, 8, 2, 8, 8, 8, 64, bf, 0, None) != 0 and b"norm tiles" in lib.st_last_error()
    assert lib.st_lora_merge(8, 1, 8, 1, 32, 8, 1, 8, 1, 8, 8, None, 0, bf, 0, None) != 0 and b"workspace" in lib.st_last_error()
    assert lib.st_lora_merge(8, 1, 8, 1, 256, 8, 1, 8, 1, 8, 8, 8, 64, bf, 0, None) != 0 and b"max_rank" in lib.st_last_error()
    assert lib.st_lora_merge(8, 1, 8, 1, 32, 8, 1, 8, 1, 8, 8, 8, 64, 7, 0, None) != 0 and b"dtype" in lib.st_last_error()


def test_zero_row_takes_gain_zero():
    """A row of V that is exactly zero (zero base row, zero up row) has no norm to divide by: gain 0, the row stays zero."""
    torch.manual_seed(3)
    net = nn.Sequential(nn.Linear(6, 4, bias=False)).requires_grad_(False)
    net[0].weight[1].zero_()
    base = net[0].weight.clone()
    up = torch.randn(4, 2)
    up[1] = 0
    sd = {"0.lora_A.weight": torch.randn(2, 6), "0.lora_B.weight": up, "0.lora_magnitude_vector": torch.full((4,), 2.0)}
    ls = lora.LoraSet(net)
    ls.load("a", sd)
    w = net[0].weight
    assert bool(torch.isfinite(w).all()) and bool((w[1] == 0).all())
    assert float((w.double().norm(dim=1)[[0, 2, 3]] - 2.0).abs().max()) <= 1e-5
    ls.unload("a")
    assert torch.equal(w, base)

