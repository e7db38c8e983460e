"""LoRA adapters without a GPU: the state-dict parser, and LoraSet on a CPU fp32 TINY module (torch merge, same formula)."""
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


def _model():
    m = UNet2DConditionModel(TINY).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def _linear_shapes(m):
    return {n: tuple(l.weight.shape) for n, l in m.named_modules() if isinstance(l, nn.Linear)}


def _factors(shapes, rank, seed, names=None):
    """name -> (down (r, K), up (N, r)), seeded."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, (N, K) in shapes.items():
        if names is not None and n not in names:
            continue
        out[n] = (torch.randn(rank, K, generator=g) * 0.1, torch.randn(N, rank, generator=g) * 0.1)
    return out


def _peft(facs, prefix="unet.", alpha=None):
    sd = {}
    for n, (down, up) in facs.items():
        sd[f"{prefix}{n}.lora_A.weight"] = down
        sd[f"{prefix}{n}.lora_B.weight"] = up
        if alpha is not None:
            sd[f"{prefix}{n}.alpha"] = torch.tensor(float(alpha))
    return sd


def _old_diffusers(facs, processor):
    """Attention projections as `<attn>[.processor].to_q_lora.down.weight`; everything else as `<path>.lora.down.weight`."""
    sd = {}
    for n, (down, up) in facs.items():
        m = re.match(r"^(.+\.attn[12])\.(to_q|to_k|to_v|to_out)(\.0)?$", n)
        if m:
            stem = f"unet.{m[1]}{'.processor' if processor else ''}.{m[2]}_lora"
        else:
            stem = f"unet.{n}.lora"
        sd[f"{stem}.down.weight"] = down
        sd[f"{stem}.up.weight"] = up
    return sd


def _kohya(facs, alpha=None):
    sd = {}
    for n, (down, up) in facs.items():
        stem = "lora_unet_" + n.replace(".", "_")
        sd[f"{stem}.lora_down.weight"] = down
        sd[f"{stem}.lora_up.weight"] = up
        if alpha is not None:
            sd[f"{stem}.alpha"] = torch.tensor(float(alpha))
    return sd


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_places_three_spellings_on_the_same_modules():
    shapes = _linear_shapes(_model())
    facs = _factors(shapes, 4, 1)
    assert any("to_out.0" in n for n in facs) and any("ff.net.0.proj" in n for n in facs) and "time_embedding.linear_1" in facs
    forms = {"peft": _peft(facs), "peft, no prefix": _peft(facs, prefix=""), "old, processor": _old_diffusers(facs, True),
             "old": _old_diffusers(facs, False), "kohya": _kohya(facs)}
    for what, sd in forms.items():
        placed, unplaced = lora.parse_lora_state_dict(sd, shapes.keys())
        assert unplaced == [], what
        assert sorted(placed) == sorted(facs), what
        for n, (down, up, alpha) in placed.items():
            assert torch.equal(down, facs[n][0]) and torch.equal(up, facs[n][1]), f"{what}: {n}"
            assert alpha == 4.0, f"{what}: alpha defaults to the rank"


def test_parser_alpha_and_peft_adapter_names():
    shapes = _linear_shapes(_model())
    facs = _factors(shapes, 8, 2, names={"mid_block.attentions.0.transformer_blocks.0.attn1.to_q", "add_embedding.linear_2"})
    for sd in (_kohya(facs, alpha=2), _peft(facs, alpha=2)):
        placed, unplaced = lora.parse_lora_state_dict(sd, shapes.keys())
        assert unplaced == [] and sorted(placed) == sorted(facs)
        assert all(a == 2.0 for _, _, a in placed.values())
    sd = {k.replace(".lora_A.", ".lora_A.default.").replace(".lora_B.", ".lora_B.default."): v for k, v in _peft(facs).items()}
    placed, unplaced = lora.parse_lora_state_dict(sd, shapes.keys())
    assert unplaced == [] and sorted(placed) == sorted(facs)


def test_kohya_names_resolve_against_the_model_not_by_guessing():
    """`to_out_0`, `ff_net_0_proj`, `time_emb_proj` hold underscores of their own: only the model's names settle them."""
    shapes = _linear_shapes(_model())
    for n in ("down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_out.0", "down_blocks.1.attentions.0.transformer_blocks.0.ff.net.0.proj",
              "down_blocks.0.resnets.0.time_emb_proj", "up_blocks.0.attentions.2.proj_in"):
        facs = _factors(shapes, 4, 3, names={n})
        placed, unplaced = lora.parse_lora_state_dict(_kohya(facs), shapes.keys())
        assert list(placed) == [n] and unplaced == []


def test_parser_reports_conv_and_text_encoder_keys():
    m = _model()
    shapes = _linear_shapes(m)
    facs = _factors(shapes, 4, 4, names={"mid_block.attentions.0.proj_out"})
    sd = _kohya(facs)
    conv = {"lora_unet_down_blocks_0_resnets_0_conv1.lora_down.weight": torch.zeros(4, 64, 3, 3),
            "lora_unet_down_blocks_0_resnets_0_conv1.lora_up.weight": torch.zeros(64, 4, 1, 1),
            "unet.conv_in.lora_A.weight": torch.zeros(4, 4, 3, 3), "unet.nowhere.to_q.lora_A.weight": torch.zeros(4, 4)}
    te = {"lora_te1_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": torch.zeros(4, 8),
          "text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight": torch.zeros(4, 8),
          "text_encoder_2.text_model.encoder.layers.0.mlp.fc1.lora_B.weight": torch.zeros(8, 4)}
    sd.update(conv)
    sd.update(te)
    placed, unplaced = lora.parse_lora_state_dict(sd, shapes.keys())
    assert list(placed) == ["mid_block.attentions.0.proj_out"]
    assert sorted(unplaced) == sorted(list(conv) + list(te))
    assert all(lora.is_text_encoder_key(k) for k in te) and not any(lora.is_text_encoder_key(k) for k in conv)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ls = lora.LoraSet(m)
    with pytest.raises(ValueError, match="conv1"):
        ls.load("a", sd)                                           # strict: conv keys refuse, nothing is written
    assert ls.names() == [] and all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    left = ls.load("a", sd, strict=False)
    assert sorted(left) == sorted(list(conv) + list(te)) and ls.adapted_modules() == ["mid_block.attentions.0.proj_out"]
    ls.unload("a")
    only_te = dict(_kohya(facs), **te)
    assert sorted(ls.load("b", only_te)) == sorted(te)             # text-encoder keys are reported, never an error


def test_errors_are_raised_before_any_write():
    m = _model()
    shapes = _linear_shapes(m)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ls = lora.LoraSet(m)
    good = _factors(shapes, 4, 5)
    name = "mid_block.attentions.0.transformer_blocks.1.ff.net.2"
    N, K = shapes[name]

    def with_bad(down, up):
        f = dict(good)
        f[name] = (down, up)
        return _peft(f)

    with pytest.raises(ValueError, match=re.escape(name)):
        ls.load("a", with_bad(torch.zeros(4, K + 1), torch.zeros(N, 4)))
    with pytest.raises(ValueError, match=re.escape(name)):
        ls.load("a", with_bad(torch.zeros(4, K), torch.zeros(N, 5)))
    with pytest.raises(ValueError, match=re.escape(name)):
        ls.load("a", with_bad(torch.zeros(4, K), torch.zeros(N + 1, 4)))
    with pytest.raises(ValueError, match="rank 129"):
        ls.load("a", with_bad(torch.zeros(129, K), torch.zeros(N, 129)))
    with pytest.raises(ValueError, match="incomplete"):
        sd = _peft(good)
        del sd[f"unet.{name}.lora_B.weight"]
        ls.load("a", sd)
    with pytest.raises(ValueError, match="two down"):
        ls.load("a", dict(_peft(good), **_kohya({name: good[name]})))
    with pytest.raises(ValueError, match="no key"):
        ls.load("a", {"lora_te1_x.lora_down.weight": torch.zeros(2, 2)})
    assert ls.names() == [] and ls.adapted_modules() == []
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    ls.load("a", _peft(good))
    merged = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="already loaded"):
        ls.load("a", _peft(good))
    with pytest.raises(KeyError):
        ls.set_scale("b", 1.0)
    with pytest.raises(KeyError):
        ls.set_scales({"a": 0.5, "b": 1.0})                        # all or nothing
    with pytest.raises(KeyError):
        ls.unload("b")
    assert ls.scales() == {"a": 1.0} and all(torch.equal(v, merged[k]) for k, v in m.state_dict().items())
    for i in range(lora.MAX_ADAPTERS - 1):
        ls.load(f"x{i}", _peft(_factors(shapes, 2, 10 + i, names={name})))
    with pytest.raises(ValueError, match=f"at most {lora.MAX_ADAPTERS}"):
        ls.load("one too many", _peft(good))


# ------------------------------------------------------------------------------------------------ LoraSet on the CPU
FP32 = (24, -126)


def _spacing32(x64):
    _, e = torch.frexp(x64.abs())
    e = torch.where(x64 == 0, torch.full_like(e, FP32[1]), e - 1).clamp_min(FP32[1])
    return torch.ldexp(torch.ones_like(x64), e - (FP32[0] - 1))


def _assert_float64_formula(m, base, adapters):
    """adapters: [(facs, alpha, scale)].  |W - W64| <= 1/2 spacing(W64) + (sum r + 3) 2^-24 (|Base| + sum |s| |Up| |Down|), every element."""
    worst = 0.0
    for n, l in m.named_modules():
        if not isinstance(l, nn.Linear):
            continue
        w64 = base[n + ".weight"].double()
        mag = w64.abs()
        sum_r = 0
        for facs, alpha, s in adapters:
            if n not in facs:
                continue
            down, up = facs[n]
            r = down.shape[0]
            sum_r += r
            w64 = w64 + s * (alpha / r) * (up.double() @ down.double())
            mag = mag + abs(s) * (alpha / r) * (up.double().abs() @ down.double().abs())
        bound = 0.5 * _spacing32(w64) + (sum_r + 3) * 2.0 ** -24 * mag
        err = (l.weight.double() - w64).abs()
        assert int((err > bound).sum()) == 0, f"{n}: outside the bound"
        worst = max(worst, float((err / bound).max()))
    print(f"worst |W - W64| / bound = {worst:.3f}")


def test_loraset_round_trip_is_bit_exact_and_matches_float64():
    m = _model()
    shapes = _linear_shapes(m)
    base = {k: v.clone() for k, v in m.state_dict().items()}
    ls = lora.attach(m)
    assert lora.attach(m) is ls
    facs = _factors(shapes, 16, 6)
    versions = {n: l.weight._version for n, l in m.named_modules() if isinstance(l, nn.Linear)}
    assert ls.load("style", _kohya(facs, alpha=8), scale=0.8) == []
    assert ls.names() == ["style"] and ls.scales() == {"style": 0.8} and sorted(ls.adapted_modules()) == sorted(shapes)
    assert all(l.weight._version > versions[n] for n, l in m.named_modules() if isinstance(l, nn.Linear)), "version counters must move"
    assert not any(torch.equal(m.state_dict()[n + ".weight"], base[n + ".weight"]) for n in shapes)
    _assert_float64_formula(m, base, [(facs, 8.0, 0.8)])
    at_08 = {k: v.clone() for k, v in m.state_dict().items()}
    ls.set_scale("style", -1.3)
    _assert_float64_formula(m, base, [(facs, 8.0, -1.3)])
    ls.set_scale("style", 0.8)
    assert all(torch.equal(v, at_08[k]) for k, v in m.state_dict().items()), "returning to a scale must return the bits"
    ls.set_scale("style", 0.0)
    assert all(torch.equal(v, base[k]) for k, v in m.state_dict().items()), "scale 0 is the base"
    ls.set_scale("style", 0.8)
    ls.unload("style")
    assert ls.names() == [] and ls.adapted_modules() == []
    assert all(torch.equal(v, base[k]) for k, v in m.state_dict().items()), "unload restores the state dict bit for bit"
    assert sorted(m.state_dict()) == sorted(base)


def test_two_adapters_commute_and_unload_one_keeps_the_other():
    shapes = _linear_shapes(_model())
    attn = {n for n in shapes if ".attn" in n}
    time_path = {n for n in shapes if "time_emb" in n or "embedding" in n}
    fa, fb = _factors(shapes, 4, 7, names=attn | time_path), _factors(shapes, 32, 8, names=attn)
    ma, mb = _model(), _model()
    base = {k: v.clone() for k, v in ma.state_dict().items()}
    la, lb = lora.LoraSet(ma), lora.LoraSet(mb)
    la.load("a", _peft(fa), 0.5)
    la.load("b", _kohya(fb, alpha=16), -0.75)
    lb.load("b", _kohya(fb, alpha=16), -0.75)
    lb.load("a", _peft(fa), 0.5)
    _assert_float64_formula(ma, base, [(fa, 4.0, 0.5), (fb, 16.0, -0.75)])
    _assert_float64_formula(mb, base, [(fa, 4.0, 0.5), (fb, 16.0, -0.75)])
    # the same two adapters in either load order: the same weights up to the rounding of two fp32 sums, far inside the bound;
    # after either is unloaded both models hold the one-adapter weights, bit for bit
    la.unload("b")
    lb.unload("b")
    assert sorted(la.adapted_modules()) == sorted(attn | time_path)
    assert all(torch.equal(v, mb.state_dict()[k]) for k, v in ma.state_dict().items())
    _assert_float64_formula(ma, base, [(fa, 4.0, 0.5)])
    la.load("b", _kohya(fb, alpha=16), 1.0)
    la.set_scales({"a": 0.0, "b": 0.0})
    assert all(torch.equal(v, base[k]) for k, v in ma.state_dict().items())
    la.unload_all()
    assert la.names() == [] and all(torch.equal(v, base[k]) for k, v in ma.state_dict().items())


def test_global_scale_multiplies_every_adapter():
    m = _model()
    shapes = _linear_shapes(m)
    base = {k: v.clone() for k, v in m.state_dict().items()}
    facs = _factors(shapes, 8, 9, names={n for n in shapes if n.endswith("to_v")})
    ls = lora.LoraSet(m)
    ls.load("a", _peft(facs), 1.0)
    assert ls.set_global_scale(0.5) and not ls.set_global_scale(0.5)
    half = {k: v.clone() for k, v in m.state_dict().items()}
    ls.set_global_scale(1.0)
    ls.set_scale("a", 0.5)
    assert all(torch.equal(v, half[k]) for k, v in m.state_dict().items())
    _assert_float64_formula(m, base, [(facs, 8.0, 0.5)])


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_lora_merge(lib):
    assert lib.st_abi_version() == 18 == _C.ABI_VERSION
    assert hasattr(lib, "st_lora_merge") and "st_lora_merge" in _C.SIGNATURES
    header = open(os.path.join(ROOT, "include", "stabletriton_amd.h")).read()
    assert re.search(r"\bint st_lora_merge\(", header)
    assert f"ST_LORA_TILE_N = {_C.LORA_TILE_N}" in header and f"ST_LORA_TILE_K = {_C.LORA_TILE_K}" in header
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path()], capture_output=True, text=True).stdout
    assert re.search(r" T st_lora_merge\b", out)
    # argument validation happens on the host, before any launch
    # (targets, n, segments, n, max_rank, tiles, n, norm tiles, n, scales, n, workspace, bytes, dtype, forms, stream)
    assert lib.st_lora_merge(None, 1, None, 0, 0, None, 1, None, 0, None, 8, None, 0, _C.ST_BF16, 0, None) != 0 and b"null" in lib.st_last_error()
    assert lib.st_lora_merge(8, 1, 8, 1, 32, 8, 0, None, 0, 8, 8, None, 0, _C.ST_BF16, 0, None) != 0 and b"tiles" in lib.st_last_error()
    assert lib.st_lora_merge(8, 1, 8, 1, 256, 8, 1, None, 0, 8, 8, None, 0, _C.ST_BF16, 0, None) != 0 and b"max_rank" in lib.st_last_error()
    assert lib.st_lora_merge(8, 1, 8, 1, 32, 8, 1, None, 0, 8, 8, None, 0, 7, 0, None) != 0 and b"dtype" in lib.st_last_error()
