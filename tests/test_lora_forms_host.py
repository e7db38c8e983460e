"""LyCORIS forms (Tucker LoCon, LoHa, Tucker LoHa, LoKr) without a GPU: parsing under kohya / LyCORIS keys, every refusal with
the weights left unwritten, the opt-in, the host contraction of Tucker cores, and LoraSet's torch route (`_merge_torch`, the
kernel's formula) on fp32 CPU modules against the float64 restatement of lora_forms_util.py.

Tolerance of the fp32 route: an element is built from at most 24 + 24 products per LoHa pair, 16 per Tucker contraction, the
elementwise product, the scale's fma and the final sums - under 80 fp32 roundings (u = 2^-24) of quantities bounded by
A = |B| + sum_j |s_j| |D_j| up to the cancellation inside a dot product, for which a factor 4 is allowed over the weight's
largest A: |W - W64| <= 320 u max(A) (2e-5 max(A)), times the largest DoRA gain, plus the gain's own relative error
(K / 2 + 80) u |W64| with magnitudes."""
import os
import re
import subprocess

import pytest
import torch
from torch import nn

import lora_forms_util as lf
from stabletriton_amd import _C, lora
from stabletriton_amd.build import lib_path

U = 2.0 ** -24
# the (N, K) views of test_lora_forms_gpu.py as modules: name -> (module, LoKr (a, b))
AB = {"lin": (4, 8), "odd": (5, 7), "conv": (8, 16), "conv_in": (2, 4), "wide": (8, 48)}
FORMS = ["tucker", "loha", "loha_tucker", "lokr", "lokr_w2fac", "lokr_w1fac", "lokr_bothfac", "lokr_tucker"]


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(328, 72)
        self.odd = nn.Linear(77, 50, bias=False)
        self.conv = nn.Conv2d(128, 192, 3, padding=1)
        self.conv_in = nn.Conv2d(4, 130, 3, padding=1)
        self.wide = nn.Linear(2304, 64)


def _net(channels_last=True):
    torch.manual_seed(0)
    m = Net().eval().requires_grad_(False)
    return m.to(memory_format=torch.channels_last) if channels_last else m


def _shapes(m):
    return {n: tuple(l.weight.shape) for n, l in m.named_modules() if isinstance(l, (nn.Linear, nn.Conv2d))}


def _adapter(m, form, seed, dora=False, alpha=None, names=None):
    """(state dict, {module: parts}) of one form on the modules it fits (Tucker forms: the convs)."""
    g = torch.Generator().manual_seed(seed)
    sd, parts = {}, {}
    for n, shape in _shapes(m).items():
        if (names is not None and n not in names) or ("tucker" in form and len(shape) != 4):
            continue
        p = lf.make(form, shape, g, rank=4, std=0.3, alpha=alpha, ab=AB[n], rank2=6)
        if dora:
            w = dict(m.named_modules())[n].weight
            p["dora_scale"] = (w.detach().reshape(shape[0], -1).norm(dim=1) * (0.5 + torch.rand(shape[0], generator=g))
                               ).reshape(-1, *([1] * (len(shape) - 1)))
        parts[n] = p
        sd.update(lf.keyed(n, p))
    return sd, parts


# ------------------------------------------------------------------------------------------------ parsing
def test_forms_are_refused_unless_asked_for():
    m = _net()
    for form, word in (("tucker", "Tucker"), ("loha", "LoHa"), ("lokr", "LoKr")):
        sd, _ = _adapter(m, form, 1)
        with pytest.raises(ValueError, match=word):
            lora.parse_adapter(sd, _shapes(m))
        with pytest.raises(ValueError, match="lycoris=True"):
            lora.parse_lora_state_dict(sd, _shapes(m).keys())
        before = {k: v.clone() for k, v in m.state_dict().items()}
        with pytest.raises(ValueError, match="lycoris=True"):
            lora.LoraSet(m).load("x", sd, convs=True)
        assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize("form", FORMS)
def test_parse_places_every_form_on_linear_and_conv_targets(form):
    m = _net()
    sd, parts = _adapter(m, form, 2, dora=True, alpha=2.0)
    sd["lora_te1_text_model_encoder_layers_0_mlp_fc1.hada_w1_a"] = torch.zeros(4, 4)
    placed, unplaced = lora.parse_adapter(sd, _shapes(m), lycoris=True)
    assert unplaced == ["lora_te1_text_model_encoder_layers_0_mlp_fc1.hada_w1_a"]
    assert sorted(placed) == sorted(parts) and ("conv" in placed) and (("lin" in placed) == ("tucker" not in form))
    want = {"tucker": "tucker", "loha": "loha", "loha_tucker": "loha"}.get(form, "lokr")
    for n, p in placed.items():
        assert p.form == want and p.alpha == 2.0 and p.magnitude is parts[n]["dora_scale"]
        if want == "tucker":
            assert p.down is parts[n]["lora_down.weight"] and p.up is parts[n]["lora_up.weight"] and p.parts["lora_mid"] is parts[n]["lora_mid.weight"]
        else:
            assert p.down is None and p.up is None
            assert {k: v for k, v in parts[n].items() if k not in ("alpha", "dora_scale")}.keys() == p.parts.keys()
            assert all(p.parts[k] is parts[n][k] for k in p.parts)
    # the Linear names alone: conv keys name no target (reported, as LoCon keys are), and a conv target needs convs=True
    lin_only = {n: s for n, s in _shapes(m).items() if len(s) == 2}
    placed, unplaced = lora.parse_adapter(sd, lin_only, lycoris=True)
    assert all(len(_shapes(m)[n]) == 2 for n in placed) and any("conv" in k for k in unplaced)
    with pytest.raises(ValueError, match="pass convs=True"):
        lora.LoraSet(m).load("x", {k: v for k, v in sd.items() if not k.startswith("lora_te")}, lycoris=True)
    # a missing alpha is kept as missing (the scalar in front is then 1); the `.weight` spelling of the keys is read too
    sd2, _ = _adapter(m, form, 2)
    placed, _ = lora.parse_adapter({(k if k.endswith(".weight") else k + ".weight"): v for k, v in sd2.items()}, _shapes(m), lycoris=True)
    assert placed and all(p.alpha is None or p.form == "tucker" for p in placed.values())


def _refusals(m):
    g = torch.Generator().manual_seed(3)
    shapes = _shapes(m)
    mk = lambda form, n, **kw: lf.make(form, shapes[n], g, rank=kw.pop("rank", 4), ab=AB[n], **kw)      # noqa: E731
    drop = lambda p, *ks: {k: v for k, v in p.items() if k not in ks}                                      # noqa: E731
    cases = [("incomplete LoHa", lf.keyed("lin", drop(mk("loha", "lin"), "hada_w2_a", "hada_w2_b"))),
             ("incomplete LoHa", lf.keyed("conv", drop(mk("loha_tucker", "conv"), "hada_t2"))),
             ("incomplete LoKr", lf.keyed("lin", drop(mk("lokr", "lin"), "lokr_w2"))),
             ("incomplete LoKr", lf.keyed("lin", drop(mk("lokr_w2fac", "lin"), "lokr_w2_b"))),
             ("incomplete LoKr", lf.keyed("conv", drop(mk("lokr_tucker", "conv"), "lokr_w2_a", "lokr_w2_b"))),
             ("incomplete adapter", lf.keyed("conv", drop(mk("tucker", "conv"), "lora_up.weight"))),
             ("mixes factorisations", {**lf.keyed("lin", mk("loha", "lin")), **lf.keyed("lin", mk("lokr", "lin"))}),
             ("mixes factorisations", {**lf.keyed("lin", mk("lokr", "lin")), lf.stem("lin") + ".lora_down.weight": torch.zeros(4, 328),
                                       lf.stem("lin") + ".lora_up.weight": torch.zeros(72, 4)}),
             ("LoKr", lf.keyed("lin", {"lokr_w1": torch.zeros(5, 8), "lokr_w2": torch.zeros(14, 41)})),           # 5 does not divide 72
             ("LoKr", lf.keyed("lin", {"lokr_w1": torch.zeros(4, 8), "lokr_w2": torch.zeros(18, 40)})),           # b d != K
             ("LoKr", lf.keyed("conv", {"lokr_w1": torch.zeros(8, 16), "lokr_w2": torch.zeros(24, 8, 1, 1)})),    # the wrong kernel
             ("LoHa pair", lf.keyed("lin", {**mk("loha", "lin"), "hada_w2_b": torch.zeros(4, 327)})),
             ("LoHa pair", lf.keyed("conv", {**mk("loha", "conv"), "hada_w1_a": torch.zeros(191, 4)})),
             ("Tucker LoHa pair", lf.keyed("conv", {**mk("loha_tucker", "conv"), "hada_t1": torch.zeros(4, 4, 1, 1)})),
             ("Tucker LoCon", lf.keyed("conv", {**mk("tucker", "conv"), "lora_mid.weight": torch.zeros(4, 4, 1, 1)})),
             ("Tucker core", lf.keyed("lin", {"lora_down.weight": torch.zeros(4, 328), "lora_mid.weight": torch.zeros(4, 4, 1, 1),
                                              "lora_up.weight": torch.zeros(72, 4)})),
             ("rank 129", lf.keyed("lin", mk("loha", "lin", rank=129))),
             ("rank 129", lf.keyed("wide", mk("lokr_w2fac", "wide", rank=129))),
             ("rank 129", lf.keyed("conv", mk("tucker", "conv", rank=129))),
             ("input axis", {**lf.keyed("lin", mk("loha", "lin")), lf.stem("lin") + ".dora_scale": torch.ones(1, 328)}),
             ("magnitude", {**lf.keyed("lin", mk("lokr", "lin")), lf.stem("lin") + ".dora_scale": torch.ones(71, 1)})]
    return cases


def test_every_refusal_leaves_the_weights_unwritten():
    m = _net()
    good, _ = _adapter(m, "lokr", 4, names=["odd"])
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ls = lora.LoraSet(m)
    for match, sd in _refusals(m):
        with pytest.raises(ValueError, match=match):
            lora.parse_adapter(sd, _shapes(m), lycoris=True)
        with pytest.raises(ValueError, match=match):
            ls.load("x", {**good, **sd}, convs=True, lycoris=True)          # a good module beside the bad one is not written either
        assert ls.names() == [] and ls.adapted_modules() == []
        assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items()), match
    assert ls.load("x", good, lycoris=True) == [] and not torch.equal(m.odd.weight, before["odd.weight"])
    ls.unload("x")
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


# ------------------------------------------------------------------------------------------------ the host contraction
@pytest.mark.parametrize("nhwc", [True, False])
def test_tucker_core_contraction_vs_float64_einsum(nhwc):
    g = torch.Generator().manual_seed(5)
    core, down = torch.randn(6, 5, 3, 3, generator=g), torch.randn(5, 20, generator=g)
    got = lora.contract_core(core, down, nhwc)
    want = torch.einsum("abyx,bi->ayxi" if nhwc else "abyx,bi->aiyx", core.double(), down.double()).reshape(6, -1)
    assert got.dtype == torch.float32 and got.shape == (6, 180)
    # 5 products and 4 additions in fp32 per element
    bound = 6 * U * torch.einsum("abyx,bi->ayxi" if nhwc else "abyx,bi->aiyx", core.double().abs(), down.double().abs()).reshape(6, -1)
    assert bool(((got.double() - want).abs() <= bound).all())
    # the K order is the weight view's: contracting, then multiplying by up, is the Tucker delta in that view
    w = torch.zeros(7, 20, 3, 3)
    w = w.to(memory_format=torch.channels_last) if nhwc else w
    rows, is_nhwc = lora.weight_rows(w)
    assert is_nhwc == nhwc
    up = torch.randn(7, 6, generator=g)
    rows.copy_(up @ got)
    want4 = torch.einsum("oa,abyx,bi->oiyx", up.double(), core.double(), down.double())
    assert float((w.double() - want4).abs().max()) <= 1e-5 * float(want4.abs().max())


# ------------------------------------------------------------------------------------------------ the torch route
@pytest.mark.parametrize("channels_last", [True, False], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("dora", [False, True], ids=["plain", "dora"])
@pytest.mark.parametrize("form", FORMS)
def test_merge_torch_vs_float64(form, dora, channels_last):
    m = _net(channels_last)
    base = {n: dict(m.named_modules())[n].weight.detach().double().clone() for n in _shapes(m)}
    sd, parts = _adapter(m, form, 6, dora=dora, alpha=3.0)
    sd_l, parts_l = _adapter(m, "loha", 7, alpha=None)                         # a second, different kind on the same weights
    ls = lora.LoraSet(m)
    assert ls.load("a", sd, 0.75, convs=True, lycoris=True) == []
    assert ls.load("b", sd_l, -1.5, convs=True, lycoris=True) == []
    for n, b in base.items():
        stack = [(p[n], s) for p, s in ((parts, 0.75), (parts_l, -1.5)) if n in p]
        want = lf.merged64(b, stack)
        mag, gmax = lf.abs_terms64(b, stack)
        tol = 320 * U * float(mag.max()) * gmax + ((b[0].numel() / 2 + 80) * U * want.abs() if dora else 0.0)
        got = dict(m.named_modules())[n].weight.detach().double()
        err = (got - want).abs()
        assert bool((err <= tol).all()), f"{form} {n}: max err {float(err.max()):.3e}"
        assert float((want - b).abs().max()) > 1e3 * float(torch.as_tensor(tol).max()), "the adapter must matter"
    ls.set_scales({"a": 0.0, "b": 0.0})
    assert all(torch.equal(dict(m.named_modules())[n].weight.double(), b) for n, b in base.items())
    ls.unload_all()
    assert all(torch.equal(dict(m.named_modules())[n].weight.double(), b) for n, b in base.items())


def test_mixed_kinds_stack_in_load_order():
    """A plain LoRA, a LoHa and a LoKr (with DoRA) on the same weights."""
    m = _net()
    g = torch.Generator().manual_seed(8)
    base = {n: dict(m.named_modules())[n].weight.detach().double().clone() for n in _shapes(m)}
    plain = {n: {"lora_down.weight": torch.randn(8, *s[1:], generator=g) * 0.1,
                 "lora_up.weight": torch.randn(s[0], 8, *([1, 1] if len(s) == 4 else []), generator=g) * 0.1, "alpha": torch.tensor(4.0)}
             for n, s in _shapes(m).items()}
    sd_h, parts_h = _adapter(m, "loha", 9, alpha=2.0)
    sd_k, parts_k = _adapter(m, "lokr_w2fac", 10, dora=True, alpha=2.0)
    ls = lora.LoraSet(m)
    ls.load("p", {k: v for n, p in plain.items() for k, v in lf.keyed(n, p).items()}, 0.75, convs=True)
    ls.load("h", sd_h, -1.5, convs=True, lycoris=True)
    ls.load("k", sd_k, 0.3, convs=True, lycoris=True)
    for n, b in base.items():
        stack = [(plain[n], 0.75), (parts_h[n], -1.5), (parts_k[n], 0.3)]
        want = lf.merged64(b, stack)
        mag, gmax = lf.abs_terms64(b, stack)
        tol = 320 * U * float(mag.max()) * gmax + (b[0].numel() / 2 + 80) * U * want.abs()
        assert bool(((dict(m.named_modules())[n].weight.double() - want).abs() <= tol).all()), n


def test_library_exports_the_forms_entry_point():
    """LoHa and LoKr segments go through st_lora_merge with `forms` set: their own entry point is gone."""
    lib = _C.load()
    assert hasattr(lib, "st_lora_merge") and "st_lora_merge" in _C.SIGNATURES
    assert not hasattr(lib, "st_lora_merge_forms") and "st_lora_merge_forms" not in _C.SIGNATURES
    assert lib.st_abi_version() == 18 == _C.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stabletriton_amd.h")).read()
    assert re.search(r"\bint st_lora_merge\(", header) and not re.search(r"\bint st_lora_merge_forms\(", header)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path()], capture_output=True, text=True).stdout
    assert re.search(r" T st_lora_merge\b", out) and not re.search(r" T st_lora_merge_forms\b", out)
