"""LoRA adapters, merged into the weights in place.

A step of the compiled UNet is launch-bound, so an adapter never runs as a side branch here: it is merged into the
`nn.Linear` weights the kernels already read, and a merged weight adds no launch.  Every merge REBUILDS the weight from a
snapshot of its base,

    W = round_to_dtype( fp32(Base) + sum_j scale_j * (Up_j @ Down_j) ),        Up_j = (alpha_j / rank_j) * up_j, folded at load

in one grouped launch over all adapted modules (`ops.lora_merge`, csrc/lora.hip).  Rebuilding instead of adding and
subtracting is what makes `unload` restore the base bit for bit, scale 0 equal the base, and a scale change free of drift in
16-bit models.  The weights keep their addresses, so captured graphs stay valid; the owner re-derives what was computed
from them (fused q|k|v, LayerNorm-folded projections, split images, the fp8 plan's e4m3 weights: `refresh_derived`).

`parse_adapter` reads the three spellings in the wild (PEFT / current diffusers, older diffusers, kohya);
`LoraSet` owns the state of one module; `attach(compiled)` returns the set of an `optimize_model` result.
`DenoiseLoop.load_lora` and the hooks' `load_lora` are thin wrappers over it.

DoRA: an adapter that carries a magnitude m (one value per output row / channel) renormalises the rows it touches,

    V_j = Base + s_j * Up_j @ Down_j,    g_j[n] = m_j[n] / ||V_j[n, :]||_2    (g_j = 1 for a plain adapter)
    W   = round_to_dtype( Base + sum_j (g_j (.) V_j - Base) )

which is PEFT's DoRA (the scale sits inside the norm); several adapters on one weight are each normalised against the base
alone, as PEFT's forward with several active adapters does.  An adapter whose effective scale is exactly 0 is skipped whole,
magnitude included, so scale 0 and `unload` still give the base's bits.  That is a jump at 0: PEFT's DoRA at scale 0 is
m / ||Base|| (.) Base, which a scale that merely approaches 0 approaches here too, and which is not Base.  A row of V_j that is
exactly zero has no direction (PEFT divides by zero there); its gain is 0 here, so the row's g_j (.) V_j stays the zero it was.

Scope: `nn.Linear` targets (attention projections, feed-forward, proj_in / proj_out, and the time-path Linears when an
adapter names them) and, with `convs=True`, `nn.Conv2d` targets (LoCon: conv_in / conv_out, the resnets' conv1 / conv2 /
conv_shortcut, the samplers' conv).  A conv weight (O, I, R, S) is merged through the 2-D view of its own memory - (O, R S I)
for the channels_last weights of an `optimize_model` result, (O, I R S) for a contiguous one - so the kernel sees it as it
sees a Linear.  Conv factors are down (r, I, R, S) with the target's kernel size and up (O, r, 1, 1).

With `lycoris=True` the other factorisations LyCORIS trainers write are applied too (conv targets still need `convs=True`).
Shapes as the trainers store them; a missing alpha makes the scalar in front 1; N x K stands for O x (I R S) on a conv:

    Tucker LoCon  lora_down (r, I, 1, 1), lora_mid (r, r, R, S), lora_up (O, r, 1, 1)
                  D[o,i,y,x] = (alpha / r) sum_ab up[o,a] mid[a,b,y,x] down[b,i]
    LoHa          hada_w1_a (N, r), hada_w1_b (r, K), hada_w2_a (N, r), hada_w2_b (r, K), K = I R S flattened in that order
                  D = (alpha / r) (w1_a w1_b) (.) (w2_a w2_b),   r = hada_w1_b.shape[0]
    Tucker LoHa   adds hada_t1, hada_t2 (r, r, R, S); hada_w?_a is (r, O), hada_w?_b (r, I)
                  W_m[o,i,y,x] = sum_pq t_m[p,q,y,x] w_m_a[p,o] w_m_b[q,i],   D = (alpha / r) W_1 (.) W_2
    LoKr          w1 = lokr_w1 (a, b) or lokr_w1_a (a, r) lokr_w1_b (r, b);
                  w2 = lokr_w2 (c, d[, R, S]), or lokr_w2_a (c, r) lokr_w2_b (r, d R S), or - Tucker - lokr_t2 (r, r, R, S) with
                  lokr_w2_a (r, c) and lokr_w2_b (r, d) contracted like a Tucker LoHa pair;   a c = O, b d = I
                  D[i c + p, j d + q, y, x] = sigma w1[i,j] w2[p,q,y,x];  sigma = alpha / r with r the rank of a factorised w2,
                  else of a factorised w1; sigma = 1 when both are stored full

What is scale-independent is done once at load, in fp32 on the weight's device (`build_factors`): a Tucker core is
contracted into its down factor (`contract_core`) and rounded to the storage dtype once, which leaves an ordinary factor
pair; LoKr's w1 (sigma folded in) and w2 become small fp32 tables that are never rounded to a 16-bit dtype; LoHa's
alpha / r is folded into its first up factor before rounding.  The kernel then forms each segment's delta by kind - a
product, the elementwise product of two products, or a Kronecker product - and everything after that (scales, DoRA,
stacking in load order, the final rounding) is shared, so a `dora_scale` along the output axis composes with every form and
the kinds mix on one weight.

Still refused: DoRA magnitudes along the input axis, full `diff` matrices, norm / bias adapters, (IA)^3, GLoRA, grouped or
dilated targets; text-encoder adapters are reported, not applied.
"""
from __future__ import annotations

import re
from collections import OrderedDict
from typing import Callable, Dict, Iterable, List, Mapping, NamedTuple, Optional, Tuple

import torch
from torch import nn

MAX_ADAPTERS = 8        # capacity of a LoraSet: the device scale table has this many slots and never moves
MAX_RANK = 128          # largest rank of one adapter on one module

_TEXT_ENCODER = re.compile(r"^(lora_te\d*_|text_encoder(_\d+)?\.|te\d*\.|lora_prior_te)")
_PEFT = re.compile(r"^(?P<path>.+)\.lora_(?P<ab>[AB])(?:\.[^.]+)?\.weight$")
_OLD_PROC = re.compile(r"^(?P<attn>.+?)\.(?:processor\.)?(?P<proj>to_q|to_k|to_v|to_out)_lora\.(?P<du>down|up)\.weight$")
_OLD_LAYER = re.compile(r"^(?P<path>.+)\.lora(?:_layer)?\.(?P<du>down|up)\.weight$")
_KOHYA = re.compile(r"^(?P<stem>lora_unet_[^.]+)\.(?P<what>lora_down\.weight|lora_up\.weight|alpha|dora_scale)$")
_PEFT_MAGNITUDE = re.compile(r"^(?P<path>.+)\.lora_magnitude_vector(?:\.[^.]+)?(?:\.weight)?$")
# factorisations that are applied only with `lycoris=True`: Tucker's core (`lora_mid`), LoHa (`hada_*`), LoKr (`lokr_*`)
_OTHER_FORMS = re.compile(r"^(?P<stem>.+?)\.(?P<what>lora_mid|hada_(?:w[12]_[ab]|t[12])|lokr_(?:w[12](?:_[ab])?|t2))(?:\.weight)?$")


def is_text_encoder_key(key: str) -> bool:
    return _TEXT_ENCODER.match(key) is not None


def _place(key: str, flat: Mapping[str, str], names, lycoris: bool = False) -> Optional[Tuple[str, str]]:
    """(module name, 'down' | 'up' | 'alpha' | 'magnitude') for one state-dict key, or None when the key names no target.  With
    `lycoris` also (module name, 'lora_mid' | 'hada_w1_a' | ... | 'lokr_t2'); without it such a key on a listed module raises."""
    m = _OTHER_FORMS.match(key)
    if m:
        stem = m["stem"]
        name = flat.get(stem[len("lora_unet_"):]) if stem.startswith("lora_unet_") else stem[len("unet."):] if stem.startswith("unet.") else stem
        if name in names:
            if lycoris:
                return name, m["what"]
            raise ValueError(f"{name}: {key!r} belongs to a Tucker (lora_mid), LoHa or LoKr factorisation, which is not supported "
                             "unless it is asked for: pass lycoris=True")
        return None
    m = _KOHYA.match(key)
    if m:
        name = flat.get(m["stem"][len("lora_unet_"):])
        what = {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha", "dora_scale": "magnitude"}[m["what"]]
        return (name, what) if name is not None else None
    if key.startswith("unet."):
        key = key[len("unet."):]
    m = _PEFT_MAGNITUDE.match(key)
    if m:
        return (m["path"], "magnitude") if m["path"] in names else None
    m = _PEFT.match(key)
    if m:
        return (m["path"], "down" if m["ab"] == "A" else "up") if m["path"] in names else None
    m = _OLD_PROC.match(key)
    if m:
        path = f"{m['attn']}.{m['proj']}" + (".0" if m["proj"] == "to_out" else "")
        return (path, m["du"]) if path in names else None
    m = _OLD_LAYER.match(key)
    if m:
        return (m["path"], m["du"]) if m["path"] in names else None
    if key.endswith(".alpha") and key[:-len(".alpha")] in names:
        return key[:-len(".alpha")], "alpha"
    return None


class Placed(NamedTuple):
    """What an adapter holds for one module: down (r, K) and up (N, r) - (r, I, R, S) and (O, r, 1, 1) for a convolution - its
    alpha, and its DoRA magnitude as the file holds it (None for a plain adapter).  `form` is "lora", or with `lycoris=True`
    "tucker" (down and up as usual, the core in `parts["lora_mid"]`), "loha" or "lokr" (down and up None, the file's tensors in
    `parts` under their key names, alpha None when the file has none)."""
    down: Optional[torch.Tensor]
    up: Optional[torch.Tensor]
    alpha: Optional[float]
    magnitude: Optional[torch.Tensor] = None
    form: str = "lora"
    parts: Optional[Dict[str, torch.Tensor]] = None


def parse_lora_state_dict(sd: Mapping[str, torch.Tensor], module_names, lycoris: bool = False):
    """`parse_adapter` in the form this function has always had: `placed[name] = (down, up, alpha)`.  DoRA magnitudes are placed
    and checked like everything else but are not part of the triples; `parse_adapter` returns them.

    Keys that name a listed module in a form the merge cannot apply RAISE ValueError; they are no longer reported as unplaced:
    Tucker (`lora_mid`), LoHa (`hada_*`) and LoKr (`lokr_*`) factors unless `lycoris=True` asks for them (their triples then
    hold None for the factors, see `Placed`), a `dora_scale` along the input axis or with the wrong first
    dimension, a magnitude without its factors.  Applying the rest of such a file would merge something its author never
    trained, so `strict=False` in `LoraSet.load` does not turn these into a list either; the same keys on modules that are
    not listed (a conv key with the Linear names alone) stay in `unplaced` as before."""
    placed, unplaced = parse_adapter(sd, module_names, lycoris=lycoris)
    return {n: (p.down, p.up, p.alpha) for n, p in placed.items()}, unplaced


_HADA = ("hada_w1_a", "hada_w1_b", "hada_w2_a", "hada_w2_b")


def _form_of(name: str, p: Mapping[str, torch.Tensor]) -> str:
    """Which factorisation the parts of one module are, complete and unmixed, or ValueError."""
    hada = sorted(k for k in p if k.startswith("hada_"))
    lokr = sorted(k for k in p if k.startswith("lokr_"))
    lora = sorted(k for k in p if k in ("down", "up", "lora_mid"))
    if sum(bool(x) for x in (hada, lokr, lora)) > 1:
        raise ValueError(f"{name}: the state dict mixes factorisations on one module: {hada + lokr + lora}")
    if hada:
        missing = [k for k in _HADA if k not in p]
        if missing or ("hada_t1" in p) != ("hada_t2" in p):
            raise ValueError(f"{name}: incomplete LoHa adapter, found only {hada} (it takes hada_w1_a/b and hada_w2_a/b, and "
                             "hada_t1 with hada_t2 or neither)")
        return "loha"
    if lokr:
        w1_full, w1_fac = "lokr_w1" in p, "lokr_w1_a" in p or "lokr_w1_b" in p
        w2_full, w2_fac = "lokr_w2" in p, "lokr_w2_a" in p or "lokr_w2_b" in p
        ok = (w1_full != w1_fac and w2_full != w2_fac and (not w1_fac or ("lokr_w1_a" in p and "lokr_w1_b" in p))
              and (not w2_fac or ("lokr_w2_a" in p and "lokr_w2_b" in p)) and ("lokr_t2" not in p or w2_fac))
        if not ok:
            raise ValueError(f"{name}: incomplete LoKr adapter, found only {lokr} (it takes lokr_w1 or lokr_w1_a/b, and lokr_w2 or "
                             "lokr_w2_a/b, the latter with or without lokr_t2)")
        return "lokr"
    if "down" not in p or "up" not in p:
        raise ValueError(f"{name}: incomplete adapter, found only {sorted(k for k in p if k != 'kohya_magnitude')}")
    return "tucker" if "lora_mid" in p else "lora"


def parse_adapter(sd: Mapping[str, torch.Tensor], module_names, lycoris: bool = False) -> Tuple[Dict[str, Placed], List[str]]:
    """Place a LoRA state dict on the modules named by `module_names`: the model's own `nn.Linear` (and, for conv adapters,
    `nn.Conv2d`) names, or a mapping from those names to the weights' shapes, with which every placed adapter is also checked
    against its target (`check_shapes`).

    Returns `(placed, unplaced)`: `placed[name] = Placed(down, up, alpha, magnitude)` - down (r, K) and up (N, r), or
    (r, I, R, S) and (O, r, 1, 1) for a convolution; magnitude None for a plain adapter - `unplaced` the keys that name no target
    (modules not listed, other networks, text encoders - `is_text_encoder_key` tells the latter apart).  Spellings:
      PEFT / diffusers      <path>.lora_A.weight, <path>.lora_B.weight  [, <path>.alpha]
                            <path>.lora_magnitude_vector[.<adapter>][.weight]
      older diffusers       <attn>.to_q_lora.down.weight / .up.weight, with or without `.processor`; <path>.lora.down.weight
      kohya / LyCORIS       lora_unet_<path with underscores>.lora_down.weight / .lora_up.weight / .alpha / .dora_scale
      LyCORIS, `lycoris`    <stem>.lora_mid, <stem>.hada_w1_a / _w1_b / _w2_a / _w2_b / _t1 / _t2,
                            <stem>.lokr_w1 / _w1_a / _w1_b / _w2 / _w2_a / _w2_b / _t2  (each with or without `.weight`)
    An optional `unet.` prefix is dropped.  kohya's underscores are resolved against the module names themselves
    (`name.replace(".", "_")`), never by guessing where the dots were.  `alpha` defaults to the rank.  A `dora_scale` along
    the input axis (first dimension 1, more than one element) and - unless `lycoris=True` - Tucker / LoHa / LoKr keys on a
    listed module are errors; with it they are placed (`Placed.form`, `Placed.parts`), and a set that is incomplete or mixes
    forms on one module is an error.
    A PEFT magnitude may have any shape of N elements; a kohya `dora_scale` has N (the rows of its up factor) as its first
    dimension, anything else is an error."""
    shapes = module_names if isinstance(module_names, Mapping) else None
    names = set(module_names)
    flat: Dict[str, str] = {}
    for n in names:
        f = n.replace(".", "_")
        if f in flat:
            raise ValueError(f"modules {flat[f]!r} and {n!r} have the same kohya name {f!r}")
        flat[f] = n
    parts: Dict[str, Dict[str, torch.Tensor]] = {}
    unplaced: List[str] = []
    for key, val in sd.items():
        hit = None if is_text_encoder_key(key) else _place(key, flat, names, lycoris)
        if hit is None:
            unplaced.append(key)
            continue
        name, what = hit
        slot = parts.setdefault(name, {})
        if what in slot:
            raise ValueError(f"{name}: the state dict holds two {what} entries (the second is {key!r})")
        if what == "magnitude" and key.endswith(".dora_scale") and val.dim() > 1 and val.shape[0] == 1 and val.numel() > 1:
            raise ValueError(f"{name}: {key!r} has shape {tuple(val.shape)}: a DoRA magnitude along the input axis (LyCORIS's "
                             "other decomposition) is not supported, only one value per output row / channel")
        slot[what] = val
        if what == "magnitude":
            slot["kohya_magnitude"] = key.endswith(".dora_scale")
    placed = {}
    for name, p in parts.items():
        form = _form_of(name, p)
        if form in ("loha", "lokr"):
            held = {k: v for k, v in p.items() if k.startswith(("hada_", "lokr_"))}
            placed[name] = Placed(None, None, float(p["alpha"]) if "alpha" in p else None, p.get("magnitude"), form, held)
            if p.get("kohya_magnitude") and p["magnitude"].dim() == 0:
                raise ValueError(f"{name}: a dora_scale has the output rows / channels as its first dimension; got a scalar")
            if shapes is not None:
                check_shapes(name, tuple(shapes[name]), None, None, p.get("magnitude"), form, held)
            continue
        down, up = p["down"], p["up"]
        if (form == "lora" and down.dim() == 4 and tuple(down.shape[2:]) == (1, 1) and up.dim() == 4
                and tuple(up.shape[2:]) == (1, 1)):
            down, up = down[:, :, 0, 0], up[:, :, 0, 0]          # a Linear that another exporter wrote as a 1x1 convolution
        alpha = float(p["alpha"]) if "alpha" in p else float(down.shape[0])
        held = {"lora_mid": p["lora_mid"]} if form == "tucker" else None
        placed[name] = Placed(down, up, alpha, p.get("magnitude"), form, held)
        if p.get("kohya_magnitude") and (p["magnitude"].dim() == 0 or p["magnitude"].shape[0] != up.shape[0]):
            raise ValueError(f"{name}: a dora_scale has the output rows / channels ({up.shape[0]}) as its first dimension; "
                             f"got shape {tuple(p['magnitude'].shape)}")
        if shapes is not None:
            check_shapes(name, tuple(shapes[name]), down, up, p.get("magnitude"), form, held)
    return placed, unplaced


def _check_rank(name: str, r: int) -> None:
    if r < 1 or r > MAX_RANK:
        raise ValueError(f"{name}: rank {r} is outside 1 .. {MAX_RANK}")


def _check_forms(name: str, weight_shape, form: str, down, up, parts) -> int:
    """The shape rules of the LyCORIS forms (the module docstring); returns the largest rank of any factor pair."""
    if len(weight_shape) == 4:
        o, i, kr, ks = weight_shape
    else:
        (o, i), kr, ks = weight_shape, 1, 1
    taps = kr * ks
    sh = lambda t: tuple(t.shape)                                             # noqa: E731

    def need(ok: bool, what: str, want: str):
        if not ok:
            got = ", ".join(f"{k} {sh(v)}" for k, v in sorted(parts.items()))
            raise ValueError(f"{name}: {what} of a {tuple(weight_shape)} weight takes {want}; got {got}")

    def tucker_pair(t, wa, wb, rows, cols, label):
        """core (p, q, R, S) with wa (p, rows) and wb (q, cols)"""
        need(t.dim() == 4 and wa.dim() == 2 and wb.dim() == 2 and sh(t) == (wa.shape[0], wb.shape[0], kr, ks)
             and wa.shape[1] == rows and wb.shape[1] == cols, label,
             f"a core (r, r, {kr}, {ks}) with factors (r, {rows}) and (r, {cols})")
        _check_rank(name, wa.shape[0])
        _check_rank(name, wb.shape[0])
        return max(wa.shape[0], wb.shape[0])

    if form == "tucker":
        mid = parts["lora_mid"]
        if len(weight_shape) != 4:
            raise ValueError(f"{name}: a Tucker core (lora_mid) belongs to a convolution, not to a {tuple(weight_shape)} weight")
        down2 = down[:, :, 0, 0] if down.dim() == 4 and sh(down)[2:] == (1, 1) else down
        up2 = up[:, :, 0, 0] if up.dim() == 4 and sh(up)[2:] == (1, 1) else up
        ok = down2.dim() == 2 and up2.dim() == 2 and mid.dim() == 4 and sh(mid) == (up2.shape[1], down2.shape[0], kr, ks) \
            and down2.shape[1] == i and up2.shape[0] == o and mid.shape[0] == mid.shape[1]
        if not ok:
            raise ValueError(f"{name}: a Tucker LoCon on a {(o, i, kr, ks)} conv weight takes down (r, {i}, 1, 1), mid (r, r, {kr}, {ks}) "
                             f"and up ({o}, r, 1, 1); got down {sh(down)}, mid {sh(mid)} and up {sh(up)}")
        _check_rank(name, down2.shape[0])
        return down2.shape[0]
    if form == "loha":
        rank = 0
        for m in "12":
            wa, wb, t = parts[f"hada_w{m}_a"], parts[f"hada_w{m}_b"], parts.get(f"hada_t{m}")
            if t is not None:
                rank = max(rank, tucker_pair(t, wa, wb, o, i, "a Tucker LoHa pair"))
            else:
                need(wa.dim() == 2 and wb.dim() == 2 and wa.shape[0] == o and wb.shape[1] == i * taps and wa.shape[1] == wb.shape[0],
                     "a LoHa pair", f"hada_w?_a ({o}, r) and hada_w?_b (r, {i * taps})")
                _check_rank(name, wb.shape[0])
                rank = max(rank, wb.shape[0])
        return rank
    if form == "lokr":
        rank = 0
        if "lokr_w1" in parts:
            w1 = parts["lokr_w1"]
            need(w1.dim() == 2, "LoKr", "a 2-D lokr_w1 (a, b)")
            a, b = sh(w1)
        else:
            wa, wb = parts["lokr_w1_a"], parts["lokr_w1_b"]
            need(wa.dim() == 2 and wb.dim() == 2 and wa.shape[1] == wb.shape[0], "LoKr", "lokr_w1_a (a, r) and lokr_w1_b (r, b)")
            _check_rank(name, wb.shape[0])
            (a, rank), b = sh(wa), wb.shape[1]
        need(a >= 1 and b >= 1 and o % a == 0 and i % b == 0, "LoKr", f"w1 (a, b) with a dividing {o} and b dividing {i}")
        c, d = o // a, i // b
        if "lokr_w2" in parts:
            w2 = parts["lokr_w2"]
            need(sh(w2) == (c, d, kr, ks) or (taps == 1 and sh(w2) == (c, d)), "LoKr", f"lokr_w2 ({c}, {d}, {kr}, {ks}) beside a w1 {(a, b)}")
        elif "lokr_t2" in parts:
            rank = max(rank, tucker_pair(parts["lokr_t2"], parts["lokr_w2_a"], parts["lokr_w2_b"], c, d, f"a Tucker LoKr w2 beside a w1 {(a, b)}"))
        else:
            wa, wb = parts["lokr_w2_a"], parts["lokr_w2_b"]
            need(wa.dim() == 2 and wb.dim() == 2 and wa.shape[1] == wb.shape[0] and wa.shape[0] == c and wb.shape[1] == d * taps,
                 "LoKr", f"lokr_w2_a ({c}, r) and lokr_w2_b (r, {d * taps}) beside a w1 {(a, b)}")
            _check_rank(name, wb.shape[0])
            rank = max(rank, wb.shape[0])
        return rank
    raise ValueError(f"{name}: unknown adapter form {form!r}")


def check_shapes(name: str, weight_shape, down: Optional[torch.Tensor], up: Optional[torch.Tensor],
                 magnitude: Optional[torch.Tensor] = None, form: str = "lora", parts: Optional[Mapping[str, torch.Tensor]] = None) -> int:
    """A Linear weight (N, K) takes up (N, r) and down (r, K); a conv weight (O, I, R, S) takes up (O, r, 1, 1) and down
    (r, I, R, S) (2-D factors stand for 1x1 ones); r at most MAX_RANK; a magnitude has N (O) elements (the parser
    also holds kohya's `dora_scale` to N as its first dimension).  Returns r.  The LyCORIS forms (`form`, `parts` of a
    `Placed`) follow the module docstring's shapes, every factor pair at most MAX_RANK; returns the largest rank."""
    if form != "lora":
        r = _check_forms(name, tuple(weight_shape), form, down, up, parts or {})
        n = weight_shape[0]
        if magnitude is not None and (magnitude.numel() != n or (magnitude.dim() > 1 and magnitude.shape[0] != n)):
            raise ValueError(f"{name}: a DoRA magnitude has one value per output row ({n}); got shape {tuple(magnitude.shape)}")
        return r
    if len(weight_shape) == 4:
        o, i, kr, ks = weight_shape
        down4 = down[:, :, None, None] if down.dim() == 2 else down
        up4 = up[:, :, None, None] if up.dim() == 2 else up
        if down4.dim() != 4 or up4.dim() != 4:
            raise ValueError(f"{name}: conv LoRA factors must be 4-D, got down {tuple(down.shape)} and up {tuple(up.shape)}")
        if tuple(down4.shape[2:]) != (kr, ks):
            raise ValueError(f"{name}: the down factor's kernel {tuple(down4.shape[2:])} differs from the convolution's {(kr, ks)}")
        r = down4.shape[0]
        ok = tuple(down4.shape) == (r, i, kr, ks) and tuple(up4.shape) == (o, r, 1, 1)
        n, want = o, f"a {(o, i, kr, ks)} conv weight takes down ({r}, {i}, {kr}, {ks}) and up ({o}, {r}, 1, 1)"
    else:
        n, k = weight_shape
        if down.dim() != 2 or up.dim() != 2:
            raise ValueError(f"{name}: LoRA factors must be 2-D, got down {tuple(down.shape)} and up {tuple(up.shape)}")
        r = down.shape[0]
        ok = tuple(down.shape) == (r, k) and tuple(up.shape) == (n, r)
        want = f"a ({n}, {k}) weight takes down ({r}, {k}) and up ({n}, {r})"
    if r < 1 or r > MAX_RANK:
        raise ValueError(f"{name}: rank {r} is outside 1 .. {MAX_RANK}")
    if not ok:
        raise ValueError(f"{name}: {want}; got down {tuple(down.shape)} and up {tuple(up.shape)}")
    if magnitude is not None and magnitude.numel() != n:
        raise ValueError(f"{name}: a DoRA magnitude has one value per output row ({n}); got shape {tuple(magnitude.shape)}")
    return r


def contract_core(core: torch.Tensor, down: torch.Tensor, nhwc: bool) -> torch.Tensor:
    """A Tucker core (p, q, R, S) contracted into its down factor (q, I), in fp32: down'[p, .] = sum_q core[p, q, y, x] down[q, i]
    as a (p, K) matrix whose K runs (y, x, i) for a channels_last conv weight (`nhwc`) and (i, y, x) for a contiguous one."""
    out = torch.einsum("pqyx,qi->pyxi" if nhwc else "pqyx,qi->piyx", core.float(), down.float())
    return out.reshape(core.shape[0], -1)


def _k_order(m: torch.Tensor, weight_shape, nhwc: bool) -> torch.Tensor:
    """A (rows, I R S) matrix with its columns in the K order of the weight's memory."""
    if len(weight_shape) == 4 and nhwc:
        _, i, kr, ks = weight_shape
        return m.reshape(m.shape[0], i, kr, ks).permute(0, 2, 3, 1).reshape(m.shape[0], -1)
    return m


def _padded_pair(up: torch.Tensor, down: torch.Tensor, like: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Up (N, rp), DownT (K, rp)) as the kernel takes them, from fp32 up (N, r) and down (r, K): each rounded to the storage
    dtype once, the rank zero-padded to the kernel's multiple."""
    r = down.shape[0]
    mult = 4 if like.dtype == torch.float32 else 32
    rp = -(-r // mult) * mult
    up_p = torch.zeros((up.shape[0], rp), dtype=like.dtype, device=like.device)
    down_t = torch.zeros((down.shape[1], rp), dtype=like.dtype, device=like.device)
    up_p[:, :r] = up.to(like.dtype)
    down_t[:, :r] = down.to(like.dtype).t()
    return up_p, down_t


class Factor(NamedTuple):
    """What the merge holds for one adapter on one weight (`build_factors`).  `kind` "plain": `tensors` (Up (N, rp), DownT (K, rp));
    "hada" (LoHa): (Up1, DownT1, Up2, DownT2); "kron" (LoKr): the fp32 tables (W1, W2) with the weight's `taps` and `layout`
    (`ops.lora_plan`).  Ranks are zero-padded; `magnitude` is the DoRA magnitude, (N,) fp32 on the weight's device, or None."""
    kind: str
    tensors: Tuple[torch.Tensor, ...]
    taps: int = 1
    layout: int = 0
    magnitude: Optional[torch.Tensor] = None

    def entry(self, slot: int) -> tuple:
        """The factor tuple `ops.lora_plan` takes for this record in scale slot `slot`."""
        mag = () if self.magnitude is None else (self.magnitude,)
        if self.kind == "plain":
            return (*self.tensors, slot, *mag)
        if self.kind == "hada":
            return ("hada", *self.tensors, slot, *mag)
        return ("kron", *self.tensors, self.taps, self.layout, slot, *mag)


def build_factors(p: Placed, w: torch.Tensor, weight_shape, nhwc: bool) -> Factor:
    """What the merge holds for one adapter on one weight, everything scale-independent done: `w` is the weight's (N, K) view,
    `weight_shape` the parameter's own shape.  "lora" and "tucker" give a "plain" Factor, "loha" a "hada" and "lokr" a "kron" one."""
    f32 = lambda t: t.detach().to(device=w.device, dtype=torch.float32)         # noqa: E731
    mag = None if p.magnitude is None else f32(p.magnitude).reshape(-1).contiguous()
    conv = len(weight_shape) == 4
    taps = weight_shape[2] * weight_shape[3] if conv else 1
    if p.form in ("lora", "tucker"):
        down, up = f32(p.down), f32(p.up)
        r = down.shape[0]
        up = up.reshape(up.shape[0], -1)
        if p.form == "tucker":
            down = contract_core(f32(p.parts["lora_mid"]), down.reshape(r, -1), nhwc)
        elif conv:                                                           # the down factor in the K order of the weight's memory
            down = down[:, :, None, None] if down.dim() == 2 else down
            down = (down.permute(0, 2, 3, 1) if nhwc else down).reshape(r, -1)
        return Factor("plain", _padded_pair(up * (p.alpha / r), down, w), magnitude=mag)
    parts = {k: f32(v) for k, v in p.parts.items()}
    if p.form == "loha":
        sigma = 1.0 if p.alpha is None else p.alpha / parts["hada_w1_b"].shape[0]
        pairs = []
        for m in "12":
            wa, wb, t = parts[f"hada_w{m}_a"], parts[f"hada_w{m}_b"], parts.get(f"hada_t{m}")
            up, down = (wa.t(), contract_core(t, wb, nhwc)) if t is not None else (wa, _k_order(wb, weight_shape, nhwc))
            pairs += _padded_pair(up * sigma if m == "1" else up, down, w)
        return Factor("hada", tuple(pairs), magnitude=mag)
    # LoKr
    rank = None
    if "lokr_w1" in parts:
        w1 = parts["lokr_w1"]
    else:
        w1, rank = parts["lokr_w1_a"] @ parts["lokr_w1_b"], parts["lokr_w1_b"].shape[0]
    a, b = w1.shape
    c, d = weight_shape[0] // a, weight_shape[1] // b
    if "lokr_w2" in parts:
        w2 = parts["lokr_w2"]
    elif "lokr_t2" in parts:
        w2, rank = torch.einsum("pqyx,pc,qd->cdyx", parts["lokr_t2"], parts["lokr_w2_a"], parts["lokr_w2_b"]), parts["lokr_w2_b"].shape[0]
    else:
        w2, rank = parts["lokr_w2_a"] @ parts["lokr_w2_b"], parts["lokr_w2_b"].shape[0]
    w2 = w2.reshape(c, d, *(weight_shape[2:] if conv else (1, 1)))
    sigma = 1.0 if p.alpha is None or rank is None else p.alpha / rank
    layout = 1 if conv and nhwc else 0
    w2 = (w2.permute(0, 2, 3, 1) if layout else w2).reshape(c, -1)
    return Factor("kron", ((w1 * sigma).contiguous(), w2.contiguous()), taps, layout, mag)


def factor_delta(f: Factor) -> torch.Tensor:
    """The fp32 delta (N, K) of one factor as the kernel forms it (torch, any device): a product, the elementwise product
    of two products, or a Kronecker product in the column order of the factor's layout."""
    if f.kind == "kron":
        w1, w2 = f.tensors
        if not f.layout:
            return torch.kron(w1, w2)                                        # [i c + p, j (d taps) + col]
        (a, b), c, d = w1.shape, w2.shape[0], w2.shape[1] // f.taps
        return torch.einsum("ij,ptq->iptjq", w1, w2.reshape(c, f.taps, d)).reshape(a * c, f.taps * b * d)
    up, down_t = f.tensors[:2]
    delta = up.float() @ down_t.float().t()
    if f.kind == "hada":
        up2, down2_t = f.tensors[2:]
        delta = delta * (up2.float() @ down2_t.float().t())
    return delta


def target_linears(module: nn.Module) -> "OrderedDict[str, nn.Linear]":
    """The module's `nn.Linear` submodules under the names an adapter uses.  A compiled module also holds its hoisted
    context / time sub-graphs, which reference the same Linear objects: each object is listed once, under its first (own)
    name.  A wrapper that keeps the network in `.unet` (the label-vector entry) does not add its prefix."""
    return target_modules(module, convs=False)


def target_modules(module: nn.Module, convs: bool) -> "OrderedDict[str, nn.Module]":
    """`target_linears`, and with `convs` also the module's `nn.Conv2d` submodules, under the same naming rule."""
    kinds = (nn.Linear, nn.Conv2d) if convs else nn.Linear
    out = OrderedDict()
    for name, m in module.named_modules():
        if isinstance(m, kinds):
            out[name[len("unet."):] if name.startswith("unet.") else name] = m
    return out


def weight_rows(w: torch.Tensor) -> Tuple[torch.Tensor, bool]:
    """The row-major (N, K) view of a weight's own memory, and whether K runs (R, S, I) - a channels_last conv weight - and
    not (I, R, S).  A Linear weight is its own view."""
    if w.dim() == 2:
        return w, False
    nhwc = w.permute(0, 2, 3, 1)
    if nhwc.is_contiguous():
        return nhwc.reshape(w.shape[0], -1), True
    if w.is_contiguous():
        return w.reshape(w.shape[0], -1), False
    raise ValueError(f"a conv weight must be dense, channels_last or contiguous; got strides {w.stride()} for {tuple(w.shape)}")


class _Adapter:
    def __init__(self, slot: int, scale: float):
        self.slot, self.scale = slot, scale
        self.factors: Dict[str, Factor] = {}      # module -> what `build_factors` made of the adapter's tensors for it


class LoraSet:
    """The adapters of ONE module (an `optimize_model` result or the plain `nn.Module`).  Up to MAX_ADAPTERS at once.

    On the GPU every change is one launch of the grouped merge kernel over all adapted weights; on the CPU the same formula
    runs in torch (fp32), so host tests and tools work.  After a merge the version counter of every rewritten parameter is
    bumped (the kernel writes through raw pointers) and `on_change()` runs: by default the module's
    `exec_context.refresh_derived(full=True)`.  Owners that cache more than derived weights (hoisted text K/V, time tables)
    re-derive those themselves after calling in here (`DenoiseLoop.load_lora`, the hooks' `load_lora`).

    Memory: one snapshot per ADAPTED weight (taken when the first adapter touches it, freed when the last one leaves) plus the
    factors."""

    def __init__(self, module: nn.Module, on_change: Optional[Callable[[], object]] = None):
        self.module = module
        self.linears = target_linears(module)
        if not self.linears:
            raise ValueError("LoraSet: the module has no nn.Linear to adapt")
        self.targets = target_modules(module, convs=True)      # what `load(convs=True)` may name; `linears` is the default
        ectx = getattr(module, "exec_context", None)
        self.on_change = on_change if on_change is not None else ((lambda: ectx.refresh_derived(full=True)) if ectx is not None else None)
        self._adapters: "OrderedDict[str, _Adapter]" = OrderedDict()
        self._base: Dict[str, torch.Tensor] = {}
        self._global = 1.0                   # diffusers' cross_attention_kwargs scale: one multiplier over every adapter
        self._scales: Optional[torch.Tensor] = None      # device table, MAX_ADAPTERS floats, allocated once
        self._plan = None
        self.last_unplaced: List[str] = []

    # ---- queries -------------------------------------------------------------------------------
    def names(self) -> List[str]:
        return list(self._adapters)

    def scales(self) -> Dict[str, float]:
        return {n: a.scale for n, a in self._adapters.items()}

    def adapted_modules(self) -> List[str]:
        return list(self._base)

    @property
    def global_scale(self) -> float:
        return self._global

    # ---- changes -------------------------------------------------------------------------------
    def load(self, name: str, state_dict: Mapping[str, torch.Tensor], scale: float = 1.0, strict: bool = True,
             convs: bool = False, lycoris: bool = False) -> List[str]:
        """Merge the adapter `state_dict` under `name` at `scale`.  Everything is checked before anything is written.
        `convs=True` also takes the adapter's convolution factors (LoCon) on this module's `nn.Conv2d`; DoRA magnitudes are
        applied wherever their module is a target.  `lycoris=True` also takes Tucker cores, LoHa and LoKr factors (the module
        docstring) on those targets.  Returns the keys that were not applied (text-encoder keys always; with
        strict=False also keys that name no target of this module, which strict=True refuses).  Input-axis magnitudes ON a
        target, and without `lycoris=True` Tucker / LoHa / LoKr keys, raise whatever `strict` says (`parse_lora_state_dict`)."""
        if name in self._adapters:
            raise ValueError(f"a LoRA named {name!r} is already loaded (unload it first)")
        if len(self._adapters) >= MAX_ADAPTERS:
            raise ValueError(f"at most {MAX_ADAPTERS} adapters can be loaded at once")
        targets = self.targets if convs else self.linears
        kind = "nn.Linear or nn.Conv2d" if convs else "nn.Linear"
        placed, unplaced = parse_adapter(state_dict, targets.keys(), lycoris=lycoris)
        foreign = [k for k in unplaced if not is_text_encoder_key(k)]
        if strict and foreign:
            hint = "" if convs else "convolution adapters are only applied on request: pass convs=True; "
            raise ValueError(f"LoRA {name!r}: {len(foreign)} keys name no {kind} of this model ({hint}"
                             f"pass strict=False to load the rest): {foreign[:8]}{' ...' if len(foreign) > 8 else ''}")
        if not placed:
            raise ValueError(f"LoRA {name!r}: no key names an {kind} of this model")
        for mod, p in placed.items():
            m = targets[mod]
            if isinstance(m, nn.Conv2d) and (m.groups != 1 or tuple(m.dilation) != (1, 1)):
                raise ValueError(f"{mod}: a grouped or dilated convolution (groups {m.groups}, dilation {tuple(m.dilation)}) takes no adapter")
            check_shapes(mod, tuple(m.weight.shape), p.down, p.up, p.magnitude, p.form, p.parts)
            if isinstance(m, nn.Conv2d):
                weight_rows(m.weight)                                  # (refuses a weight that is not dense)
        scale = float(scale)
        slot = min(set(range(MAX_ADAPTERS)) - {a.slot for a in self._adapters.values()})
        ad = _Adapter(slot, scale)
        with torch.no_grad():
            for mod, p in placed.items():
                w, nhwc = weight_rows(targets[mod].weight.detach())
                ad.factors[mod] = build_factors(p, w, tuple(targets[mod].weight.shape), nhwc)
                if mod not in self._base:
                    self._base[mod] = w.clone(memory_format=torch.contiguous_format)
        self._adapters[name] = ad
        self._plan = None
        self._merge()
        self.last_unplaced = unplaced
        return unplaced

    def set_scale(self, name: str, scale: float) -> None:
        self.set_scales({name: scale})

    def set_scales(self, scales: Mapping[str, float]) -> None:
        """New scales for some of the loaded adapters: a copy into the device scale table and one launch."""
        for n in scales:
            if n not in self._adapters:
                raise KeyError(f"no LoRA named {n!r} is loaded (loaded: {self.names()})")
        vals = {n: float(s) for n, s in scales.items()}
        for n, s in vals.items():
            self._adapters[n].scale = s
        self._merge()

    def set_global_scale(self, scale: float) -> bool:
        """One multiplier over every loaded adapter (what diffusers' `cross_attention_kwargs={"scale": s}` means).  Merges
        again only when it differs from the current one; returns whether it did."""
        scale = float(scale)
        if scale == self._global:
            return False
        self._global = scale
        if self._adapters:
            self._merge()
        return True

    def unload(self, name: str) -> None:
        """Remove one adapter.  Weights no other adapter touches get their base's bits back and their snapshot is freed."""
        if name not in self._adapters:
            raise KeyError(f"no LoRA named {name!r} is loaded (loaded: {self.names()})")
        del self._adapters[name]
        self._plan = None
        self._merge()
        still = {m for a in self._adapters.values() for m in a.factors}
        for mod in [m for m in self._base if m not in still]:
            del self._base[mod]
        self._plan = None

    def unload_all(self) -> None:
        if not self._adapters:
            return
        self._adapters.clear()
        self._plan = None
        self._merge()
        self._base.clear()
        self._plan = None

    # ---- the merge -----------------------------------------------------------------------------
    def _effective(self) -> List[float]:
        eff = [0.0] * MAX_ADAPTERS
        for a in self._adapters.values():
            eff[a.slot] = a.scale * self._global
        return eff

    def _entries(self):
        """Per snapshotted module: (parameter, its (N, K) view, base, [(Factor, slot), ...]) in load order (the kernel's
        summation order)."""
        out = []
        for mod, base in self._base.items():
            facs = [(a.factors[mod], a.slot) for a in self._adapters.values() if mod in a.factors]
            param = self.targets[mod].weight
            out.append((param, weight_rows(param.detach())[0], base, facs))
        return out

    def _merge(self) -> None:
        if not self._base:
            return
        eff = self._effective()
        entries = self._entries()
        w0 = entries[0][1]
        with torch.no_grad():
            if w0.device.type == "cuda":
                from . import ops
                if any(not w.is_contiguous() for _, w, _, _ in entries):
                    raise ops.BackendError("LoraSet: an adapted weight is not contiguous")
                if self._scales is None:
                    self._scales = torch.zeros(MAX_ADAPTERS, dtype=torch.float32, device=w0.device)
                if self._plan is None:
                    self._plan = ops.lora_plan([(w, b, [f.entry(slot) for f, slot in facs]) for _, w, b, facs in entries])
                self._scales.copy_(torch.tensor(eff, dtype=torch.float32))
                ops.lora_merge(self._plan, self._scales)
            else:
                for _, w, base, facs in entries:
                    _merge_torch(w, base, facs, eff)
        for param, _, _, _ in entries:
            torch.autograd.graph.increment_version(param)
        if self.on_change is not None:
            self.on_change()


def _merge_torch(w: torch.Tensor, base: torch.Tensor, facs, eff) -> None:
    """The kernel's formula in torch (CPU): fp32 products and sums, one rounding to the storage dtype, base bits when every
    scale is zero.  `w` is the weight's (N, K) view, `facs` its [(Factor, slot), ...]; `factor_delta` forms each one's delta."""
    live = [(f, eff[slot], f.magnitude) for f, slot in facs if eff[slot] != 0.0]
    if not live:
        w.detach().copy_(base)
        return
    delta = torch.zeros(w.shape, dtype=torch.float32)
    if all(mag is None for _, _, mag in live):
        for f, s, _ in live:
            delta.add_(factor_delta(f), alpha=s)
        w.detach().copy_((base.float() + delta).to(w.dtype))
        return
    b = base.float()
    bcoef = torch.ones((w.shape[0], 1), dtype=torch.float32)
    for f, s, mag in live:
        acc = factor_delta(f)
        if mag is None:
            delta.add_(acc, alpha=s)
            continue
        ss = (b + s * acc).pow(2).sum(dim=1)
        gain = torch.where(ss > 0, mag / ss.sqrt(), torch.zeros_like(ss))[:, None]      # m / ||Base + s Up Down|| per row; 0 for a zero row
        bcoef += gain - 1.0
        delta += (gain * s) * acc
    w.detach().copy_((bcoef * b + delta).to(w.dtype))


def attach(compiled: nn.Module) -> LoraSet:
    """The LoraSet of a module (an `optimize_model` result, or a plain `nn.Module`), created on first use.  One set per
    module: every owner that drives this module shares it."""
    holder = compiled.__dict__
    ls = holder.get("_lora_set")
    if ls is None:
        if not isinstance(compiled, nn.Module):
            raise TypeError("lora.attach: expected an nn.Module (the result of optimize_model, or the model itself)")
        ls = holder["_lora_set"] = LoraSet(compiled)
    return ls
