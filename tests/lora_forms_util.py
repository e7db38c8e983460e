"""Synthetic LyCORIS adapters (Tucker LoCon, LoHa, Tucker LoHa, LoKr in its variants) under kohya keys, and the float64
restatement of what they mean, written from the definitions in stabletriton_amd/lora.py's docstring on the weights' own
4-D / 2-D shapes (no memory layout, no padding, no tables):

    D_j = sigma_j * (the form's delta),   V_j = B + s_j D_j,   g_j[n] = m_j[n] / ||V_j[n]||  (1 without a dora_scale),
    W = B + sum_j (g_j V_j - B)."""
import math

import torch


def stem(name: str) -> str:
    return "lora_unet_" + name.replace(".", "_")


def divisor(n: int) -> int:
    """The largest divisor of n that is at most sqrt(n): LyCORIS's default factorisation, (divisor, n // divisor)."""
    return max(d for d in range(1, math.isqrt(n) + 1) if n % d == 0)


def make(form: str, shape, g: torch.Generator, rank: int = 4, std: float = 0.1, alpha=None, ab=None, rank2=None):
    """The tensors of one module's adapter under their key suffixes.  `form`: "tucker", "loha", "loha_tucker", "lokr" (w1 full,
    w2 full), "lokr_w2fac", "lokr_w1fac" (w1 factorised, w2 full), "lokr_bothfac", "lokr_tucker".  `ab`: LoKr's (a, b),
    default divisor(O), divisor(I).  `rank2`: LoHa's second rank (default `rank`)."""
    conv = len(shape) == 4
    o, i = shape[:2]
    rs = tuple(shape[2:]) if conv else ()
    taps = math.prod(rs)
    rn = lambda *s: torch.randn(*s, generator=g) * std                               # noqa: E731
    p = {}
    if form == "tucker":
        p = {"lora_down.weight": rn(rank, i, 1, 1), "lora_mid.weight": rn(rank, rank, *rs) * (0.5 / std), "lora_up.weight": rn(o, rank, 1, 1)}
    elif form == "loha":
        r2 = rank2 or rank
        p = {"hada_w1_a": rn(o, rank), "hada_w1_b": rn(rank, i * taps), "hada_w2_a": rn(o, r2), "hada_w2_b": rn(r2, i * taps)}
    elif form == "loha_tucker":
        p = {"hada_t1": rn(rank, rank, *rs) * (0.5 / std), "hada_w1_a": rn(rank, o), "hada_w1_b": rn(rank, i),
             "hada_t2": rn(rank, rank, *rs) * (0.5 / std), "hada_w2_a": rn(rank, o), "hada_w2_b": rn(rank, i)}
    elif form.startswith("lokr"):
        a, b = ab or (divisor(o), divisor(i))
        c, d = o // a, i // b
        if form in ("lokr_w1fac", "lokr_bothfac"):
            p["lokr_w1_a"], p["lokr_w1_b"] = rn(a, rank), rn(rank, b) * (1.0 / std)
        else:
            p["lokr_w1"] = rn(a, b)
        if form in ("lokr_w2fac", "lokr_bothfac"):
            p["lokr_w2_a"], p["lokr_w2_b"] = rn(c, rank), rn(rank, d * taps) * (1.0 / std)
        elif form == "lokr_tucker":
            p["lokr_t2"], p["lokr_w2_a"], p["lokr_w2_b"] = rn(rank, rank, *rs) * (0.5 / std), rn(rank, c), rn(rank, d) * (1.0 / std)
        else:
            p["lokr_w2"] = rn(c, d, *rs)
    else:
        raise ValueError(form)
    if alpha is not None:
        p["alpha"] = torch.tensor(float(alpha))
    return p


def keyed(name: str, parts) -> dict:
    return {f"{stem(name)}.{k}": v for k, v in parts.items()}


def delta64(parts, shape) -> torch.Tensor:
    """sigma * delta of one module's adapter in float64, in the weight's own shape."""
    p = {k[:-len(".weight")] if k.endswith(".weight") else k: v.double() for k, v in parts.items() if k != "dora_scale"}
    conv = len(shape) == 4
    o, i = shape[:2]
    r_, s_ = (shape[2], shape[3]) if conv else (1, 1)
    alpha = float(p["alpha"]) if "alpha" in p else None

    def tucker(t, wa, wb):                      # sum_pq t[p,q,y,x] wa[p,o] wb[q,i]
        return torch.einsum("pqyx,po,qi->oiyx", t, wa, wb)

    if "lora_mid" in p:
        up, down = p["lora_up"].reshape(o, -1), p["lora_down"].reshape(-1, i)
        d = torch.einsum("oa,abyx,bi->oiyx", up, p["lora_mid"], down)
        rank = down.shape[0]
    elif "hada_w1_a" in p:
        ws = []
        for m in "12":
            wa, wb = p[f"hada_w{m}_a"], p[f"hada_w{m}_b"]
            ws.append(tucker(p[f"hada_t{m}"], wa, wb) if f"hada_t{m}" in p else (wa @ wb).reshape(o, i, r_, s_))
        d, rank = ws[0] * ws[1], p["hada_w1_b"].shape[0]
    elif any(k.startswith("lokr_") for k in p):
        rank = None
        if "lokr_w1" in p:
            w1 = p["lokr_w1"]
        else:
            w1, rank = p["lokr_w1_a"] @ p["lokr_w1_b"], p["lokr_w1_b"].shape[0]
        a, b = w1.shape
        c, dd = o // a, i // b
        if "lokr_w2" in p:
            w2 = p["lokr_w2"].reshape(c, dd, r_, s_)
        elif "lokr_t2" in p:
            w2, rank = tucker(p["lokr_t2"], p["lokr_w2_a"], p["lokr_w2_b"]), p["lokr_w2_b"].shape[0]
        else:
            w2, rank = (p["lokr_w2_a"] @ p["lokr_w2_b"]).reshape(c, dd, r_, s_), p["lokr_w2_b"].shape[0]
        d = torch.einsum("ij,pqyx->ipjqyx", w1, w2).reshape(o, i, r_, s_)
        if rank is None:
            alpha = None                        # both stored full: sigma = 1
    else:
        down = p["lora_down"]
        rank = down.shape[0]
        d = torch.einsum("oa,aiyx->oiyx", p["lora_up"].reshape(o, rank), down.reshape(rank, i, r_, s_))
    sigma = 1.0 if alpha is None else alpha / rank
    return (sigma * d).reshape(shape)


def merged64(base: torch.Tensor, adapters) -> torch.Tensor:
    """W of the module docstring for one weight: `base` float64 in its own shape, `adapters` [(parts, scale), ...] in load order."""
    rows = base.reshape(base.shape[0], -1)
    w = rows.clone()
    for parts, s in adapters:
        v = rows + s * delta64(parts, tuple(base.shape)).reshape(rows.shape)
        gain = (parts["dora_scale"].double().reshape(-1) / v.norm(dim=1))[:, None] if "dora_scale" in parts else 1.0
        w = w + gain * v - rows
    return w.reshape(base.shape)


def abs_terms64(base: torch.Tensor, adapters):
    """(|B| + sum_j |s_j| |D_j|) elementwise and the largest |g_j|: what an fp32 evaluation's error scales with."""
    rows = base.reshape(base.shape[0], -1)
    mag, gmax = rows.abs().clone(), 1.0
    for parts, s in adapters:
        d = delta64(parts, tuple(base.shape)).reshape(rows.shape)
        mag += abs(s) * d.abs()
        if "dora_scale" in parts:
            gmax = max(gmax, float((parts["dora_scale"].double().reshape(-1) / (rows + s * d).norm(dim=1)).max()))
    return mag.reshape(base.shape), gmax
