"""IP-Adapter, the tests' own float64 restatement and shared helpers (tests/test_ip_adapter_*.py).

    out[b,t,h,:] = sum_r fl32(scale_r * w[b,r,t]) * softmax_s(sm * q[b,t,h] . k_r[b,s,h]) v_r[b,s,h]        (s over segment r's keys)

written per head with explicit matrix products in float64, independently of stabletriton_amd.ip_adapter.reference (which goes
through pag.identity_attention_reference), and a synthetic checkpoint builder from synth."""
import torch
from torch import fx

from stabletriton_amd import pag, synth


def attention64(q, k, v, heads, sm):
    """Plain softmax attention in float64 on (B, T, H*D) / (B, S, H*D) projections, one head at a time -> (B, T, H*D) float64."""
    B, T, C = q.shape
    d = C // heads
    out = torch.empty((B, T, C), dtype=torch.float64)
    for h in range(heads):
        cols = slice(h * d, (h + 1) * d)
        qh, kh, vh = q[..., cols].double().cpu(), k[..., cols].double().cpu(), v[..., cols].double().cpu()
        s = qh @ kh.transpose(1, 2) * float(sm)
        e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
        out[..., cols] = (e / e.sum(dim=-1, keepdim=True)) @ vh
    return out


def effective_weights(weights, seg_scale):
    """w_eff = fl32(seg_scale[r] * weights[b,r,t]), in fp32 torch: (B, S, T) float32 on the host."""
    w = weights.float().cpu()
    return w if seg_scale is None else torch.as_tensor(seg_scale, dtype=torch.float32).cpu()[None, :, None] * w


def segments64(q, segments, weights, seg_scale, heads, sm):
    """The formula above in float64: (B, T, H*D) float64."""
    w = effective_weights(weights, seg_scale).double()
    out = torch.zeros(q.shape, dtype=torch.float64)
    for r, (k, v) in enumerate(segments):
        out += w[:, r].unsqueeze(-1) * attention64(q, k, v, heads, sm)
    return out


def checkpoint(state, n_tokens, emb_dim=32, seed=5, layout="published", slot=0):
    """A synthetic adapter for the compiled module whose state is `state`: to_k_ip / to_v_ip for every site, numbered in diffusers'
    attn_processors order (down, up, mid) for the published / flat layouts, and a linear image projection.
    -> (state dict in `layout`, {site path: (wk, wv)})."""
    sites = list(state.sites)
    stage = lambda p: 0 if "down_blocks." in p else (1 if "up_blocks." in p else 2)
    order = sorted(range(len(sites)), key=lambda i: (stage(sites[i]), i))
    by_path, numbered = {}, {}
    for rank, i in enumerate(order):
        c, x = state.dims[i]
        wk = synth.normal(f"ip.k.{seed}.{sites[i]}", (c, x), seed) * x ** -0.5
        wv = synth.normal(f"ip.v.{seed}.{sites[i]}", (c, x), seed + 1) * x ** -0.5
        by_path[sites[i]] = (wk, wv)
        numbered[f"{2 * rank + 1}.to_k_ip.weight"] = wk
        numbered[f"{2 * rank + 1}.to_v_ip.weight"] = wv
    cross = state.dims[0][1]
    proj = {"proj.weight": synth.normal(f"ip.proj.w.{seed}", (n_tokens * cross, emb_dim), seed + 2) * emb_dim ** -0.5,
            "proj.bias": synth.normal(f"ip.proj.b.{seed}", (n_tokens * cross,), seed + 3) * 0.1,
            "norm.weight": 1.0 + 0.1 * synth.normal(f"ip.norm.w.{seed}", (cross,), seed + 4),
            "norm.bias": 0.1 * synth.normal(f"ip.norm.b.{seed}", (cross,), seed + 5)}
    if layout == "published":
        return {"image_proj": proj, "ip_adapter": numbered}, by_path
    if layout == "flat":
        sd = {f"ip_adapter.{k}": v for k, v in numbered.items()}
        sd.update({f"image_proj.{k}": v for k, v in proj.items()})
        return sd, by_path
    if layout == "processor":
        sd = {}
        for p, (wk, wv) in by_path.items():
            sd[f"{p}.processor.to_k_ip.{slot}.weight"] = wk
            sd[f"{p}.processor.to_v_ip.{slot}.weight"] = wv
        return sd, by_path
    assert layout == "path"
    sd = {}
    for p, (wk, wv) in by_path.items():
        sd[f"{p}.to_k_ip.weight"] = wk
        sd[f"{p}.to_v_ip.weight"] = wv
    return sd, by_path


def image_tokens(rows, n_tokens, cross_dim, seed=91):
    return synth.normal(f"ip.tokens.{seed}", (rows, n_tokens, cross_dim), seed)


def traced_cpu(m, ip_adapter=None):
    """fuse_attention (+ insert_ip_adapter) on a traced eager module; the remaining attention_wrapper leaves have no CPU route and
    get the plain torch attention: every node is then eager torch, the module runs on the CPU.  Returns (module, sites)."""
    from stabletriton_amd.optimizers import fuse_attention, insert_ip_adapter
    from stabletriton_amd.optimizers.wrappers import attention_wrapper
    gm = fx.symbolic_trace(m)
    fuse_attention(gm)
    sites = insert_ip_adapter(gm, ip_adapter) if ip_adapter else 0
    for n in list(gm.graph.nodes):
        if n.op == "call_function" and n.target is attention_wrapper:
            with gm.graph.inserting_before(n):
                new = gm.graph.call_function(pag.identity_attention_reference, (n.args[0], n.args[1], n.args[2], n.args[5], n.args[4], 0))
            n.replace_all_uses_with(new)
            gm.graph.erase_node(n)
    gm.recompile()
    return gm, sites
