"""Regional cross-attention, the tests' own float64 restatement and shared helpers (tests/test_regions_*.py).

    out[b,t,h,:] = sum_r w[b,r,t] * softmax_s(scale * q[b,t,h] . k[b, r*L+s, h]) v[b, r*L+s, h]        (s over segment r's L keys)

written with einsum on (B, T, H, D) views, independently of stabletriton_amd.regions.reference (matmul on transposed heads)."""
import torch
from torch import fx

from stabletriton_amd import pag, synth


def attention64(q, k, v, heads, scale):
    """Plain softmax attention in float64 on (B, T, H*D) / (B, S, H*D) projections -> (B, T, H*D) float64."""
    B, T, C = q.shape
    S = k.shape[1]
    d = C // heads
    q4, k4, v4 = (t.double().reshape(B, -1, heads, d) for t in (q, k, v))
    s = torch.einsum("bthd,bshd->bhts", q4, k4) * float(scale)
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    p = p / p.sum(dim=-1, keepdim=True)
    return torch.einsum("bhts,bshd->bthd", p, v4).reshape(B, T, C)


def regions64(q, k, v, weights, heads, scale, seg_len):
    """The formula above in float64: (B, T, H*D) float64."""
    R = weights.shape[1]
    assert k.shape[1] == R * seg_len
    out = torch.zeros(q.shape, dtype=torch.float64)
    for r in range(R):
        seg = slice(r * seg_len, (r + 1) * seg_len)
        out += weights[:, r].double().unsqueeze(-1) * attention64(q, k[:, seg], v[:, seg], heads, scale)
    return out


def left_right_masks(lh, lw, R=2):
    """R vertical stripes of a (lh, lw) latent: mask r is 1 on columns [r * lw / R, (r + 1) * lw / R)."""
    m = torch.zeros((R, lh, lw))
    for r in range(R):
        m[r, :, (r * lw) // R:((r + 1) * lw) // R] = 1.0
    return m


def two_prompts(rows, tokens, cross_dim, seed=77):
    """(rows, 2 * tokens, cross_dim): synth's prompt states for segment 0 beside a second, different prompt."""
    a = synth.normal(f"regions.prompt.a.{seed}", (rows, tokens, cross_dim), seed)
    b = synth.normal(f"regions.prompt.b.{seed}", (rows, tokens, cross_dim), seed + 1)
    return torch.cat([a, b], dim=1)


def traced_cpu(m, R=None, seg_len=77):
    """fuse_attention (+ insert_regions) on a traced eager module; the remaining attention_wrapper leaves have no CPU route and get
    the plain torch attention: every node is then eager torch, the module runs on the CPU.  Returns (module, region sites)."""
    from stabletriton_amd.optimizers import fuse_attention, insert_regions
    from stabletriton_amd.optimizers.wrappers import attention_wrapper
    gm = fx.symbolic_trace(m)
    fuse_attention(gm)
    sites = insert_regions(gm, R, seg_len) if R else 0
    for n in list(gm.graph.nodes):
        if n.op == "call_function" and n.target is attention_wrapper:
            with gm.graph.inserting_before(n):
                new = gm.graph.call_function(pag.identity_attention_reference, (n.args[0], n.args[1], n.args[2], n.args[5], n.args[4], 0))
            n.replace_all_uses_with(new)
            gm.graph.erase_node(n)
    gm.recompile()
    return gm, sites


def euler_loop_cpu(mod, tables, noise, ehs, text_embeds, time_ids):
    """The unguided Euler trajectory of pipeline.DenoiseLoop in fp32 on the CPU around the module `mod`: final latent."""
    lat = noise.float() * tables.init_noise_sigma
    in_scale, dsigma = tables.in_scale(), tables.dsigma()
    with torch.no_grad():
        for i in range(tables.n_steps):
            t = torch.tensor(float(tables.timesteps[i]))
            eps = mod(lat * float(in_scale[i]), t, ehs, {"text_embeds": text_embeds, "time_ids": time_ids})[0]
            lat = lat + eps.float() * float(dsigma[i])
    return lat
