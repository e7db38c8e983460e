"""The ControlNet tests' own statement of the method (checker only; shares no code with stabletriton_amd/controlnet.py's sites).

`controlled` is the reference of every test: the EAGER UNet2DConditionModel's `denoise` restated with skips[k] + s * w_k * r_k after
the encoder and mid + s * w_m * r_m behind the middle block (diffusers' `down_block_additional_residuals` /
`mid_block_additional_residual`), in whatever precision the module has - float64 in the tests.  The residuals come from the eager
ControlNetXL (`branch_residuals`).  Never the compiled module."""
import torch

from stabletriton_amd import synth
from stabletriton_amd.controlnet import ControlNetXL


def controlled(unet, sample, timesteps, encoder_hidden_states, added_cond_kwargs, residuals=None, scale=0.0, weights=None):
    """[eps] of the eager `unet` with the residuals (the skips' in encoder order, the middle block's last) added at `scale` times the
    per-site `weights`; residuals None: the plain network."""
    text_embeds, time_ids = added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]
    tid = unet.add_time_proj(time_ids.flatten()).reshape((text_embeds.shape[0], -1))
    add = torch.concat([text_embeds, tid], dim=-1)
    timesteps = timesteps.expand(sample.shape[0])
    emb = unet.time_embedding(unet.time_proj(timesteps).to(dtype=sample.dtype))
    emb = emb + unet.add_embedding(add.to(emb.dtype))
    x = unet.conv_in(sample)
    skips = [x]
    for blk in unet.down_blocks:
        x = blk.encode(x, emb, encoder_hidden_states, skips)
    x = unet.mid_block(x, emb, encoder_hidden_states)
    if residuals is not None:
        assert len(residuals) == len(skips) + 1
        w = [1.0] * len(residuals) if weights is None else list(weights)
        rep = lambda r, like: r.to(like.dtype).repeat(like.shape[0] // r.shape[0], 1, 1, 1)
        skips = [s + scale * w[k] * rep(residuals[k], s) for k, s in enumerate(skips)]
        x = x + scale * w[-1] * rep(residuals[-1], x)
    for blk in unet.up_blocks:
        x = blk.decode(x, emb, encoder_hidden_states, skips)
    return [unet.conv_out(unet.conv_act(unet.conv_norm_out(x)))]


def site_shapes(spec, latent_hw):
    """(C, h, w) per site, written out: conv_in and each resnet at its level's size, each downsampler at the next (the stride-2
    convolutions round up), the middle block at the last."""
    lh, lw = (latent_hw, latent_hw) if isinstance(latent_hw, int) else latent_hw
    sizes = [(lh, lw)]
    for _ in spec.widths[1:]:
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    out = [(spec.widths[0],) + sizes[0]]
    for lvl, c in enumerate(spec.widths):
        out += [(c,) + sizes[lvl]] * spec.resnets_per_level
        if lvl < len(spec.widths) - 1:
            out.append((c,) + sizes[lvl + 1])
    return out + [(spec.widths[-1],) + sizes[-1]]


def residuals(spec, latent_hw, rows=1, seed=7, magnitude=0.25):
    """Synthetic residuals, fp32, deterministic (the pass and kernel tests; the network tests take the branch's)."""
    return [synth.normal(f"cn.residual.{k}.{rows}.{c}x{h}x{w}", (rows, c, h, w), seed + k) * magnitude
            for k, (c, h, w) in enumerate(site_shapes(spec, latent_hw))]


def branch(spec, seed=3):
    """An eager fp32 ControlNetXL with every parameter filled, the zero convolutions too (zero weights would test nothing)."""
    m = ControlNetXL(spec).eval().requires_grad_(False)
    synth.fill_module_(m, seed)
    return m


def control_image(rows, latent_hw, seed=5):
    lh, lw = (latent_hw, latent_hw) if isinstance(latent_hw, int) else latent_hw
    return synth.normal(f"cn.image.{rows}.{lh}x{lw}", (rows, 3, 8 * lh, 8 * lw), seed)


def branch_residuals(net, sample, timesteps, encoder_hidden_states, added_cond_kwargs, cond_embed):
    """The flat list the sites take: the eager branch's skip residuals, then its middle one."""
    with torch.no_grad():
        down, mid = net(sample, timesteps, encoder_hidden_states, added_cond_kwargs, cond_embed)
    return list(down) + [mid]
