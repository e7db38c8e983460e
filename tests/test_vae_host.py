"""DecoderXL (stabletriton_amd/vae.py) without a GPU: what the rewrite passes make of its trace, its state-dict keys, and the
head sizes st_attention refuses before any launch."""
import torch
import torch.nn.functional as F
from torch import nn

from stabletriton_amd import _C, vae
from stabletriton_amd.optimization import replace_backend
from stabletriton_amd.optimizers.wrappers import attention_wrapper, conv2d_wrapper

P = 1 << 20            # a fake, aligned, never dereferenced device address: validation happens before any launch


def test_rewrite_stats():
    """14 resnets (28 GroupNorm+SiLU) + conv_norm_out; the attention's GroupNorm has no SiLU.  34 3x3 / 1x1 convs + the widened
    conv_out; post_quant_conv stays a torch call.  Every resnet's skip add and the attention's residual ride in an epilogue."""
    gm = replace_backend(vae.DecoderXL().eval())
    s = gm.rewrite_stats
    assert (s["attention"], s["group_norm_silu"], s["group_norm"], s["conv"]) == (1, 29, 1, 35)
    assert (s["residual_adds"], s["token_residuals"], s["shared_input_gemms"], s["group_norm_stats"]) == (14, 1, 1, 30)
    mods = dict(gm.named_modules())
    calls = [n for n in gm.graph.nodes if n.op == "call_function"]
    assert not [n for n in gm.graph.nodes if n.op == "call_module" and isinstance(mods[n.target], (nn.GroupNorm, nn.Conv2d))]
    assert not [n for n in calls if n.target is F.interpolate]
    att = [n for n in calls if n.target is attention_wrapper]
    assert len(att) == 1 and att[0].args[5:] == (1, 512)
    assert sum(bool(n.args[2]) for n in calls if n.target is conv2d_wrapper) == 3          # the three Upsample gathers
    assert gm.decoder.conv_out.out_channels == 4 and not gm.decoder.conv_out.weight[3].any()


def test_state_dict_round_trip():
    torch.manual_seed(0)
    a, b = vae.DecoderXL(), vae.DecoderXL()
    sd = a.state_dict()
    assert len(sd) == 140
    for key in ("post_quant_conv.weight", "decoder.conv_in.bias", "decoder.mid_block.attentions.0.to_q.weight",
                "decoder.mid_block.attentions.0.to_out.0.bias", "decoder.mid_block.attentions.0.group_norm.weight",
                "decoder.up_blocks.2.resnets.0.conv_shortcut.weight", "decoder.up_blocks.2.upsamplers.0.conv.bias",
                "decoder.conv_norm_out.weight", "decoder.conv_out.weight"):
        assert key in sd, key
    assert "decoder.up_blocks.3.upsamplers.0.conv.weight" not in sd and sd["decoder.conv_out.weight"].shape == (3, 128, 3, 3)
    whole = dict(sd, **{"encoder.conv_in.weight": torch.zeros(1), "quant_conv.bias": torch.zeros(8)})      # a whole AutoencoderKL
    b.load_state_dict(whole)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in sd.items())


def test_head_sizes_refused_before_launch():
    lib = _C.load()

    def att(D, dtype):
        return lib.st_attention(P, P, P, P, 1, 64, 64, 1, D, D, D, D, D, 0.125, dtype, None)

    assert att(512, _C.ST_F32) != 0 and b"head_dim" in lib.st_last_error()
    assert att(256, _C.ST_BF16) != 0 and b"head_dim" in lib.st_last_error()
