"""DecoderXL compiled by optimize_model against the same module evaluated eagerly in float64 on the CPU from the bf16-rounded
weights (synthetic, seeded), through vae.decode, at latents 16 x 16 and 24 x 16 (T = 384 tokens in the attention), B = 1 and 2.

The figure is max |out - ref| / max |ref|.  Its bound is not tests/test_unet_gpu.py's constant (that one belongs to the golden
fixtures of the tiny UNet): it is twice the same figure of an EAGER bf16 torch run of the same module on the same card, measured in
the test itself - the margin for one more rounding per fused epilogue - and never read from the compiled output.
Measured on the MI355X (compiled / eager bf16, bound = 2 x eager): 16 x 16 B = 1 0.0261 / 0.0469, B = 2 0.0299 / 0.0469;
24 x 16 B = 1 0.0211 / 0.0393, B = 2 0.0264 / 0.0393."""
import copy
import functools

import pytest
import torch

from stabletriton_amd import ops, vae
from stabletriton_amd.optimization import optimize_model

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=1)
def _modules(gpu):
    torch.manual_seed(1234)
    eager = vae.DecoderXL().eval().to(gpu, torch.bfloat16)
    ref64 = copy.deepcopy(eager).to("cpu", torch.float64)          # the bf16-rounded weights, exactly
    return eager, ref64, optimize_model(eager, cuda_graph=False)


@functools.lru_cache(maxsize=2)
def _problem(gpu, hw):
    """latent (B = 2), float64 reference, and the eager bf16 run's error: once per latent size."""
    eager, ref64, _ = _modules(gpu)
    latent = torch.randn((2, 4, *hw), generator=torch.Generator().manual_seed(hw[0])) * vae.SCALING_FACTOR
    ref = vae.decode(ref64, (latent.to(torch.bfloat16) / vae.SCALING_FACTOR).to(torch.bfloat16).double(), 1.0)
    e = vae.decode(eager, latent.to(gpu, torch.bfloat16)).double().cpu()
    return latent, ref, ((e - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("hw", [(16, 16), (24, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_against_float64(gpu, monkeypatch, hw, batch):
    _, _, compiled = _modules(gpu)
    latent, ref, eager_err = _problem(gpu, hw)
    seen = []
    plain = ops.attention
    monkeypatch.setattr(ops, "attention", lambda q, k, v, num_heads, scale: seen.append((num_heads, q.shape[-1])) or plain(q, k, v, num_heads, scale))
    out = vae.decode(compiled, latent[:batch].to(gpu, torch.bfloat16))
    assert out.shape == (batch, 3, 8 * hw[0], 8 * hw[1]) and out.dtype == torch.bfloat16
    assert seen == [(1, 512)], "the middle block's attention did not take ops.attention as one 512-channel head"
    err = ((out.double().cpu() - ref[:batch]).abs().max() / ref.abs().max()).item()
    print(f"VAE {hw} B={batch}: compiled {err:.5f}, eager bf16 {eager_err:.5f} of max |ref| = {ref.abs().max().item():.3f}")
    assert err <= 2.0 * eager_err
