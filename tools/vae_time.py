"""What the compiled SDXL VAE decoder costs beside the same DecoderXL run eagerly by torch, and what the head_dim 512 attention
kernel (csrc/attention_d512.hip) costs beside torch's scaled_dot_product_attention on the same tensors: one process, one device, bf16.

    python tools/vae_time.py [--rounds 7] [--latent 128] [--out profiles/vae_time.json]

decode: vae.decode of a (1, 4, latent, latent) latent, synthetic seeded weights, compiled with optimize_model(cuda_graph=False)
against the eager module.  attention: ops.attention on q, k, v as column slices of one (1, T, 1536) buffer (the fused projection's
rows), T = S = latent^2, one head of 512, against F.scaled_dot_product_attention on the same slices viewed as (1, 1, T, 512).
Each figure is device time between two events around one call; the two sides of a pair run in turn, compiled, eager, compiled ...,
after one warm-up round; medians over --rounds with min and max, and the ratio eager / compiled (torch / kernel) of the medians.
Not measured: other batches and latent sizes, fp16, a captured graph of the decode, published weights."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from stabletriton_amd import ops, vae  # noqa: E402
from stabletriton_amd.optimization import optimize_model  # noqa: E402


def call_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def pair(fns, rounds, dev):
    times = {name: [] for name in fns}
    for i in range(rounds + 1):                                    # (round 0 warms up)
        for name, fn in fns.items():
            ms = call_ms(fn, dev)
            if i:
                times[name].append(ms)
    out = {}
    for name, t in times.items():
        out[f"{name}_ms"] = round(statistics.median(t), 3)
        out[f"{name}_min_max"] = [round(min(t), 3), round(max(t), 3)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T = args.latent * args.latent
    with torch.no_grad():
        torch.manual_seed(1234)
        eager = vae.DecoderXL().eval().to(dev, torch.bfloat16)
        compiled = optimize_model(eager, cuda_graph=False)
        latent = torch.randn((1, 4, args.latent, args.latent), device=dev) * vae.SCALING_FACTOR
        dec = pair({"compiled": lambda: vae.decode(compiled, latent), "eager": lambda: vae.decode(eager, latent)}, args.rounds, dev)
        dec["eager_over_compiled"] = round(dec["eager_ms"] / dec["compiled_ms"], 3)
        qkv = torch.randn((1, T, 1536), device=dev).to(torch.bfloat16)
        q, k, v = qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:]
        att = pair({"kernel": lambda: ops.attention(q, k, v, 1, 512 ** -0.5),
                    "torch_sdpa": lambda: F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])}, args.rounds, dev)
        att["torch_over_kernel"] = round(att["torch_sdpa_ms"] / att["kernel_ms"], 3)
        att["kernel_tflops"] = round(4.0 * T * T * 512 / (att["kernel_ms"] * 1e-3) / 1e12, 1)
        diff = (ops.attention(q, k, v, 1, 512 ** -0.5).float() - F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0].float()).abs().max()
        att["max_abs_difference"] = float(diff)
    line = json.dumps({"tool": "vae_time", "dtype": "bf16", "batch": 1, "latent": args.latent, "tokens": T, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(dev), "decode": dec, "attention": att})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
