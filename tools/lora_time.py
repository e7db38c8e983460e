"""What one LoRA scale change costs on SDXL-base bf16: `DenoiseLoop.set_lora_scale` with a synthetic adapter on every
transformer-block Linear (attention projections, feed-forward, proj_in / proj_out), at rank 16 and at rank 128.

    python tools/lora_time.py [--ranks 16 128] [--runs 7] [--spec sdxl|tiny] [--convs] [--dora] [--form lora|loha|lokr] [--out lora_time.json]

`--convs` puts the adapter on EVERY Linear and every Conv2d of the UNet (LoCon; `load_lora(convs=True)`), `--dora` gives every
adapted module a magnitude, so that the merge is the two-launch DoRA form (row norms, then the merge).  `--form loha` / `--form lokr`
make the synthetic adapter a LoHa (two rank-r pairs per module) or a LoKr (w1 full at LyCORIS's default factorisation - the largest
divisors at most sqrt(N), sqrt(K) - and w2 a rank-r product) on the same module sets (`load_lora(lycoris=True)`).

Per rank, one JSON object:
  kernel_ms        the grouped merge launch alone (device events), and `floor_ms`: its own traffic - bytes of base read plus
                   weight written, from the target list - at 6.3 TB/s, the achievable HBM rate
  call_ms          the whole `set_lora_scale` call: scale-table copy, merge, version bumps, derived-weight refresh, and the
                   loop's hoisted text K/V and time tables recomputed in place (`rederive_ms`: that last part alone)
                   with --dora the two launches together; `norm_read_gb` is what the norm pass adds to the traffic (the base
                   read once more; its partial sums are 1/64 of that), counted in `floor_ms`
  torch_merge_ms   the same update the old way: per module `W.copy_(base + s * up @ down)` in torch (plain adapters only: null with --dora or another --form, as is torch_route_ms)
  torch_route_ms   ... followed by `refresh_weights()`, the surface before load_lora existed (which left the hoisted K/V and
                   the time tables to the next set_conditioning)
The two routes alternate in one process, host clock around a device synchronise, after one warm-up of each; medians.
Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from stabletriton_amd import lora, ops, synth  # noqa: E402
from stabletriton_amd.optimization import optimize_model  # noqa: E402
from stabletriton_amd.pipeline import DenoiseLoop  # noqa: E402
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel  # noqa: E402

HBM_ACHIEVABLE = 6.3e12      # bytes / s


def _divisor(n):
    return max(d for d in range(1, math.isqrt(n) + 1) if n % d == 0)


def synthetic_adapter(targets, rank, seed, device, everything=False, dora=False, form="lora"):
    """On the transformer-block Linears, or with `everything` on every module of `targets`; with `dora` a magnitude per module;
    `form`: plain LoRA / LoCon factors, LoHa pairs, or LoKr tables (w2 factorised)."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for name, mod in targets.items():
        if not everything and "attentions" not in name:
            continue
        shape = tuple(mod.weight.shape)
        r = min(rank, shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1))
        rn = lambda *s: torch.randn(s, generator=g, device=device)                  # noqa: E731
        k = math.prod(shape[1:])
        if form == "loha":
            for m in "12":
                sd[f"unet.{name}.hada_w{m}_a"], sd[f"unet.{name}.hada_w{m}_b"] = rn(shape[0], r) * 0.15, rn(r, k) * 0.15
        elif form == "lokr":
            a, b = _divisor(shape[0]), _divisor(shape[1])
            sd[f"unet.{name}.lokr_w1"] = rn(a, b) * 0.1
            sd[f"unet.{name}.lokr_w2_a"], sd[f"unet.{name}.lokr_w2_b"] = rn(shape[0] // a, r) * 0.1, rn(r, k // b) * 0.1
            sd[f"unet.{name}.alpha"] = torch.tensor(float(r))
        else:
            sd[f"unet.{name}.lora_A.weight"] = rn(r, *shape[1:]) * 0.02
            sd[f"unet.{name}.lora_B.weight"] = rn(shape[0], r, *([1, 1] if len(shape) == 4 else [])) * 0.02
        if dora:
            sd[f"unet.{name}.lora_magnitude_vector"] = mod.weight.detach().float().reshape(shape[0], -1).norm(dim=1)
    return sd


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--convs", action="store_true", help="adapt every Linear and every Conv2d (LoCon)")
    ap.add_argument("--dora", action="store_true", help="give every adapted module a DoRA magnitude")
    ap.add_argument("--form", choices=("lora", "loha", "lokr"), default="lora", help="the factorisation of the synthetic adapter")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    spec, latent = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 16)
    with torch.device("meta"):
        m = UNet2DConditionModel(spec)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    gm = optimize_model(m, cuda_graph=False)
    x = synth.denoise_inputs(2, latent, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    loop = DenoiseLoop(gm, 1, latent, dt, dev, mode="loop", guidance_scale=5.0, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    ls = lora.attach(gm)
    results = []
    with torch.no_grad():
        loop.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
        for rank in args.ranks:
            sd = synthetic_adapter(ls.targets if args.convs else ls.linears, rank, rank, dev, everything=args.convs, dora=args.dora,
                                   form=args.form)
            load_ms = timed(lambda: loop.load_lora("probe", sd, 1.0, convs=args.convs, lycoris=args.form != "lora"), dev)
            mods = ls.adapted_modules()
            weight_bytes = sum(ls.targets[n].weight.numel() * ls.targets[n].weight.element_size() for n in mods)
            norm_read = weight_bytes if args.dora else 0             # the norm pass reads every base once more
            traffic = 2 * weight_bytes + norm_read
            ad = ls._adapters["probe"]
            no_torch = args.dora or args.form != "lora"           # (no do-it-yourself route to compare with: both figures are null)
            old_way = [] if no_torch else [(lora.weight_rows(ls.targets[n].weight)[0], ls._base[n], ad.factors[n].tensors[0],
                                            ad.factors[n].tensors[1].t().contiguous()) for n in mods]

            def torch_merge(s):
                for w, base, up, down in old_way:
                    w.copy_(base + s * up @ down)

            def torch_route(s):
                torch_merge(s)
                loop.refresh_weights()

            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            kernel, call, rederive, t_merge, t_route = [], [], [], [], []
            for i in range(args.runs + 1):                         # (round 0 warms both routes up)
                s = 0.5 + 0.05 * i
                c = timed(lambda: loop.set_lora_scale("probe", s), dev)
                ev[0].record()
                ops.lora_merge(ls._plan, ls._scales)
                ev[1].record()
                torch.cuda.synchronize(dev)
                k = ev[0].elapsed_time(ev[1])
                r = timed(loop._rederive_conditioning, dev)
                tm = None if no_torch else timed(lambda: torch_merge(s), dev)
                tr = None if no_torch else timed(lambda: torch_route(s), dev)
                if i:
                    kernel.append(k); call.append(c); rederive.append(r); t_merge.append(tm); t_route.append(tr)
            finite = all(bool(torch.isfinite(t).all()) for t in loop.ctx)
            loop.unload_lora("probe")
            med = statistics.median
            results.append({"rank": rank, "modules": len(mods), "convs": args.convs, "dora": args.dora, "form": args.form,
                            "traffic_gb": round(traffic / 1e9, 3), "norm_read_gb": round(norm_read / 1e9, 3),
                            "floor_ms": round(traffic / HBM_ACHIEVABLE * 1e3, 3), "kernel_ms": round(med(kernel), 3),
                            "kernel_ms_min": round(min(kernel), 3), "kernel_x_floor": round(med(kernel) / (traffic / HBM_ACHIEVABLE * 1e3), 2),
                            "call_ms": round(med(call), 2), "rederive_ms": round(med(rederive), 2),
                            "torch_merge_ms": None if no_torch else round(med(t_merge), 2),
                            "torch_route_ms": None if no_torch else round(med(t_route), 2),
                            "load_ms": round(load_ms, 1), "finite": finite})
    line = json.dumps({"tool": "lora_time", "spec": args.spec, "dtype": "bf16", "runs": args.runs, "results": results})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
