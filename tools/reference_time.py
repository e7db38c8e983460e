"""What reference-only control costs on SDXL-base bf16 (synthetic weights), in one process on one device.

1. The joint-attention launch at SDXL's two self-attention site shapes with the loop's rows, B = 3 = [negative | positive | reference],
   lead = 2 (T = S1 = S2 = 4096 with 10 heads, 1024 with 20), q / k / v column slices of one fused buffer as the UNet leaves them:
     (i)   ops.attention_joint: one launch, the second source read in place;
     (ii)  ops.attention on the two lead rows over a PRE-concatenated contiguous K / V (the concatenation is not timed) plus
           ops.attention on the reference row: the same MFMA and exponent work as (i), which differs only in loader addresses;
     (iii) the slow path (fused=False): the concatenation, the two launches, the batch concatenation of their results.
   Each variant is a captured graph of --launches calls; the three graphs are replayed in turn, (i) (ii) (iii) (i) ..., device events
   around a replay, after one warm-up round; medians over --runs with min and max, in microseconds per call.
2. ms/step of the guided Euler loop at 1024 x 1024 (latent 128), batch 1, --steps steps: the loop built without `reference`, the
   reference loop on, and the reference loop gated off (`set_reference(None)`: the reference rows are still evaluated, the sites run
   ordinary attention); the captured loop graphs are replayed in turn, host clock around a device synchronise.

    python tools/reference_time.py [--spec sdxl|tiny] [--steps 20] [--runs 7] [--out profiles/reference_time.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from stabletriton_amd import ops, synth  # noqa: E402
from stabletriton_amd.optimization import optimize_model  # noqa: E402
from stabletriton_amd.pipeline import DenoiseLoop  # noqa: E402
from stabletriton_amd.scheduler import euler_discrete_tables  # noqa: E402
from stabletriton_amd.unet import SDXL_BASE, TINY, UNet2DConditionModel  # noqa: E402


def build(spec, dt, dev):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def graph_of(fn, dev, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize(dev)
    return g


def replay_us(g, dev, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / n * 1e3


def site(T, H, dev, dt, runs, launches):
    B, lead, C = 3, 2, H * 64
    scale = 64 ** -0.5
    fused = (synth.normal(f"reference_time.qkv{T}", (B, T, 3 * C), 3, dev)).to(dt)
    q, k, v = fused[..., :C], fused[..., C:2 * C], fused[..., 2 * C:]
    kcat = torch.cat([k[:lead], k[lead:].expand(lead, -1, -1)], dim=1).contiguous()
    vcat = torch.cat([v[:lead], v[lead:].expand(lead, -1, -1)], dim=1).contiguous()
    variants = {
        "joint": lambda: ops.attention_joint(q, k, v, k[lead:], v[lead:], H, scale, lead=lead),
        "preconcatenated": lambda: (ops.attention(q[:lead], kcat, vcat, H, scale), ops.attention(q[lead:], k[lead:], v[lead:], H, scale)),
        "slow_path": lambda: ops.attention_joint(q, k, v, k[lead:], v[lead:], H, scale, lead=lead, fused=False),
    }
    want = variants["slow_path"]()
    same = bool(torch.equal(variants["joint"](), want))
    pre = variants["preconcatenated"]()
    same = same and bool(torch.equal(torch.cat(pre, dim=0), want))
    graphs = {name: graph_of(fn, dev, launches) for name, fn in variants.items()}
    times = {name: [] for name in variants}
    for i in range(runs + 1):                                      # (round 0 warms up)
        for name, g in graphs.items():
            t = replay_us(g, dev, launches)
            if i:
                times[name].append(t)
    out = {"T": T, "H": H, "B": B, "lead": lead, "bits_equal": same}
    for name, ts in times.items():
        out[f"{name}_us"] = round(statistics.median(ts), 2)
        out[f"{name}_min_max"] = [round(min(ts), 2), round(max(ts), 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    with torch.no_grad():
        sites = [site(T, H, dev, dt, args.runs, args.launches) for T, H in (((4096, 10), (1024, 20)) if args.spec == "sdxl" else ((256, 2),))]
        spec, side = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 32)
        gm = optimize_model(build(spec, dt, dev), cuda_graph=False, reference_layers=(".*",))
        x = synth.denoise_inputs(2, side, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
        cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
        kw = dict(cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim, guidance_scale=5.0, mode="loop")
        plain = DenoiseLoop(gm, 1, side, dt, dev, euler_discrete_tables(args.steps), **kw)
        ref = DenoiseLoop(gm, 1, side, dt, dev, euler_discrete_tables(args.steps), reference=True, **kw)
        for loop in (plain, ref):
            loop.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
        noise = synth.normal("reference_time.noise", (1, 4, side, side), 7, dev)
        init = synth.normal("reference_time.init", (1, 4, side, side), 8, dev) * 0.8
        rnoise = synth.normal("reference_time.rnoise", (1, 4, side, side), 9, dev)
        names = ("plain", "reference_on", "reference_off")
        times = {k: [] for k in names}
        finals = {k: [] for k in names}
        for i in range(args.runs + 1):                             # (round 0 captures and warms both graphs up)
            for name, loop, on in ((names[0], plain, None), (names[1], ref, True), (names[2], ref, False)):
                if on is not None:
                    loop.set_reference(*((init, rnoise) if on else (None,)))
                loop.set_noise(noise)
                t = timed(lambda: loop.run_steps(args.steps), dev)
                finals[name].append(loop.latent.clone())
                if i:
                    times[name].append(t / args.steps)
        finite = all(bool(torch.isfinite(v).all()) for vs in finals.values() for v in vs)
        repeats = {k: all(bool(torch.equal(v, vs[0])) for v in vs) for k, vs in finals.items()}
    med = {k: statistics.median(v) for k, v in times.items()}
    line = json.dumps({
        "tool": "reference_time", "spec": args.spec, "dtype": "bf16", "latent": side, "batch": 1, "guided": True, "steps": args.steps,
        "runs": args.runs, "launches_per_graph": args.launches, "sites": sites, "reference_sites": gm.rewrite_stats["reference_sites"],
        **{f"{k}_ms_per_step": round(med[k], 4) for k in names},
        **{f"{k}_min_max": [round(min(times[k]), 4), round(max(times[k]), 4)] for k in names},
        "on_over_plain": round(med[names[1]] / med[names[0]], 4), "off_over_plain": round(med[names[2]] / med[names[0]], 4),
        "on_changes_the_result": not bool(torch.equal(finals[names[1]][0], finals[names[2]][0])),
        **{f"{k}_repeats_its_bits": repeats[k] for k in names}, "finite": finite})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
