"""What the T2I-Adapter residual sites cost per step on SDXL-base bf16 at 1024 x 1024 (latent 128), bs = 1, guided (2 UNet rows),
mode loop: three variants of the captured loop, same weights, alternated in one process.

    python tools/t2i_adapter_time.py [--spec sdxl|tiny] [--steps 50] [--runs 5] [--out t2i_adapter_time.json]

One JSON object:
  a_ms_per_step   (a) a UNet compiled WITHOUT sites: the default graph
  b_ms_per_step   (b) sites compiled in, scale 0: four launches per step that read their scale and leave;  b_minus_a_ms
  c_ms_per_step   (c) sites on (scale 0.8 on every step);                                                   c_minus_a_ms
  *_min_max       min and max over the runs: the spread the deltas are to be read against
  floor_us        the sites' own traffic - x read and written, the features read: 3 x tensor bytes - at 6.3 TB/s
  kernel          per site: the launch alone (with the producer's statistics geometry, 256 rows per tile), microseconds per launch
                  from device events around one replay of a graph of --kernel-iters launches (buffers resident in the caches; the
                  boundary between two launches is inside the figure), its floor, and the ratio
Each run is one replay of the loop graph (host clock around a device synchronise) after one warm-up replay of each; medians
over --runs.
"""
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

HBM_ACHIEVABLE = 6.3e12      # bytes / s


def build(spec, dt, dev):
    with torch.device("meta"):
        m = UNet2DConditionModel(spec)
    m = m.to_empty(device=dev).to(dt).eval().requires_grad_(False)
    synth.fill_module_(m, 0)
    return m


def make_loop(gm, spec, latent, dt, dev, steps, x):
    loop = DenoiseLoop(gm, 1, latent, dt, dev, euler_discrete_tables(steps), cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim,
                       guidance_scale=5.0, mode="loop")
    cond = [x[k].to(dt) for k in ("encoder_hidden_states", "text_embeds", "time_ids")]
    loop.set_conditioning(*(c[1:2] for c in cond), *(c[0:1] for c in cond))
    return loop


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def kernel_alone(shapes, rows, dt, dev, iters):
    """The launch by itself at every site's shape, scale on, statistics rewritten."""
    out = []
    table = torch.full((1,), 0.8, dtype=torch.float32, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for c, h, w in shapes:
        x = torch.zeros((rows, c, h, w), dtype=dt, device=dev).contiguous(memory_format=torch.channels_last)
        f = torch.ones((1, c, h, w), dtype=dt, device=dev).contiguous(memory_format=torch.channels_last)
        srows = 256 if (h * w) % 256 == 0 else 0
        stats = ops.ColStats(torch.zeros((rows * h * w // srows, c, 2), dtype=torch.float32, device=dev), srows, c) if srows else None
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                ops.residual_add(x, f, table, step, stats)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()                                 # (captured: the host's launch rate is not what is measured)
        with torch.cuda.graph(g):
            for _ in range(iters):
                ops.residual_add(x, f, table, step, stats)
        g.replay()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        g.replay()
        end.record()
        torch.cuda.synchronize(dev)
        us = start.elapsed_time(end) * 1e3 / iters
        floor = 3 * rows * c * h * w * x.element_size() / HBM_ACHIEVABLE * 1e6
        out.append({"shape": [rows, c, h, w], "us_per_launch": round(us, 2), "floor_us": round(floor, 2), "ratio": round(us / floor, 2)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spec", choices=("sdxl", "tiny"), default="sdxl")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    spec, latent = (SDXL_BASE, 128) if args.spec == "sdxl" else (TINY, 16)
    m = build(spec, dt, dev)
    x = synth.denoise_inputs(2, latent, 1234, device=dev, cross_dim=spec.cross_dim, pooled_dim=spec.pooled_dim)
    noise = x["latent"][:1]
    without = optimize_model(m, cuda_graph=False)
    sites = optimize_model(m, cuda_graph=False, t2i_adapter=True)
    shapes = sites.t2i_adapter.site_shapes(latent)
    feats = [synth.normal(f"t2i.time.{k}", (1, c, h, w), k).to(dev, dt) for k, (c, h, w) in enumerate(shapes)]
    times = {"a": [], "b": [], "c": []}
    finite = True
    with torch.no_grad():
        l_a = make_loop(without, spec, latent, dt, dev, args.steps, x)
        l_s = make_loop(sites, spec, latent, dt, dev, args.steps, x)
        for i in range(args.runs + 1):                             # (round 0 captures and warms both graphs up)
            for name in ("a", "b", "c"):
                loop = l_a if name == "a" else l_s
                if name == "b":
                    loop.set_t2i_adapter(None)
                elif name == "c":
                    loop.set_t2i_adapter(feats, 0.8)
                loop.set_noise(noise)
                t = timed(lambda: loop.run_steps(args.steps), dev)
                finite = finite and bool(torch.isfinite(loop.latent).all())
                if i:
                    times[name].append(t / args.steps)
        kernel = kernel_alone(shapes, 2, dt, dev, args.kernel_iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    elems = 2 * sum(c * h * w for c, h, w in shapes)
    res = {"tool": "t2i_adapter_time", "spec": args.spec, "dtype": "bf16", "latent": latent, "unet_rows": 2, "steps": args.steps,
           "runs": args.runs, "sites": [list(s) for s in shapes], "finite": finite,
           "floor_us": round(3 * elems * 2 / HBM_ACHIEVABLE * 1e6, 2), "kernel": kernel}
    for k in ("a", "b", "c"):
        res[f"{k}_ms_per_step"] = round(med[k], 4)
        res[f"{k}_min_max"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
    res["b_minus_a_ms"] = round(med["b"] - med["a"], 4)
    res["c_minus_a_ms"] = round(med["c"] - med["a"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
